"""Golden vectors of the reference's DPMPP2SAncestralSampler and LinearMultistepSampler (sgm/modules/diffusionmodules/sampling.py:350-387,
276-311; sampling_utils.py:12-36), CPU fp32.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_highorder.py

Writes tests/golden/sampler_highorder.npz.  Neither class runs in the reference as written: BaseDiffusionSampler.denoise returns (denoised,
rgb_list) and DPMPP2SAncestralSampler.sampler_step uses that tuple as a tensor; LinearMultistepSampler unpacks two values from a denoiser
that returns four.  The DPM++ 2S subclass below overrides ONLY `denoise`, to return element [0]; the denoiser handed to the linear multistep
sampler returns the pair its line unpacks.  Every arithmetic line that runs is the reference's.  Around them: the reference's
DiscreteDenoiser configured as in make_golden.py::case_sampler, both guiders, 12 and 4 steps, and the settings

    2s  e10   eta 1.0, s_noise 1.0
    2s  e06   eta 0.6, s_noise 1.05
    2s  e15   eta 1.5, s_noise 1.0     sigma_up is clamped to sigma_next on the steep rows: sigma_down = 0 there, one evaluation (asserted below)
    lms o4 / o3 / o1                   order 4, 3, 1

The noise: `noise_sampler` is assigned a function returning row k of a stored tensor z [12, 1, 4, 8, 8] (drawn once with a seeded CPU
torch.Generator) at its k-th call; the reference draws once per step, the last included.

Stored: the inputs and z; per solver, guider, step count and setting the final latent of the reference's own __call__ and, at 12 steps,
every intermediate x (DPM++ 2S: the reference's sampler_step driven by the lines of AncestralSampler.__call__; linear multistep: the lines of
its __call__ restated here around the reference's linear_multistep_coeff and to_d; both asserted bit-equal to __call__'s result); the
sigmas handed to the denoiser, in call order (the quantisation happens behind them, inside the denoiser); per step of DPM++ 2S
(sigma_down, sigma_up, sigma_mid, mult1..4, single) in the reference's expressions; the reference's linear multistep coefficients as it
computes them (scipy's quad on the fp32 sigmas; float64).  Printed: those coefficients against cd360.sampler.lms_coefficients.

The network is tests/test_dpmpp2m_cpu.py::row_network (the three CFG branches differ pairwise; asserted by make_golden_dpmpp2m.py).
"""
from __future__ import annotations

import os
import sys

os.environ["MKL_CBWR"] = "COMPATIBLE"  # MKL's reproducible code path, as tests/conftest.py sets it for the suite

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.dirname(HERE)]
import refshim  # noqa: E402
import weights as W  # noqa: E402

ns = refshim.import_reference()
from test_dpmpp2m_cpu import GUIDERS, row_network  # noqa: E402

torch.set_grad_enabled(False)
torch.set_num_threads(8)
DISC = {"target": "sgm.modules.diffusionmodules.discretizer.LegacyDDPMDiscretization"}
SETTINGS = {"e10": (1.0, 1.0), "e06": (0.6, 1.05), "e15": (1.5, 1.0)}  # (eta, s_noise)
ORDERS = (4, 3, 1)
MAX_STEPS = 12
SINGLE_E15 = {12: [0, 1, 2, 3, 4, 8, 9, 10, 11], 4: None}  # the one-evaluation rows at eta 1.5 (4 steps: recorded, asserted to hold an interior row)
SU = ns.sampling  # (sampling.py imports get_ancestral_step, linear_multistep_coeff, to_d, to_sigma from sampling_utils)


class RunnableDPMPP2S(ns.sampling.DPMPP2SAncestralSampler):
    def denoise(self, x, denoiser, sigma, cond, uc):
        return super().denoise(x, denoiser, sigma, cond, uc)[0]


def stored_noise(z):
    calls = iter(range(z.shape[0]))
    return lambda x: z[next(calls)].expand_as(x).clone()


def main():
    den = ns.denoiser.DiscreteDenoiser(
        weighting_config={"target": "sgm.modules.diffusionmodules.denoiser_weighting.EpsWeighting"},
        scaling_config={"target": "sgm.modules.diffusionmodules.denoiser_scaling.EpsScaling"}, num_idx=1000, discretization_config=DISC)
    b, n = 1, 2
    x0 = W.tensor("x", (b, 4, 8, 8), seed=8)
    c = {"crossattn": W.tensor("c_ctx", (b + b * n, 7, 16), seed=8), "vector": W.tensor("c_vec", (b + b * n, 12), seed=8)}
    uc = {"crossattn": W.tensor("uc_ctx", (b + b * n, 7, 16), seed=8), "vector": W.tensor("uc_vec", (b + b * n, 12), seed=8)}
    z = torch.randn(MAX_STEPS, 1, 4, 8, 8, generator=torch.Generator().manual_seed(362))
    seen = []

    def denoiser(inp, sigma, cc):
        seen.append(sigma[0].clone())
        return den(row_network, inp, sigma, cc)

    def denoiser2(inp, sigma, cc, **kw):  # the pair LinearMultistepSampler.__call__ unpacks
        res = denoiser(inp, sigma, cc, **kw)
        return res[0], res[3]

    out = dict(x=x0, z=z, **{"c_" + k: v for k, v in c.items()}, **{"uc_" + k: v for k, v in uc.items()})
    for name, gcfg in GUIDERS.items():
        for steps in (12, 4):
            # ---- DPM++ 2S ancestral
            for tag, (eta, s_noise) in SETTINGS.items():
                smp = RunnableDPMPP2S(eta=eta, s_noise=s_noise, discretization_config=DISC, num_steps=50, guider_config=gcfg, device="cpu")
                smp.noise_sampler = stored_noise(z)
                final = smp(denoiser, x0.clone(), c, uc=uc, num_steps=steps)
                # the same walk, step by step (the lines of AncestralSampler.__call__), keeping every intermediate
                del seen[:]
                smp.noise_sampler = stored_noise(z)
                x, s_in, sigmas, num_sigmas, cond, ucond = smp.prepare_sampling_loop(x0.clone(), c, uc, steps)
                xs, rows = [], []
                for i in range(num_sigmas - 1):
                    s, sn = s_in * sigmas[i], s_in * sigmas[i + 1]
                    before = len(seen)
                    x = smp.sampler_step(s, sn, denoiser, x, cond, ucond)
                    single = len(seen) - before == 1
                    sd, su = SU.get_ancestral_step(s, sn, eta=eta)
                    assert single == bool(torch.sum(sd) < 1e-14)
                    if single:
                        mid, mult = torch.zeros(1), [torch.zeros(1)] * 4
                    else:
                        h, sm, t, t_next = smp.get_variables(s, sd)
                        mid, mult = SU.to_sigma(sm), smp.get_mult(h, sm, t, t_next)
                        assert torch.equal(seen[-1], mid[0])  # the second evaluation was handed to_sigma(s), un-snapped
                    xs.append(x.clone())
                    rows.append(torch.cat([sd, su, mid, *mult, torch.tensor([float(single)])]))
                assert torch.equal(x, final), (name, steps, tag)
                rows = torch.stack(rows)
                singles = [i for i in range(steps) if rows[i, 7] > 0]
                assert len(seen) == 2 * steps - len(singles) and singles[-1] == steps - 1
                if tag == "e15":
                    assert any(i < steps - 1 for i in singles), "eta 1.5 is here for its interior one-evaluation rows"
                    if SINGLE_E15[steps] is not None:
                        assert singles == SINGLE_E15[steps], singles
                    print(f"2s e15 {steps} steps: one-evaluation rows {singles}")
                else:
                    assert singles == [steps - 1], (tag, singles)
                key = f"2s_{name}_{steps}_{tag}"
                out[key] = final
                if steps == 12:  # (the 4-step intermediates are dropped: the size class of sampler_euler_a.npz)
                    out[key + "_x"] = torch.stack(xs)
                out[f"2s_{steps}_{tag}_dsig"] = torch.stack(seen)
                out[f"2s_tab_{steps}_{tag}"], out[f"sigmas_{steps}"] = rows, sigmas
            # ---- linear multistep
            for order in ORDERS:
                smp = ns.sampling.LinearMultistepSampler(order=order, discretization_config=DISC, num_steps=50, guider_config=gcfg, device="cpu")
                final = smp(denoiser2, x0.clone(), c, uc=uc, num_steps=steps)
                del seen[:]
                x, s_in, sigmas, num_sigmas, cond, ucond = smp.prepare_sampling_loop(x0.clone(), c, uc, steps)
                ds, xs, coefs = [], [], np.zeros((steps, 4))
                sigmas_cpu = sigmas.detach().cpu().numpy()
                for i in range(num_sigmas - 1):  # the lines of LinearMultistepSampler.__call__ (sampling.py:294-309)
                    sigma = s_in * sigmas[i]
                    denoised, _ = denoiser2(*smp.guider.prepare_inputs(x, sigma, cond, ucond))
                    denoised = smp.guider(denoised, sigma)
                    d = SU.to_d(x, sigma, denoised)
                    ds.append(d)
                    if len(ds) > smp.order:
                        ds.pop(0)
                    cur_order = min(i + 1, smp.order)
                    coeffs = [SU.linear_multistep_coeff(cur_order, sigmas_cpu, i, j) for j in range(cur_order)]
                    x = x + sum(coeff * d for coeff, d in zip(coeffs, reversed(ds)))
                    coefs[i, :cur_order] = coeffs
                    xs.append(x.clone())
                assert torch.equal(x, final), (name, steps, order)
                assert len(seen) == steps
                key = f"lms_{name}_{steps}_o{order}"
                out[key] = final
                if steps == 12:
                    out[key + "_x"] = torch.stack(xs)
                out[f"lms_{steps}_dsig"] = torch.stack(seen)
                out[f"lms_coef_{steps}_o{order}"] = torch.from_numpy(coefs)
    for a, bb in (("e10", "e06"), ("e10", "e15"), ("e06", "e15")):
        assert float((out[f"2s_cfg3_12_{a}"] - out[f"2s_cfg3_12_{bb}"]).abs().max()) > 1e-2, (a, bb)
    for a, bb in ((4, 3), (4, 1), (3, 1)):
        assert float((out[f"lms_cfg3_12_o{a}"] - out[f"lms_cfg3_12_o{bb}"]).abs().max()) > 1e-2, (a, bb)
    assert float((out["2s_cfg3_12_e10"] - out["2s_cfg2_12_e10"]).abs().max()) > 1e-2
    assert float((out["lms_cfg3_12_o4"] - out["lms_cfg2_12_o4"]).abs().max()) > 1e-2
    assert float((out["2s_cfg3_12_e10"] - out["lms_cfg3_12_o4"]).abs().max()) > 1e-2
    # the reference's coefficients against the product's table (scipy-free Gauss-Legendre): relative to the row's largest coefficient
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "custom-diffusion360_amd"))
    from cd360.sampler import lms_coefficients
    from scipy import integrate
    for steps in (4, 12, 50):
        sig = ns.discretizer.LegacyDDPMDiscretization()(steps)
        t32, t64 = sig.numpy(), sig.numpy().astype(np.float64)
        worst32 = worst64 = 0.0
        equal64 = total = 0
        for order in (1, 2, 3, 4):
            mine = lms_coefficients(sig, order).numpy()
            for i in range(steps):
                cur = min(i + 1, order)
                r32 = np.array([SU.linear_multistep_coeff(cur, t32, i, j) for j in range(cur)])
                r64 = np.array([SU.linear_multistep_coeff(cur, t64, i, j) for j in range(cur)])
                worst32 = max(worst32, float(np.abs(mine[i, :cur] - r32).max() / np.abs(r32).max()))
                worst64 = max(worst64, float(np.abs(mine[i, :cur] - r64.astype(np.float32)).max() / np.abs(r64).max()))
                equal64 += int((mine[i, :cur] == r64.astype(np.float32)).sum())
                total += cur
                assert not mine[i, cur:].any()
        print(f"lms_coefficients, {steps} steps, orders 1-4: vs the reference as it runs (fp32 sigmas in the integrand) max {worst32:.3e} of the row's "
              f"largest; vs quad on float64 sigmas, rounded to fp32: max {worst64:.3e}, {equal64} of {total} bit-equal")
    del integrate
    path = os.path.join(HERE, "sampler_highorder.npz")
    np.savez_compressed(path, **{k: v.detach().cpu().numpy() for k, v in out.items()})
    print(f"sampler_highorder: {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()

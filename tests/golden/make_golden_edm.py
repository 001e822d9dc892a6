"""Golden vectors of the reference's EDM samplers with churn and of its Heun corrector (sgm/modules/diffusionmodules/sampling.py:85-136,
314-337), CPU fp32.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_edm.py

Writes tests/golden/sampler_edm.npz.  The reference's EulerEDMSampler runs as written, churn included.  Its HeunEDMSampler does not:
BaseDiffusionSampler.denoise returns (denoised, rgb_list) and possible_correction_step uses that tuple as a tensor.  The subclass below
overrides ONLY `denoise`, to return element [0] while that method runs; every arithmetic line that runs is the reference's.  Around
them: the reference's DiscreteDenoiser configured as in make_golden.py::case_sampler, both guiders, 12 and 4 steps, and the settings

    euler c1   s_churn 1.0, s_noise 1.003                            un-clamped: gamma = 1/4 at 4 steps, 1/12 at 12
    euler cw   s_churn 40, s_tmin 0.05, s_tmax 10.0, s_noise 1.0     clamped to sqrt 2 - 1, and windowed: row 0 (sigma_max = 14.6) is not churned
    heun  c0   no churn
    heun  cw   as euler cw

The noise: EDMSampler calls torch.randn_like directly, whose stream nobody else can reproduce.  For the duration of each run
torch.randn_like is a function returning row k of a stored tensor z [12, 1, 4, 8, 8] (drawn once with a seeded CPU torch.Generator) at its
k-th call; which steps drew is recorded.

Stored: the inputs and z; per solver, guider, step count and setting the final latent of the reference's own __call__, every intermediate
x (the reference's sampler_step driven by the lines of its forward, asserted bit-equal to __call__'s result), per step
(gamma, sigma_hat, noise_std) and whether the step drew, and the sigmas handed to the denoiser, in call order (2n - 1 for Heun: the
quantisation happens behind them, inside the denoiser).

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
CHURN = {"c0": dict(), "c1": dict(s_churn=1.0, s_noise=1.003), "cw": dict(s_churn=40.0, s_tmin=0.05, s_tmax=10.0, s_noise=1.0)}
RUNS = (("euler", "c1"), ("euler", "cw"), ("heun", "c0"), ("heun", "cw"))
MAX_STEPS = 12


class RunnableHeun(ns.sampling.HeunEDMSampler):
    """`denoise` hands back the tensor alone while possible_correction_step runs (the reference's own lines, which use it as a tensor),
    and the (denoised, rgb_list) pair everywhere else (sampler_step unpacks it)."""

    tensor_only = False

    def denoise(self, x, denoiser, sigma, cond, uc):
        res = super().denoise(x, denoiser, sigma, cond, uc)
        return res[0] if self.tensor_only else res

    def possible_correction_step(self, *args):
        self.tensor_only = True
        try:
            return super().possible_correction_step(*args)
        finally:
            self.tensor_only = False


class stored_noise:
    """torch.randn_like for the duration of the block: row k of z at the k-th call"""

    def __init__(self, z):
        self.z, self.calls = z, 0

    def __call__(self, x, **kw):
        k, self.calls = self.calls, self.calls + 1
        return self.z[k].expand_as(x).clone()

    def __enter__(self):
        self.saved, torch.randn_like = torch.randn_like, self
        return self

    def __exit__(self, *exc):
        torch.randn_like = self.saved


def main():
    den = ns.denoiser.DiscreteDenoiser(
        weighting_config={"target": "sgm.modules.diffusionmodules.denoiser_weighting.EpsWeighting"},
        scaling_config={"target": "sgm.modules.diffusionmodules.denoiser_scaling.EpsScaling"}, num_idx=1000, discretization_config=DISC)
    b, n = 1, 2
    x0 = W.tensor("x", (b, 4, 8, 8), seed=8)
    c = {"crossattn": W.tensor("c_ctx", (b + b * n, 7, 16), seed=8), "vector": W.tensor("c_vec", (b + b * n, 12), seed=8)}
    uc = {"crossattn": W.tensor("uc_ctx", (b + b * n, 7, 16), seed=8), "vector": W.tensor("uc_vec", (b + b * n, 12), seed=8)}
    z = torch.randn(MAX_STEPS, 1, 4, 8, 8, generator=torch.Generator().manual_seed(361))
    seen = []

    def denoiser(inp, sigma, cc):
        seen.append(sigma[0].clone())
        return den(row_network, inp, sigma, cc)

    out = dict(x=x0, z=z, **{"c_" + k: v for k, v in c.items()}, **{"uc_" + k: v for k, v in uc.items()})
    for name, gcfg in GUIDERS.items():
        for steps in (12, 4):
            for solver, tag in RUNS:
                cls = ns.sampling.EulerEDMSampler if solver == "euler" else RunnableHeun
                smp = cls(discretization_config=DISC, num_steps=50, guider_config=gcfg, device="cpu", **CHURN[tag])
                with stored_noise(z) as draws:
                    final, _ = smp(denoiser, x0.clone(), c, uc=uc, num_steps=steps)
                    n_draws = draws.calls
                # the same walk, step by step (the lines of EDMSampler.forward), keeping every intermediate
                del seen[:]
                with stored_noise(z) as draws:
                    x, s_in, sigmas, num_sigmas, cond, ucond = smp.prepare_sampling_loop(x0.clone(), c, uc, steps)
                    xs, rows = [], []
                    for i in range(num_sigmas - 1):
                        gamma = min(smp.s_churn / (num_sigmas - 1), 2 ** 0.5 - 1) if smp.s_tmin <= sigmas[i] <= smp.s_tmax else 0.0
                        before = draws.calls
                        x, _ = smp.sampler_step(s_in * sigmas[i], s_in * sigmas[i + 1], denoiser, x, cond, ucond, gamma)
                        s = s_in * sigmas[i]
                        s_hat = s * (gamma + 1.0)
                        std = (s_hat ** 2 - s ** 2) ** 0.5 if gamma > 0 else torch.zeros(1)
                        xs.append(x.clone())
                        rows.append(torch.stack([torch.tensor(gamma, dtype=torch.float32), s_hat[0], std[0], torch.tensor(float(draws.calls - before))]))
                    assert draws.calls == n_draws
                assert torch.equal(x, final), (name, steps, solver, tag)
                rows = torch.stack(rows)
                assert len(seen) == (2 * steps - 1 if solver == "heun" else steps)
                if tag == "cw":  # clamped and windowed: at least one churned and one un-churned row, row 0 among the latter
                    assert rows[0, 0] == 0 and bool((rows[:, 0] > 0).any()) and float(rows[:, 0].max()) == float(torch.tensor(2 ** 0.5 - 1))
                if tag == "c1":
                    assert bool((rows[:, 0] > 0).all()) and float(rows[0, 0]) == float(torch.tensor(1.0 / steps))
                assert torch.equal(rows[:, 3], (rows[:, 0] > 0).float())
                key = f"{solver}_{name}_{steps}_{tag}"
                out[key] = final
                if steps == 12:  # (the 4-step intermediates are dropped: the size class of sampler_euler_a.npz)
                    out[key + "_x"] = torch.stack(xs)
                out[f"{solver}_{steps}_{tag}_dsig"] = torch.stack(seen)
                out[f"churn_{steps}_{tag}"], out[f"sigmas_{steps}"] = rows, sigmas
    assert float((out["heun_cfg3_12_c0"] - out["heun_cfg2_12_c0"]).abs().max()) > 1e-2
    assert float((out["euler_cfg3_12_c1"] - out["euler_cfg3_12_cw"]).abs().max()) > 1e-2
    assert float((out["heun_cfg3_12_c0"] - out["heun_cfg3_12_cw"]).abs().max()) > 1e-2
    path = os.path.join(HERE, "sampler_edm.npz")
    np.savez_compressed(path, **{k: v.detach().cpu().numpy() for k, v in out.items()})
    print(f"sampler_edm: {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()

"""Golden vectors of the reference's ancestral Euler solver (sgm/modules/diffusionmodules/sampling.py:236-273, 340-347), CPU fp32.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_euler_a.py

Writes tests/golden/sampler_euler_a.npz.  The reference's EulerAncestralSampler does not run in its own fork as written:
BaseDiffusionSampler.denoise returns (denoised, rgb_list) and EulerAncestralSampler.sampler_step uses that tuple as a tensor.  The subclass
below overrides ONLY `denoise`, to return element [0]; every arithmetic line that runs is the reference's.  Around it: the reference's
DiscreteDenoiser configured as in make_golden.py::case_sampler, both guiders, 12 and 4 steps, (eta, s_noise) in {(1.0, 1.0), (0.6, 1.05)}.

The noise: `noise_sampler` is replaced by a closure that returns row i of a stored tensor z [steps, 1, 4, 8, 8] at its i-th call, drawn
once with a seeded CPU torch.Generator -- the reference draws torch.randn_like there, whose stream nobody else can reproduce.

Stored: the inputs and z; per guider, step count and setting the final latent of the reference's own __call__, every intermediate x (the
reference's sampler_step driven by the lines of its __call__, asserted bit-equal to __call__'s result) and the reference's
(sigma_down, sigma_up) per step (get_ancestral_step, sampling_utils.py:27-36).

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
SETTINGS = {"e10": (1.0, 1.0), "e06": (0.6, 1.05)}  # (eta, s_noise)
MAX_STEPS = 12


class RunnableEulerAncestral(ns.sampling.EulerAncestralSampler):
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
    z = torch.randn(MAX_STEPS, 1, 4, 8, 8, generator=torch.Generator().manual_seed(360))
    denoiser = lambda inp, sigma, cc: den(row_network, inp, sigma, cc)  # noqa: E731
    out = dict(x=x0, z=z, **{"c_" + k: v for k, v in c.items()}, **{"uc_" + k: v for k, v in uc.items()})
    for name, gcfg in GUIDERS.items():
        for steps in (12, 4):
            for tag, (eta, s_noise) in SETTINGS.items():
                smp = RunnableEulerAncestral(eta=eta, s_noise=s_noise, discretization_config=DISC, num_steps=50, guider_config=gcfg, device="cpu")
                smp.noise_sampler = stored_noise(z)
                final = smp(denoiser, x0.clone(), c, uc=uc, num_steps=steps)
                # the same walk, step by step (the lines of AncestralSampler.__call__), keeping every intermediate
                smp.noise_sampler = stored_noise(z)
                x, s_in, sigmas, num_sigmas, cond, ucond = smp.prepare_sampling_loop(x0.clone(), c, uc, steps)
                xs, anc = [], []
                for i in range(num_sigmas - 1):
                    s, sn = s_in * sigmas[i], s_in * sigmas[i + 1]
                    x = smp.sampler_step(s, sn, denoiser, x, cond, ucond)
                    sd, su = ns.sampling.get_ancestral_step(s, sn, eta=eta)
                    xs.append(x.clone())
                    anc.append(torch.stack([sd[0], su[0]]))
                assert torch.equal(x, final), (name, steps, tag)
                key = f"{name}_{steps}_{tag}"
                out[key], out[key + "_x"] = final, torch.stack(xs)
                out[f"anc_{steps}_{tag}"], out[f"sigmas_{steps}"] = torch.stack(anc), sigmas
    assert float((out["cfg3_12_e10"] - out["cfg2_12_e10"]).abs().max()) > 1e-2
    assert float((out["cfg3_12_e10"] - out["cfg3_12_e06"]).abs().max()) > 1e-2
    path = os.path.join(HERE, "sampler_euler_a.npz")
    np.savez_compressed(path, **{k: v.detach().cpu().numpy() for k, v in out.items()})
    print(f"sampler_euler_a: {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()

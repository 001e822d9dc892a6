"""Golden vectors of the reference's DPM++ 2M solver (sgm/modules/diffusionmodules/sampling.py:390-465), CPU fp32.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_dpmpp2m.py

Writes tests/golden/sampler_dpmpp2m.npz.  The reference's DPMPP2MSampler does not run in its own fork as written: BaseDiffusionSampler.denoise
returns (denoised, rgb_list) and DPMPP2MSampler.sampler_step multiplies that tuple.  The subclass below overrides ONLY `denoise`, to return
element [0]; every arithmetic line that runs is the reference's.  Around it: the reference's DiscreteDenoiser configured as in
make_golden.py::case_sampler, both guiders, 12 and 4 steps.

Stored: the inputs; per guider and step count the final latent of the reference's own __call__, every intermediate x and denoised (the
reference's sampler_step driven by the lines of its __call__, asserted bit-equal to __call__'s result), and the reference's multipliers per
step ((m3, m4) = (1, 0) where it takes its first-order shortcut, sampling.py:433-435).

The network is tests/test_dpmpp2m_cpu.py::row_network: case_sampler's toy network plus a per-row term.  The toy network alone gives the
image branch the unconditional branch's output (their conditioning rows are both `uc1`), so cfg3 == cfg2 on it and scale_im would never be
exercised; asserted here: the three branches' outputs differ pairwise.
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


class RunnableDPMPP2M(ns.sampling.DPMPP2MSampler):
    def denoise(self, x, denoiser, sigma, cond, uc):
        return super().denoise(x, denoiser, sigma, cond, uc)[0]


def main():
    den = ns.denoiser.DiscreteDenoiser(
        weighting_config={"target": "sgm.modules.diffusionmodules.denoiser_weighting.EpsWeighting"},
        scaling_config={"target": "sgm.modules.diffusionmodules.denoiser_scaling.EpsScaling"}, num_idx=1000, discretization_config=DISC)
    b, n = 1, 2
    x0 = W.tensor("x", (b, 4, 8, 8), seed=8)
    c = {"crossattn": W.tensor("c_ctx", (b + b * n, 7, 16), seed=8), "vector": W.tensor("c_vec", (b + b * n, 12), seed=8)}
    uc = {"crossattn": W.tensor("uc_ctx", (b + b * n, 7, 16), seed=8), "vector": W.tensor("uc_vec", (b + b * n, 12), seed=8)}
    denoiser = lambda inp, sigma, cc: den(row_network, inp, sigma, cc)  # noqa: E731
    out = dict(x=x0, **{"c_" + k: v for k, v in c.items()}, **{"uc_" + k: v for k, v in uc.items()})
    for name, gcfg in GUIDERS.items():
        for steps in (12, 4):
            smp = RunnableDPMPP2M(discretization_config=DISC, num_steps=50, guider_config=gcfg, device="cpu")
            final = smp(denoiser, x0.clone(), c, uc=uc, num_steps=steps)
            # the same walk, step by step (the lines of DPMPP2MSampler.__call__), keeping every intermediate
            x, s_in, sigmas, num_sigmas, cond, ucond = smp.prepare_sampling_loop(x0.clone(), c, uc, steps)
            xs, dens, mults, old = [], [], [], None
            for i in range(num_sigmas - 1):
                prev, s, sn = (None if i == 0 else s_in * sigmas[i - 1]), s_in * sigmas[i], s_in * sigmas[i + 1]
                x, old_next = smp.sampler_step(old, prev, s, sn, denoiser, x, cond, uc=ucond)
                m = smp.get_mult(*smp.get_variables(s, sn, prev), prev)
                first_order = old is None or torch.sum(sn) < 1e-14  # sampling.py:433
                mults.append(torch.stack([m[0][0], m[1][0]] + ([torch.tensor(1.0), torch.tensor(0.0)] if first_order else [m[2][0], m[3][0]])))
                old = old_next
                xs.append(x.clone())
                dens.append(old.clone())
            assert torch.equal(x, final), (name, steps)
            key = f"{name}_{steps}"
            out[key], out[key + "_x"], out[key + "_den"] = final, torch.stack(xs), torch.stack(dens)
            out[f"mult_{steps}"], out[f"sigmas_{steps}"] = torch.stack(mults), sigmas
            if name == "cfg3" and steps == 12:  # the three CFG branches must differ pairwise, or scale_im is never exercised
                xin, sin, cin = smp.guider.prepare_inputs(x0, torch.full((b,), 3.3), c, uc)
                d3 = den(row_network, xin, sin, cin)[0]
                for i, j in ((0, 1), (0, 2), (1, 2)):
                    assert float((d3[i] - d3[j]).abs().max()) > 1e-2, (i, j)
    assert float((out["cfg3_12"] - out["cfg2_12"]).abs().max()) > 1e-2
    path = os.path.join(HERE, "sampler_dpmpp2m.npz")
    np.savez_compressed(path, **{k: v.detach().cpu().numpy() for k, v in out.items()})
    print(f"sampler_dpmpp2m: {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()

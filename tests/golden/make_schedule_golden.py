"""Generate tests/golden/schedules.npz by running the reference's own EDMDiscretization and EulerEDMSampler (CPU, fp32) in this container.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_schedule_golden.py

The reference is imported as make_golden.py imports it (tests/golden/refshim.py); the toy network and the inputs are that generator's
(case_sampler).  The fixture holds arrays only:

    sig_<k> / sig0_<k>     EDMDiscretization(sigma_min, sigma_max, rho)(n) without / with the appended zero, k indexing SETS below
    params                 SETS as an array [4, 4] = (n, sigma_min, sigma_max, rho)
    euler_k80              the final latent of EulerEDMSampler + DiscreteDenoiser (EpsScaling, the legacy 1000-entry table) +
                           ScheduledCFGImgTextRef(7.5, 3.5) over the 4-step schedule (0.002, 80, 7): every sigma off the denoiser's grid,
                           q(sigma_0) / sigma_0 = 0.18
"""
from __future__ import annotations

import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as G  # noqa: E402  (imports the reference through refshim; runs no case on import)
import weights as W  # noqa: E402

SETS = ((4, 0.0292, 14.6146, 3.0), (10, 0.0292, 14.6146, 3.0), (25, 0.0292, 14.6146, 7.0), (4, 0.002, 80.0, 7.0))
EDM = "sgm.modules.diffusionmodules.discretizer.EDMDiscretization"


def case_schedules():
    ns = G.ns
    out = {"params": G.np.asarray(SETS, dtype=G.np.float64)}
    for k, (n, lo, hi, rho) in enumerate(SETS):
        disc = ns.discretizer.EDMDiscretization(sigma_min=lo, sigma_max=hi, rho=rho)
        out[f"sig_{k}"] = disc(n, do_append_zero=False)
        out[f"sig0_{k}"] = disc(n)
    den = ns.denoiser.DiscreteDenoiser(
        weighting_config={"target": "sgm.modules.diffusionmodules.denoiser_weighting.EpsWeighting"},
        scaling_config={"target": "sgm.modules.diffusionmodules.denoiser_scaling.EpsScaling"}, num_idx=1000,
        discretization_config={"target": "sgm.modules.diffusionmodules.discretizer.LegacyDDPMDiscretization"})
    n, lo, hi, rho = SETS[3]
    smp = ns.sampling.EulerEDMSampler(discretization_config={"target": EDM, "params": {"sigma_min": lo, "sigma_max": hi, "rho": rho}}, num_steps=n,
                                      guider_config={"target": "sgm.modules.diffusionmodules.guiders.ScheduledCFGImgTextRef",
                                                     "params": {"scale": 7.5, "scale_im": 3.5}}, device="cpu")
    b, r = 1, 2  # case_sampler's inputs, regenerated (tests/golden/sampler.npz stores the same arrays)
    x = W.tensor("x", (b, 4, 8, 8), seed=8)
    c = {"crossattn": W.tensor("c_ctx", (b + b * r, 7, 16), seed=8), "vector": W.tensor("c_vec", (b + b * r, 12), seed=8)}
    uc = {"crossattn": W.tensor("uc_ctx", (b + b * r, 7, 16), seed=8), "vector": W.tensor("uc_vec", (b + b * r, 12), seed=8)}
    res, _ = smp(lambda inp, sigma, cc: den(G.dummy_network, inp, sigma, cc), x.clone(), c, uc=uc)
    out["euler_k80"] = res
    G.npz("schedules", **out)


if __name__ == "__main__":
    case_schedules()
    assert not os.path.exists(os.path.join(G.refshim.REF_ROOT, "sgm", "__pycache__")), "bytecode leaked into the reference tree"

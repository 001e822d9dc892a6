"""What tests/test_schedules_cpu.py and tests/test_schedules_gpu.py share (plain helper module, like sampler_cases.py; no tests, no
fixtures): the Karras parameter sets of tests/golden/schedules.npz, the two 4-step schedules the GPU file walks, their YAML form and the
loader of the fixture."""
import os

import numpy as np
import torch

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
EDM = "sgm.modules.diffusionmodules.discretizer.EDMDiscretization"
# (n, sigma_min, sigma_max, rho): tests/golden/make_schedule_golden.py::SETS, in the fixture's order
SETS = ((4, 0.0292, 14.6146, 3.0), (10, 0.0292, 14.6146, 3.0), (25, 0.0292, 14.6146, 7.0), (4, 0.002, 80.0, 7.0))
K3, K80 = SETS[0], SETS[3]  # inside the denoiser's table; the reference's defaults, q(sigma_0) / sigma_0 = 0.18
SCHEDULES = {"K3": K3, "K80": K80}
OFF_GRID = ("euler", "heun", "dpmpp2m")
REFUSED = ("euler_a", "dpmpp2s_a", "lms")


def load():
    g = {k: torch.from_numpy(v) for k, v in np.load(os.path.join(GOLD, "schedules.npz")).items()}
    assert g["params"].tolist() == [list(s) for s in SETS]
    return g


def params(s):
    return {"sigma_min": s[1], "sigma_max": s[2], "rho": s[3]}


def config(s):
    """The YAML discretization_config of parameter set s."""
    return {"target": EDM, "params": params(s)}


def karras(s):
    from cd360 import sampler as S
    return S.EDMDiscretization(**params(s))


def one_ulp(a, b):
    """tests/test_sampler_cpu.py's rule for a stored power: at most one float32 ulp of b from b."""
    return a.shape == b.shape and bool(((a - b).abs() <= torch.nextafter(b.abs(), torch.full_like(b, float("inf"))) - b.abs()).all())

"""Generate tests/golden/lr_schedules.npz by running the reference's own sgm/lr_scheduler.py classes in this container.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_lr_schedule_golden.py

The reference's module imports numpy only, so it is loaded by path under a private name (the tree's root is refshim.REF_ROOT).  The fixture
holds float64 arrays only: for every configuration k of CONFIGS[cls] (the dictionaries tests/test_optim_cpu.py imports from here),
`<cls>_<k>` = the multipliers cls(**config).schedule(n) for n = 0 .. N[cls][k].  Each class has a configuration with n below the warm-up
length, one running past the end of the decay (cosine) or onto a cycle boundary and into the next cycle (the two cycle classes), and a
warm-up of zero steps.
"""
from __future__ import annotations

import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

CONFIGS = {
    "LambdaWarmUpCosineScheduler": [
        dict(warm_up_steps=10, lr_min=0.01, lr_max=1.0, lr_start=1e-6, max_decay_steps=50),
        dict(warm_up_steps=0, lr_min=0.1, lr_max=0.7, lr_start=0.3, max_decay_steps=33),
        dict(warm_up_steps=7, lr_min=0.0, lr_max=1.3, lr_start=0.0, max_decay_steps=8),
    ],
    "LambdaWarmUpCosineScheduler2": [
        dict(warm_up_steps=[5, 3], f_min=[0.1, 0.05], f_max=[1.0, 0.5], f_start=[1e-6, 0.01], cycle_lengths=[20, 17]),
        dict(warm_up_steps=[0], f_min=[0.3], f_max=[0.9], f_start=[0.2], cycle_lengths=[13]),
        dict(warm_up_steps=[4, 4, 4], f_min=[0.0, 0.0, 0.0], f_max=[1.0, 0.6, 0.36], f_start=[0.0, 0.1, 0.1], cycle_lengths=[9, 9, 9]),
    ],
    "LambdaLinearScheduler": [
        dict(warm_up_steps=[10000], f_min=[1.0], f_max=[1.0], f_start=[1e-6], cycle_lengths=[10000000000000]),  # the shipped training configs' schedule
        dict(warm_up_steps=[5, 3], f_min=[0.1, 0.05], f_max=[1.0, 0.5], f_start=[1e-6, 0.01], cycle_lengths=[20, 17]),
        dict(warm_up_steps=[0, 2], f_min=[0.0, 0.0], f_max=[1.0, 0.7], f_start=[1.0, 0.3], cycle_lengths=[6, 11]),
    ],
}
N = {"LambdaWarmUpCosineScheduler": [60, 40, 12], "LambdaWarmUpCosineScheduler2": [37, 13, 27], "LambdaLinearScheduler": [40, 37, 17]}


def reference_module():
    import refshim
    sys.dont_write_bytecode = True
    spec = importlib.util.spec_from_file_location("_reference_lr_scheduler", os.path.join(refshim.REF_ROOT, "sgm", "lr_scheduler.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def case_lr_schedules():
    ref = reference_module()
    out = {}
    for cls, configs in CONFIGS.items():
        for k, (cfg, last) in enumerate(zip(configs, N[cls])):
            sched = getattr(ref, cls)(**cfg)
            out[f"{cls}_{k}"] = np.asarray([float(sched.schedule(n)) for n in range(last + 1)], dtype=np.float64)
    np.savez(os.path.join(HERE, "lr_schedules.npz"), **out)
    return out


if __name__ == "__main__":
    import refshim
    res = case_lr_schedules()
    print({k: v.shape for k, v in res.items()})
    assert not os.path.exists(os.path.join(refshim.REF_ROOT, "sgm", "__pycache__")), "bytecode leaked into the reference tree"

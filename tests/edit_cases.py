"""What tests/test_edit_cpu.py and tests/test_edit_gpu.py share (plain helper module, like image_cases.py and sampler_cases.py; no tests,
no fixtures): the names and the noise domain include/edit/cd360_edit.h adds (the library's entry in sampler_cases.LIBRARIES, where the
header / table / library rule is stated) and the numpy restatement of the blend in fp32."""
import os

import numpy as np

import image_cases as IC
import sampler_cases as SC

LIBRARY = 1  # in SC.LIBRARIES
NEW = SC.LIBRARIES[LIBRARY][3]
HEADER = os.path.join("edit", "cd360_edit.h")
DOMAIN_EDIT = 3


def normals(seed, stream, step, hw, dtype=np.float64):
    """[4, hw]: the domain-3 normals of one row."""
    return IC.normals(seed, stream, step, hw, DOMAIN_EDIT, dtype)


def batch(seed, streams, step, hw, dtype=np.float64):
    """[bs, 4, hw] for one stream id per row: what cd360_edit_noise_f32 writes."""
    return np.stack([normals(seed, s, step, hw, dtype) for s in streams])


def blend(x, known, m, s_next, z):
    """The blend in numpy fp32, one rounding per operation in the header's order: x, known, z [bs, 4, hw] fp32, m [bs or 1, 1, hw] fp32,
    s_next an fp32 scalar."""
    x, known, m, z = (np.asarray(a, np.float32) for a in (x, known, m, z))
    s = np.float32(s_next)
    kn = known if s == 0 else (known + (z * s).astype(np.float32)).astype(np.float32)
    keep = (np.float32(1.0) - m).astype(np.float32)
    return ((m * x).astype(np.float32) + (keep * kn).astype(np.float32)).astype(np.float32)


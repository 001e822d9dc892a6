"""What tests/test_edit_cpu.py and tests/test_edit_gpu.py share (plain helper module, like image_cases.py and sampler_cases.py; no tests,
no fixtures): the names and the noise domain include/edit/cd360_edit.h adds, the header / table / library rule of
sampler_cases.check_header_matches_table restated for the SECOND library (its header lies in include/edit/, its table is not in
cd360._lib.ABI), the numpy restatement of the blend in fp32, and a recorder for libcd360_edit.so under tests/guarded.py."""
import contextlib
import ctypes
import os
import re

import numpy as np

import image_cases as IC
import sampler_cases as SC

NEW = ["cd360_edit_noise_f32", "cd360_mask_blend_f32"]
HEADER = os.path.join("edit", "cd360_edit.h")
DOMAIN_EDIT = 3


def check_header_matches_table():
    """include/edit/cd360_edit.h <=> cd360._edit.EDIT_SIGNATURES <=> the loaded libcd360_edit.so, by the rule of
    sampler_cases.check_header_matches_table (every `cd360_...(` word of the header, comments included).  -> (mismatch, in_abi_tables,
    in_abi_headers, mistyped, lib): the names on which header, table and NEW disagree; the new names a table of cd360._lib.ABI holds; the
    headers of include/*.h that name one; the new names the library does not export as typed; the library.  The first four must be empty."""
    from cd360 import _edit, _lib
    table = _edit.EDIT_SIGNATURES
    assert all(t is not table for t in _lib.ABI.values())
    new = set(NEW)
    declared = set(re.findall(r"\b(cd360_[a-z0-9_]+)\s*\(", SC.header_text(HEADER)))
    mismatch = (declared ^ set(table)) | (declared ^ new)
    in_abi_tables = {n for t in _lib.ABI.values() for n in t} & new
    top = [f for f in os.listdir(os.path.join(SC.ROOT, "include")) if f.endswith(".h")]
    in_abi_headers = [h for h in top if any(n in SC.header_text(h) for n in new)]
    lib = _edit.load()
    mistyped = [n for n in NEW if not (isinstance(getattr(lib, n), ctypes._CFuncPtr) and getattr(lib, n).restype is ctypes.c_int
                                       and list(getattr(lib, n).argtypes) == table[n][1])]
    return mismatch, in_abi_tables, in_abi_headers, mistyped, lib


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


@contextlib.contextmanager
def recorded(guard):
    """Inside tests/guarded.py's context: record the entry points of libcd360_edit.so as well (guarded() records cd360._lib.load()'s
    library; cd360.ops reaches the second library through cd360._edit.load()), into the same list P4 reads."""
    import guarded as G
    from cd360 import _edit
    rec = G.Recorder(_edit.load())
    saved = _edit.load
    _edit.load = lambda: rec
    try:
        yield rec
    finally:
        _edit.load = saved
        guard.lib.called.extend(rec.called)

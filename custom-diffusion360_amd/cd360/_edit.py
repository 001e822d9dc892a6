"""ctypes binding of libcd360_edit.so (the C ABI declared in include/edit/cd360_edit.h): the blend that ends a masked sampling step and
the noise it adds to the known latent.

A library with a table of its own, entered in no older library's: DESIGN.md ("Why a second library") says why,
tests/sampler_cases.py::check_library_matches_table holds every library to it.  Bound by cd360._lib.bind: no fallback, no environment
variable."""
from __future__ import annotations

import os
from ctypes import c_int, c_int64, c_void_p

from ._lib import Cd360Error, bind, check  # noqa: F401  (check: the error codes are those of include/cd360_hip.h)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(os.path.dirname(_HERE), "lib", "libcd360_edit.so")
HEADER = os.path.join("edit", "cd360_edit.h")  # under include/

_P = c_void_p

# name -> (restype, argtypes); must list every symbol of include/edit/cd360_edit.h
EDIT_SIGNATURES = {
    "cd360_edit_noise_f32": (c_int, [_P, _P, _P, _P, c_int, c_int64, _P]),
    "cd360_mask_blend_f32": (c_int, [_P, _P, _P, c_int, _P, c_int, _P, _P, _P, c_int, c_int64, _P]),
}

_lib = None


def load():
    """The library, bound by cd360._lib.bind on the first call."""
    global _lib
    if _lib is None:
        _lib = bind(LIB_PATH, EDIT_SIGNATURES)
    return _lib

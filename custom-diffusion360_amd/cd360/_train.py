"""ctypes binding of libcd360_train.so (the C ABI declared in include/train/cd360_train.h): the two ends of a fine-tuning step -- the
seeded per-sample sigma draws and scalars, the noising of the target latent and the reference views, the l2 term of the loss and its
gradient with respect to the network's output.

A library with a table of its own, entered in no older library's: DESIGN.md ("Why a second library") says why.  Bound by
cd360._lib.bind: no fallback, no environment variable."""
from __future__ import annotations

import os
from ctypes import POINTER, c_float, c_int, c_int64, c_void_p

from ._lib import Cd360Error, bind, check  # noqa: F401  (check: the error codes are those of include/cd360_hip.h)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(os.path.dirname(_HERE), "lib", "libcd360_train.so")
HEADER = os.path.join("train", "cd360_train.h")  # under include/
ROW = 12  # CD360_TRAIN_ROW: fp32 values per sample in the scalar rows
# columns of a scalar row
SIGMA, W, C_SKIP, C_OUT, C_IN, SIGMA_REF, C_IN_REF, OFF_TGT, OFF_REF = range(9)
CUBIC, DISCRETE = 0, 1  # CD360_TRAIN_CUBIC, CD360_TRAIN_DISCRETE
# counter domains of ../csrc/cd360_philox.h that this library draws in
DOMAIN_SIGMA, DOMAIN_TARGET, DOMAIN_REF_A, DOMAIN_REF_B = 4, 5, 6, 7

_P = c_void_p
_S = POINTER(c_int64)  # a host array: the four element strides (batch, channel, row, column) of eps / d_eps

# name -> (restype, argtypes); must list every symbol of include/train/cd360_train.h
TRAIN_SIGNATURES = {
    "cd360_train_sigmas_f32": (c_int, [_P, c_int, _P, c_int, c_int, c_int, _P, c_int, c_int, c_int, _P, _P, _P, c_int, _P, _P, _P, _P, c_int, _P]),
    "cd360_train_noise_f32": (c_int, [_P, _P, _P, _P, _P, _P, _P, c_float, _P, _P, _P, c_int, c_int, c_int, c_int64, _P]),
    "cd360_train_l2_f32": (c_int, [_P, c_int, _S, _P, _P, _P, _P, _P, _P, c_int, c_int, c_int, _P]),
    "cd360_train_l2_bwd_f32": (c_int, [_P, c_int, _S, _P, _P, _P, _P, _P, _P, _P, _S, c_int, c_int, c_int, _P]),
}

_lib = None


def load():
    """The library, bound by cd360._lib.bind on the first call."""
    global _lib
    if _lib is None:
        _lib = bind(LIB_PATH, TRAIN_SIGNATURES)
    return _lib

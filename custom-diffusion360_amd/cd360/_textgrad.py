"""ctypes binding of libcd360_textgrad.so (the C ABI declared in include/textgrad/cd360_textgrad.h): the backward of the prompt encoders'
causal self-attention, MLP activation and EOT pooling, and the gradient of the modifier rows of the token table.

A library with a table of its own, entered in no older library's: DESIGN.md ("Why a second library") says why.  Bound by
cd360._lib.bind: no fallback, no environment variable."""
from __future__ import annotations

import os
from ctypes import POINTER, c_float, c_int, c_int64, c_void_p

from ._lib import Cd360Error, bind, check  # noqa: F401  (check: the error codes are those of include/cd360_hip.h)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(os.path.dirname(_HERE), "lib", "libcd360_textgrad.so")
HEADER = os.path.join("textgrad", "cd360_textgrad.h")  # under include/
MAX_MODIFIERS = 3  # CD360_TEXTGRAD_MAX_MODIFIERS

_P = c_void_p
_S = POINTER(c_int64)  # a host array: three element strides (batch, head, row), or the modifier ids

# name -> (restype, argtypes); must list every symbol of include/textgrad/cd360_textgrad.h
TEXTGRAD_SIGNATURES = {
    "cd360_textgrad_causal_attn_bwd_bf16": (c_int, [_P] * 7 + [c_int, c_int, c_int] + [_S] * 7 + [c_float, _P]),
    "cd360_textgrad_act_bwd_bf16": (c_int, [_P, _P, _P, c_int64, c_int, c_int64, c_int64, c_int64, c_int, _P]),
    "cd360_textgrad_eot_scatter_bf16": (c_int, [_P, _P, _P, c_int, c_int, c_int, c_int64, c_int64, _P]),
    "cd360_textgrad_token_rows_f32": (c_int, [_P, _P, _S, _P, c_int, c_int, c_int, c_int, c_int64, _P]),
}

_lib = None


def load():
    """The library, bound by cd360._lib.bind on the first call."""
    global _lib
    if _lib is None:
        _lib = bind(LIB_PATH, TEXTGRAD_SIGNATURES)
    return _lib

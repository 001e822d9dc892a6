"""ctypes binding of libcd360_text.so (the C ABI declared in include/text/cd360_text.h): the prompt encoders' token + position embedding,
causal self-attention, MLP activation and EOT pooling.

A library with a table of its own, entered in no older library's: DESIGN.md ("Why a second library") says why,
tests/sampler_cases.py::check_library_matches_table holds every library to it.  Bound by cd360._lib.bind: no fallback, no environment
variable."""
from __future__ import annotations

import os
from ctypes import POINTER, c_float, c_int, c_int64, c_void_p

from ._lib import Cd360Error, bind, check  # noqa: F401  (check: the error codes are those of include/cd360_hip.h)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(os.path.dirname(_HERE), "lib", "libcd360_text.so")
HEADER = os.path.join("text", "cd360_text.h")  # under include/
MAX_TOKENS = 128  # CD360_TEXT_MAX_TOKENS

_P = c_void_p
_S = POINTER(c_int64)  # a host array of three element strides (batch, head, row)

# name -> (restype, argtypes); must list every symbol of include/text/cd360_text.h
TEXT_SIGNATURES = {
    "cd360_text_embed_bf16": (c_int, [_P, _P, _P, _P, c_int, c_int, c_int, c_int, c_int64, _P, _P]),
    "cd360_text_causal_attn_bf16": (c_int, [_P, _P, _P, _P, c_int, c_int, c_int, _S, _S, _S, _S, c_float, _P]),
    "cd360_text_act_bf16": (c_int, [_P, _P, c_int64, c_int, c_int64, c_int64, c_int, _P]),
    "cd360_text_eot_pool_bf16": (c_int, [_P, _P, _P, c_int, c_int, c_int, c_int64, c_int64, _P]),
}

_lib = None


def load():
    """The library, bound by cd360._lib.bind on the first call."""
    global _lib
    if _lib is None:
        _lib = bind(LIB_PATH, TEXT_SIGNATURES)
    return _lib

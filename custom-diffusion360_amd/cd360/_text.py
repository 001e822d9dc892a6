"""ctypes binding of libcd360_text.so (the C ABI declared in include/text/cd360_text.h): the prompt encoders' token + position embedding,
causal self-attention, MLP activation and EOT pooling.

A fourth library with a table of its own: the first library's headers, tables and exports are closed (cd360/_lib.py::ABI names exactly
the headers of include/*.h) and so are the second's and the third's (cd360/_edit.py, cd360/_optim.py), so TEXT_SIGNATURES is entered in
none of them.  There is NO fallback: if the shared library is missing or a symbol is absent this module raises.  The library is built
in-tree by `__graft_entry__.build()` next to libcd360_hip.so.  No environment variable is read."""
from __future__ import annotations

import ctypes
import os
from ctypes import POINTER, c_float, c_int, c_int64, c_void_p

from ._lib import Cd360Error, check  # noqa: F401  (check: the error codes are those of include/cd360_hip.h)

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
    """dlopen the library and type every entry point.  Raises if anything is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise Cd360Error(
            f"{LIB_PATH} not found: the HIP extension has not been built (run `python __graft_entry__.py`). "
            "There is no CPU or PyTorch fallback for the cd360 operators."
        )
    # torch FIRST, as in cd360._lib.load: the device pointers and streams this library is handed belong to the HIP runtime of torch's wheel,
    # and with that runtime already mapped the dynamic loader binds this library's libamdhip64 dependency to it
    import torch  # noqa: F401
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in TEXT_SIGNATURES.items():
        try:
            fn = getattr(lib, name)
        except AttributeError as e:
            raise Cd360Error(f"libcd360_text.so does not export {name}") from e
        fn.restype, fn.argtypes = res, args
    _lib = lib
    return lib

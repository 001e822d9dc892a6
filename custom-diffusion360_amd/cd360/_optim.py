"""ctypes binding of libcd360_optim.so (the C ABI declared in include/optim/cd360_optim.h): the squared gradient norm, the clip factor
and the AdamW pass with a live learning rate, clipping and EMA.

A third library with a table of its own: the first library's headers, tables and exports are closed (cd360/_lib.py::ABI names exactly
the headers of include/*.h) and so are the second's (cd360/_edit.py), so OPTIM_SIGNATURES is entered in neither.  There is NO fallback:
if the shared library is missing or a symbol is absent this module raises.  The library is built in-tree by `__graft_entry__.build()`
next to libcd360_hip.so.  No environment variable is read."""
from __future__ import annotations

import ctypes
import os
from ctypes import c_float, c_int, c_int64, c_void_p

from ._lib import Cd360Error, check  # noqa: F401  (check: the error codes are those of include/cd360_hip.h)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(os.path.dirname(_HERE), "lib", "libcd360_optim.so")
HEADER = os.path.join("optim", "cd360_optim.h")  # under include/

_P = c_void_p

# name -> (restype, argtypes); must list every symbol of include/optim/cd360_optim.h
OPTIM_SIGNATURES = {
    "cd360_grad_sumsq_bf16": (c_int, [c_int, _P, _P, _P, _P]),
    "cd360_grad_clip_f32": (c_int, [_P, c_int64, c_float, _P, _P]),
    "cd360_adamw_live_bf16": (c_int, [c_int, _P, _P, _P, _P, _P, _P, c_int, _P, _P, _P, _P, _P, c_float, _P, c_float, c_float, c_float, _P]),
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
    for name, (res, args) in OPTIM_SIGNATURES.items():
        try:
            fn = getattr(lib, name)
        except AttributeError as e:
            raise Cd360Error(f"libcd360_optim.so does not export {name}") from e
        fn.restype, fn.argtypes = res, args
    _lib = lib
    return lib

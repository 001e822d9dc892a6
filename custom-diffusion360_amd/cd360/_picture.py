"""ctypes binding of libcd360_picture.so (the C ABI declared in include/picture/cd360_picture.h): from a decoded uint8 frame to the
tensors the first stage and the loss read -- crop + antialiased resize into fp32 planes, and the maps of a mask (thresholded, cropped,
resized by the nearest rule; its dilation; the crop's "inside the picture" map).

A library with a table of its own, entered in no older library's: DESIGN.md ("Why a second library") says why.  Bound by
cd360._lib.bind: no fallback, no environment variable."""
from __future__ import annotations

import os
from ctypes import c_float, c_int, c_int64, c_void_p

from ._lib import Cd360Error, bind, check  # noqa: F401  (check: the error codes are those of include/cd360_hip.h)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(os.path.dirname(_HERE), "lib", "libcd360_picture.so")
HEADER = os.path.join("picture", "cd360_picture.h")  # under include/
MAX_TAPS = 64  # CD360_PICTURE_MAX_TAPS: the longest row of a tap table
MAX_DILATE = 31  # CD360_PICTURE_MAX_DILATE: the largest dilation window

_P = c_void_p

# name -> (restype, argtypes); must list every symbol of include/picture/cd360_picture.h
PICTURE_SIGNATURES = {
    "cd360_picture_resample_u8": (c_int, [_P, c_int, c_int, c_int, c_int64, c_int, c_int, c_int, c_int, c_int, _P, _P, _P, c_int, _P, _P, _P, c_int,
                                          c_int, c_int, c_int, c_float, c_float, c_float, _P, _P, _P]),
    "cd360_picture_mask_u8": (c_int, [_P, c_int, c_int, c_int64, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, _P, _P, _P, _P]),
}

_lib = None


def load():
    """The library, bound by cd360._lib.bind on the first call."""
    global _lib
    if _lib is None:
        _lib = bind(LIB_PATH, PICTURE_SIGNATURES)
    return _lib

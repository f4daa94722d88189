"""ctypes binding of libscg_camgrad.so (include/camgrad/scg_camgrad.h): the rasterizer's gradient with respect to the camera.

A library next to libscg_raster.so with a version and an error string of its own (build.SIDE_LIBRARIES["camgrad"]).  As there: a
missing library raises, there is no quiet stand-in for a kernel.  tests/test_camgrad_cpu.py holds SYMBOLS and the constants to
the header's text.
"""
from __future__ import annotations

import ctypes as C
import os

import torch  # noqa: F401  (first, so that torch's HIP runtime is the one the library binds to)

from ._lib import ScgModel, open_library, raise_last_error

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libscg_camgrad.so")

# the header's integer #defines under their own names minus "SCG_"
CAMGRAD_ABI_VERSION = ABI_VERSION = 2
CAMGRAD_BLOCK, CAMGRAD_SUMS, CAMGRAD_OUT_FLOATS, CAMGRAD_MAX_DIM = 256, 27, 35, 1048560
CAMGRAD_NO_CAMPOS = 1

_P = C.c_void_p
_SCALARS = [C.c_int32, C.c_int32, C.c_float, C.c_float, C.c_float, C.c_int32]          # H, W, tanfovx, tanfovy, scale_modifier, sh_degree
SYMBOLS = {
    "scg_camgrad_last_error": (C.c_char_p, []),
    "scg_camgrad_abi_version": (C.c_int32, []),
    "scg_camgrad_sizes": (C.c_int, [C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_uint64)]),
    "scg_camgrad_backward": (C.c_int, _SCALARS + [C.c_int32, C.c_int32] + [_P] * 3 + [_P] * 7 + [_P, _P, _P, _P, C.c_int32, _P]),
    "scg_camgrad_backward_model": (C.c_int, _SCALARS + [C.c_int32] + [_P] * 3 + [C.POINTER(ScgModel)] + [_P, _P, _P, _P, C.c_int32, _P]),
}

_lib = None


def load() -> C.CDLL:
    """Load (once), type and version-check the library.  Raises ScgError when it is absent (python -m scgaussian_amd.build)."""
    global _lib
    if _lib is None:
        _lib = open_library(LIB_PATH, SYMBOLS, ("scg_camgrad_abi_version", ABI_VERSION), {}, "libscg_camgrad.so")
    return _lib


def check(rc: int, what: str) -> None:
    if rc != 0:
        raise_last_error(rc, what, load().scg_camgrad_last_error)

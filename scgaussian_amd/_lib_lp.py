"""ctypes binding of libscg_lp.so (include/lp/scg_lpips.h): the LPIPS metric with VGG16 features on the GPU.

A sixth library next to libscg_raster.so with a version and an error string of its own.  As there: a missing library raises, there
is no quiet stand-in for a kernel.  tests/test_lpips_cpu.py holds SYMBOLS and the constants to the header's text (tests/abi_compare.py
check_side_library).
"""
from __future__ import annotations

import ctypes as C
import os

import torch  # noqa: F401  (first, so that torch's HIP runtime is the one the library binds to)

from ._lib import open_library, raise_last_error

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libscg_lp.so")

# the header's integer #defines under their own names minus "SCG_"
LP_ABI_VERSION = ABI_VERSION = 1
LP_LAYERS, LP_TAPS, LP_TILE_M, LP_HEAD_PIXELS, LP_SMALL_GRID = 13, 5, 128, 32, 128
LP_MIN_DIM, LP_MAX_DIM, LP_MAX_PIXELS, LP_MAX_BATCH = 16, 16384, 16777216, 2
LP_PARAM_FLOATS = 14716160
LP_RELU, LP_POOL, LP_ZSCORE = 1, 2, 4

_P = C.c_void_p
_I = C.c_int32
SYMBOLS = {
    "scg_lp_last_error": (C.c_char_p, []),
    "scg_lp_abi_version": (C.c_int32, []),
    "scg_lp_scratch_bytes": (C.c_size_t, [_I, _I]),
    "scg_lp_feature_floats": (C.c_size_t, [_I, _I]),
    "scg_lp_conv3x3": (C.c_int, [_I, _I, _I, _I, _I, _P, _P, _P, _P, _I, _P]),
    "scg_lp_forward": (C.c_int, [_I, _I, _P, _P, _P, _P, _P, _P, _P, C.c_size_t, _P]),
    "scg_lp_head": (C.c_int, [_I, _I, _P, _P, _P, _P, _P, C.c_size_t, _P]),
}

_lib = None


def load() -> C.CDLL:
    """Load (once), type and version-check the library.  Raises ScgError when it is absent (python -m scgaussian_amd.build)."""
    global _lib
    if _lib is None:
        _lib = open_library(LIB_PATH, SYMBOLS, ("scg_lp_abi_version", ABI_VERSION), {}, "libscg_lp.so")
    return _lib


def check(rc: int, what: str) -> None:
    if rc != 0:
        raise_last_error(rc, what, load().scg_lp_last_error)

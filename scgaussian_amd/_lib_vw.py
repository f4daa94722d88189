"""ctypes binding of libscg_vw.so (include/vw/scg_virtualwarp.h): the virtual-view warp loss and the depth smoothness, forward and
backward, on the GPU.

A fifth library next to libscg_raster.so with a version and an error string of its own.  As there: a missing library raises, there
is no quiet stand-in for a kernel.  tests/test_virtualwarp_cpu.py holds SYMBOLS and the constants to the header's text (tests/abi_compare.py
check_side_library).
"""
from __future__ import annotations

import ctypes as C
import os

import torch  # noqa: F401  (first, so that torch's HIP runtime is the one the library binds to)

from ._lib import open_library, raise_last_error

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libscg_vw.so")

# the header's integer #defines under their own names minus "SCG_"
VW_ABI_VERSION = ABI_VERSION = 1
VW_MAX_VIEWS, VW_TILE, VW_SMOOTH_PIXELS, VW_RECORD_FLOATS = 16, 16, 256, 12
VW_MIN_DIM, VW_MAX_DIM, VW_MAX_GUIDE_CHANNELS = 3, 16384, 64

_P = C.c_void_p
_I = C.c_int32
SYMBOLS = {
    "scg_vw_last_error": (C.c_char_p, []),
    "scg_vw_abi_version": (C.c_int32, []),
    "scg_vw_warp_scratch_bytes": (C.c_size_t, [_I, _I, _I]),
    "scg_vw_warp_forward": (C.c_int, [_I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, C.c_size_t, _P]),
    "scg_vw_warp_backward": (C.c_int, [_I, _I, _I, _P, _P, _P, _P, C.c_size_t, _P, _P, _P]),
    "scg_vw_smooth_scratch_bytes": (C.c_size_t, [_I, _I]),
    "scg_vw_smooth_forward": (C.c_int, [_I, _I, _I, _P, _P, _P, _P, C.c_size_t, _P]),
    "scg_vw_smooth_backward": (C.c_int, [_I, _I, _I, _P, _P, _P, _P, _P]),
}

_lib = None


def load() -> C.CDLL:
    """Load (once), type and version-check the library.  Raises ScgError when it is absent (python -m scgaussian_amd.build)."""
    global _lib
    if _lib is None:
        _lib = open_library(LIB_PATH, SYMBOLS, ("scg_vw_abi_version", ABI_VERSION), {}, "libscg_vw.so")
    return _lib


def check(rc: int, what: str) -> None:
    if rc != 0:
        raise_last_error(rc, what, load().scg_vw_last_error)

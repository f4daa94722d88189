"""ctypes binding of libscg_img.so (include/img/scg_resample.h): the camera images' bicubic resize on the GPU.

A third library next to libscg_raster.so and libscg_io.so with a version and an error string of its own.  As there: a missing
library raises, there is no CPU or PyTorch stand-in for a kernel.  tests/test_resize_cpu.py holds SYMBOLS and the constants to the
header's text (tests/abi_compare.py check_side_library).
"""
from __future__ import annotations

import ctypes as C
import os

import torch  # noqa: F401  (first, so that torch's HIP runtime is the one the library binds to)

from ._lib import open_library, raise_last_error

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libscg_img.so")

# the header's integer #defines under their own names minus "SCG_"
IMG_ABI_VERSION = ABI_VERSION = 1
RESAMPLE_MAX_KSIZE, RESAMPLE_MAX_SIZE = 129, 65535
RESAMPLE_STRIP, RESAMPLE_STRIP_ROWS, RESAMPLE_VTILE, RESAMPLE_PITCH_ALIGN = 32, 32, 1024, 16

_P = C.c_void_p
_I = C.c_int32
SYMBOLS = {
    "scg_img_last_error": (C.c_char_p, []),
    "scg_img_abi_version": (C.c_int32, []),
    "scg_resample_pitch": (C.c_size_t, [_I, _I]),
    "scg_resample_mid_bytes": (C.c_size_t, [_I, _I, _I, _I, _I]),
    "scg_resample_u8": (C.c_int, [_P, _I, _I, _I, _I, _I, _I, _P, _P, _I, _P, _P, _I, _P, C.c_size_t, _P, C.c_size_t, _P,
                                  C.c_size_t, _P]),
}

_lib = None


def load() -> C.CDLL:
    """Load (once), type and version-check the library.  Raises ScgError when it is absent (python -m scgaussian_amd.build)."""
    global _lib
    if _lib is None:
        _lib = open_library(LIB_PATH, SYMBOLS, ("scg_img_abi_version", ABI_VERSION), {}, "libscg_img.so")
    return _lib


def check(rc: int, what: str) -> None:
    if rc != 0:
        raise_last_error(rc, what, load().scg_img_last_error)

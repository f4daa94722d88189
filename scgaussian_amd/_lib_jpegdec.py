"""ctypes binding of libscg_jpegdec.so (include/jpegdec/scg_jpegdec.h): baseline JPEG files decoded on the GPU.

A library next to libscg_raster.so with a version and an error string of its own (build.SIDE_LIBRARIES["jpegdec"]).  As there: a
missing library raises, there is no quiet stand-in for a kernel.  tests/test_jpegdec_cpu.py holds SYMBOLS and the constants to
the header's text.
"""
from __future__ import annotations

import ctypes as C
import os

import torch  # noqa: F401  (first, so that torch's HIP runtime is the one the library binds to)

from ._lib import open_library, raise_last_error

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libscg_jpegdec.so")

# the header's integer #defines under their own names minus "SCG_"
JPEGDEC_ABI_VERSION = ABI_VERSION = 2
JPEGDEC_SUBSEQ, JPEGDEC_THREADS, JPEGDEC_MAX_DIM, JPEGDEC_MAX_SEGMENT = 128, 256, 65535, 2 ** 28 - 1
JPEGDEC_HEADER_BYTES, JPEGDEC_FRAME_WORDS, JPEGDEC_IMAGE_WORDS, JPEGDEC_MAX_BATCH = 4096, 16, 48, 65535
JPEGDEC_BAD_CODE, JPEGDEC_BAD_ZIGZAG, JPEGDEC_BAD_COUNT, JPEGDEC_BAD_SYNC, JPEGDEC_BAD_RESTART = 1, 2, 4, 8, 16

_P = C.c_void_p
_U64P = C.POINTER(C.c_uint64)
SYMBOLS = {
    "scg_jpegdec_last_error": (C.c_char_p, []),
    "scg_jpegdec_abi_version": (C.c_int32, []),
    "scg_jpegdec_sizes": (C.c_int, [C.POINTER(C.c_int32), C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_int32)]),
    "scg_jpegdec_decode": (C.c_int, [C.POINTER(C.c_int32), _P, _P, C.c_uint64, _P, C.c_size_t, _P, C.c_size_t, C.c_int32, C.c_int32, _P]),
    "scg_jpegdec_batch_plan": (C.c_int, [C.c_int32, C.POINTER(C.c_int32), _U64P, _U64P, _U64P, C.c_uint64, C.POINTER(C.c_uint32), C.c_uint64,
                                         _U64P, _U64P, _U64P, C.POINTER(C.c_int32)]),
    "scg_jpegdec_decode_batch": (C.c_int, [C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_uint32), _P, _P, C.c_uint64, _P, C.c_size_t, _P,
                                           C.c_size_t, C.c_int32, _P]),
}

_lib = None


def load() -> C.CDLL:
    """Load (once), type and version-check the library.  Raises ScgError when it is absent (python -m scgaussian_amd.build)."""
    global _lib
    if _lib is None:
        _lib = open_library(LIB_PATH, SYMBOLS, ("scg_jpegdec_abi_version", ABI_VERSION), {}, "libscg_jpegdec.so")
    return _lib


def check(rc: int, what: str) -> None:
    if rc != 0:
        raise_last_error(rc, what, load().scg_jpegdec_last_error)

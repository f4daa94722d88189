"""ctypes binding of libscg_png.so (include/png/scg_png.h): PNG files' zlib streams packed on the GPU.

A seventh library next to libscg_raster.so with a version and an error string of its own.  As there: a missing library raises, there
is no quiet stand-in for a kernel.  tests/test_png_cpu.py holds SYMBOLS, the structs and the constants to the header's text (tests/abi_compare.py
check_side_library).
"""
from __future__ import annotations

import ctypes as C
import os

import torch  # noqa: F401  (first, so that torch's HIP runtime is the one the library binds to)

from ._lib import open_library, raise_last_error

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libscg_png.so")

# the header's integer #defines under their own names minus "SCG_"
PNG_ABI_VERSION = ABI_VERSION = 1
PNG_CHUNK, PNG_THREADS, PNG_SYMBOLS, PNG_LENGTHS, PNG_HEADER_BITS, PNG_MAX_CODE_BITS = 32768, 256, 286, 288, 1226, 15
PNG_MAX_DIM, PNG_MAX_STREAM, PNG_MAX_IMAGES, PNG_ALIGN = 65535, 2 ** 31 - 1, 2 ** 20, 16
PNG_FILTER_NONE, PNG_FILTER_SUB, PNG_FILTER_UP, PNG_FILTER_PAETH = 0, 1, 2, 4
PNG_KIND_DYNAMIC, PNG_KIND_STORED = 0, 1


class ScgPngLayout(C.Structure):
    """Sizes of a batch and the regions of its workspace (include/png/scg_png.h ScgPngLayout)."""
    _fields_ = [(n, C.c_uint64) for n in ("images", "chunks", "capacity", "workspace_bytes", "lengths_offset", "info_offset",
                                          "base_offset", "scan_offset", "table_offset", "table_bytes")]


class ScgPngImage(C.Structure):
    _fields_ = [("src", C.c_uint64)] + [(n, C.c_int32) for n in ("H", "W", "channels", "first_chunk", "chunks", "stream_bytes")]


class ScgPngChunk(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("image", "index")]


class ScgPngChunkInfo(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("bytes", "kind", "sum_a", "sum_b")]


class ScgPngEncode(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("struct_bytes", "images", "filter", "gray_as_rgb")] + [
        (n, C.c_void_p) for n in ("images_host", "images_dev", "chunks_dev")]


STRUCTS = (ScgPngLayout, ScgPngImage, ScgPngChunk, ScgPngChunkInfo, ScgPngEncode)       # in the order of scg_png_struct_bytes(which)

_P = C.c_void_p
SYMBOLS = {
    "scg_png_last_error": (C.c_char_p, []),
    "scg_png_abi_version": (C.c_int32, []),
    "scg_png_struct_bytes": (C.c_size_t, [C.c_int32]),
    "scg_png_layout": (C.c_int, [C.c_int32, C.POINTER(C.c_int32), C.c_int32, C.POINTER(ScgPngLayout), C.POINTER(ScgPngImage),
                                 C.POINTER(ScgPngChunk)]),
    "scg_png_encode": (C.c_int, [C.POINTER(ScgPngEncode), _P, C.c_size_t, _P, C.c_size_t, _P]),
}

_lib = None


def load() -> C.CDLL:
    """Load (once), type and version-check the library.  Raises ScgError when it is absent (python -m scgaussian_amd.build)."""
    global _lib
    if _lib is None:
        _lib = open_library(LIB_PATH, SYMBOLS, ("scg_png_abi_version", ABI_VERSION), {"scg_png_struct_bytes": STRUCTS}, "libscg_png.so")
    return _lib


def check(rc: int, what: str) -> None:
    if rc != 0:
        raise_last_error(rc, what, load().scg_png_last_error)

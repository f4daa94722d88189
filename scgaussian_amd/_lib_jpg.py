"""ctypes binding of libscg_jpg.so (include/jpg/scg_jpeg.h): baseline JPEG files packed on the GPU.

An eighth library next to libscg_raster.so with a version and an error string of its own (build.SIDE_LIBRARIES["jpg"]).  As there:
a missing library raises, there is no quiet stand-in for a kernel.  tests/test_jpeg_cpu.py holds SYMBOLS, the structs and the
constants to the header's text.
"""
from __future__ import annotations

import ctypes as C
import os

import torch  # noqa: F401  (first, so that torch's HIP runtime is the one the library binds to)

from ._lib import open_library, raise_last_error

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libscg_jpg.so")

# the header's integer #defines under their own names minus "SCG_"
JPG_ABI_VERSION = ABI_VERSION = 1
JPEG_THREADS, JPEG_WINDOW, JPEG_MAX_DIM, JPEG_MAX_IMAGES, JPEG_MAX_HEADER, JPEG_ALIGN = 256, 16384, 65535, 2 ** 20, 700, 16
JPEG_444, JPEG_420 = 0, 2


class ScgJpegLayout(C.Structure):
    """Sizes of a batch and the regions of its workspace (include/jpg/scg_jpeg.h ScgJpegLayout)."""
    _fields_ = [(n, C.c_uint64) for n in ("images", "segments", "headers_bytes", "capacity", "workspace_bytes", "base_offset",
                                          "scan_offset", "table_offset", "table_bytes")]


class ScgJpegImage(C.Structure):
    _fields_ = [("src", C.c_uint64)] + [(n, C.c_int32) for n in ("H", "W", "channels", "first_segment", "segments", "mcus",
                                                                 "header_offset", "header_bytes")] + [
        ("capacity", C.c_uint32), ("reserved", C.c_int32)]


class ScgJpegSegment(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("image", "row")]


class ScgJpegEncode(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("struct_bytes", "images", "quality", "subsampling", "bgr", "reserved")] + [
        ("headers_bytes", C.c_uint64)] + [(n, C.c_void_p) for n in ("images_host", "images_dev", "segments_dev", "headers_dev")]


STRUCTS = (ScgJpegLayout, ScgJpegImage, ScgJpegSegment, ScgJpegEncode)       # in the order of scg_jpg_struct_bytes(which)

_P = C.c_void_p
SYMBOLS = {
    "scg_jpg_last_error": (C.c_char_p, []),
    "scg_jpg_abi_version": (C.c_int32, []),
    "scg_jpg_struct_bytes": (C.c_size_t, [C.c_int32]),
    "scg_jpeg_layout": (C.c_int, [C.c_int32, C.POINTER(C.c_int32), C.c_int32, C.c_int32, C.POINTER(C.c_uint32), C.POINTER(ScgJpegLayout),
                                  C.POINTER(ScgJpegImage), C.POINTER(ScgJpegSegment), C.POINTER(C.c_uint8)]),
    "scg_jpeg_encode": (C.c_int, [C.POINTER(ScgJpegEncode), _P, C.c_size_t, _P, C.c_size_t, _P]),
}

_lib = None


def load() -> C.CDLL:
    """Load (once), type and version-check the library.  Raises ScgError when it is absent (python -m scgaussian_amd.build)."""
    global _lib
    if _lib is None:
        _lib = open_library(LIB_PATH, SYMBOLS, ("scg_jpg_abi_version", ABI_VERSION), {"scg_jpg_struct_bytes": STRUCTS}, "libscg_jpg.so")
    return _lib


def check(rc: int, what: str) -> None:
    if rc != 0:
        raise_last_error(rc, what, load().scg_jpg_last_error)

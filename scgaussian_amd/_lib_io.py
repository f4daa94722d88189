"""ctypes binding of libscg_io.so (include/io/scg_ply.h): the scene files' bodies packed and unpacked on the GPU.

A second library next to libscg_raster.so with a version and an error string of its own; the raw model it reads and writes is
_lib.ScgModel.  As there: a missing library raises, there is no CPU or PyTorch stand-in for a kernel.
tests/test_ply_cpu.py holds SYMBOLS, the struct and the constants to the header's text (tests/abi_compare.py check_side_library).
"""
from __future__ import annotations

import ctypes as C
import os

import torch  # noqa: F401  (first, so that torch's HIP runtime is the one the library binds to)

from ._lib import ScgModel, open_library, raise_last_error

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libscg_io.so")

# the header's integer #defines under their own names minus "SCG_"
IO_ABI_VERSION = ABI_VERSION = 1
PLY_TILE_ROWS, PLY_RAY_FLOATS, PLY_BG_FLOATS, PLY_COLOR_BYTES, PLY_MAX_STRIDE = 64, 69, 62, 27, 224


class ScgPlyLayout(C.Structure):
    """Byte offsets and sizes of the three bodies in the one buffer of scg_ply_pack (include/io/scg_ply.h ScgPlyLayout)."""
    _fields_ = [(n, C.c_uint64) for n in ("ray_offset", "ray_bytes", "bg_offset", "bg_bytes", "color_offset", "color_bytes",
                                          "total")]


STRUCTS = (ScgPlyLayout,)           # the one scg_ply_layout_bytes() reports

_P = C.c_void_p
SYMBOLS = {
    "scg_io_last_error": (C.c_char_p, []),
    "scg_io_abi_version": (C.c_int32, []),
    "scg_ply_layout_bytes": (C.c_size_t, []),
    "scg_ply_layout": (C.c_int, [C.c_int32, C.c_int32, C.POINTER(ScgPlyLayout)]),
    "scg_ply_pack": (C.c_int, [C.POINTER(ScgModel), _P, C.c_size_t, _P]),
    "scg_ply_pack_color_view": (C.c_int, [C.POINTER(ScgModel), C.c_int32, _P, _P, C.c_size_t, _P]),
    "scg_ply_unpack": (C.c_int, [_P, C.c_size_t, C.POINTER(C.c_int32), C.c_int32, C.c_int32, C.c_int32, C.POINTER(ScgModel), _P]),
}

_lib = None


def load() -> C.CDLL:
    """Load (once), type and version-check the library.  Raises ScgError when it is absent (python -m scgaussian_amd.build)."""
    global _lib
    if _lib is None:
        _lib = open_library(LIB_PATH, SYMBOLS, ("scg_io_abi_version", ABI_VERSION), {"scg_ply_layout_bytes": STRUCTS}, "libscg_io.so")
    return _lib


def check(rc: int, what: str) -> None:
    if rc != 0:
        raise_last_error(rc, what, load().scg_io_last_error)

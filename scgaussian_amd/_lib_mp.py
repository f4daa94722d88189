"""ctypes binding of libscg_mp.so (include/mp/scg_matchpoint.h): the init stage's snapshot packed on the GPU.

A fourth library next to libscg_raster.so with a version and an error string of its own; its segment record is _lib.ScgSeedSegment.
As there: a missing library raises, there is no CPU or PyTorch stand-in for a kernel.
tests/test_matchpoint_cpu.py holds SYMBOLS, the structs and the constants to the header's text (tests/abi_compare.py
check_side_library).
"""
from __future__ import annotations

import ctypes as C
import os

import torch  # noqa: F401  (first, so that torch's HIP runtime is the one the library binds to)

from ._lib import ScgSeedSegment, open_library, raise_last_error  # noqa: F401  (ScgSeedSegment: the callers' name for the segment record)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libscg_mp.so")

# the header's integer #defines under their own names minus "SCG_"
MP_ABI_VERSION = ABI_VERSION = 1
MP_RECORD_BYTES, MP_TILE_RECORDS, MP_MATCH_GROUP, MP_RESOLVE_PIXELS, MP_QUANT_PIXELS = 27, 64, 256, 256, 1024
MP_MAX_SEGMENTS, MP_MAX_VIEWS, MP_MAX_DIM, MP_MAX_MATCHES, MP_MAX_PIXELS = 1024, 1024, 65535, 2 ** 31 - 1, 2 ** 31 - 1


class ScgMpLayout(C.Structure):
    """Byte offsets and sizes of the regions of the one buffer of scg_mp_pack (include/mp/scg_matchpoint.h ScgMpLayout)."""
    _fields_ = [(n, C.c_uint64) for n in ("body_offset", "body_bytes", "depth_offset", "depth_bytes", "byte_offset", "byte_bytes",
                                          "range_offset", "range_bytes", "total", "pixels", "resolve_groups", "quant_groups")]


class ScgMpView(C.Structure):
    """One view of the view table (ScgMpView): its size and where its planes and its workgroups begin."""
    _fields_ = [(n, C.c_int32) for n in ("H", "W", "first_pixel", "first_byte", "resolve_group", "quant_group")]


class ScgMpPack(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("struct_bytes", "N", "V", "nseg")] + [
        (n, C.c_void_p) for n in ("segments", "segments_dev", "views", "views_dev", "rays_o", "rays_d", "z", "color", "uv", "cam_z")]


STRUCTS = (ScgMpLayout, ScgMpView, ScgMpPack)           # in the order of scg_mp_struct_bytes(which)

_P = C.c_void_p
SYMBOLS = {
    "scg_mp_last_error": (C.c_char_p, []),
    "scg_mp_abi_version": (C.c_int32, []),
    "scg_mp_struct_bytes": (C.c_size_t, [C.c_int32]),
    "scg_mp_layout": (C.c_int, [C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.POINTER(ScgMpLayout), C.POINTER(ScgMpView)]),
    "scg_mp_workspace_bytes": (C.c_size_t, [C.c_int32, C.POINTER(C.c_int32)]),
    "scg_mp_pack": (C.c_int, [C.POINTER(ScgMpPack), _P, C.c_size_t, _P, C.c_size_t, _P]),
}

_lib = None


def load() -> C.CDLL:
    """Load (once), type and version-check the library.  Raises ScgError when it is absent (python -m scgaussian_amd.build)."""
    global _lib
    if _lib is None:
        _lib = open_library(LIB_PATH, SYMBOLS, ("scg_mp_abi_version", ABI_VERSION), {"scg_mp_struct_bytes": STRUCTS}, "libscg_mp.so")
    return _lib


def check(rc: int, what: str) -> None:
    if rc != 0:
        raise_last_error(rc, what, load().scg_mp_last_error)

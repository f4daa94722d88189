"""CPU-only checks of what the side libraries share: the build table (scgaussian_amd/build.py SIDE_LIBRARIES), the one loader
(scgaussian_amd/_lib.py open_library) and the one error text per library (csrc/host_error.h).  Each library's own header, exports
and constants are held by its own test file through tests/abi_compare.py check_side_library."""
import ctypes as C
import glob
import importlib
import itertools
import os

import pytest

import abi_text
from scgaussian_amd import _lib, _lib_img, _lib_io, _lib_png, build

# the table, restated: key -> (header, {source: extra flags}).  The -ffp-contract=off entries are pinned here, not only there.
EXPECTED = {
    "io": ("scg_ply.h", {"plypack.hip": ["-ffp-contract=off"]}),
    "img": ("scg_resample.h", {"resample.hip": []}),
    "mp": ("scg_matchpoint.h", {"matchpoint.hip": ["-ffp-contract=off"]}),
    "vw": ("scg_virtualwarp.h", {"virtualwarp.hip": ["-ffp-contract=off"]}),
    "lp": ("scg_lpips.h", {"lpips.hip": []}),
    "png": ("scg_png.h", {"pngpack.hip": []}),
    "jpg": ("scg_jpeg.h", {"jpegpack.hip": ["-ffp-contract=off"]}),
    "jpegdec": ("scg_jpegdec.h", {"jpegunpack.hip": ["-ffp-contract=off"]}),
    "camgrad": ("scg_camgrad.h", {"camgrad.hip": ["-ffp-contract=off"]}),
}
CONTRACT_OFF = {"geometry.hip", "evalview.hip", "optim.hip", "initstage.hip", "densify.hip", "seed.hip", "geocheck.hip", "mono.hip",
                "depthviz.hip"}


def _binding(key):
    return _lib if key == "main" else importlib.import_module(f"scgaussian_amd._lib_{key}")


def _header_names(key):
    paths = None if key == "main" else sorted(glob.glob(os.path.join(build.INCLUDE, build.SIDE_LIBRARIES[key][0], "*.h")))
    return set(abi_text.declared_in(abi_text.read(paths)))


def test_the_table_names_the_nine_libraries_in_order():
    assert list(build.SIDE_LIBRARIES) == list(EXPECTED) == ["io", "img", "mp", "vw", "lp", "png", "jpg", "jpegdec", "camgrad"]
    assert not any("jpeg" in s or "jpg" in s for s in build.SOURCES)     # the JPEG packer is a side library's, not the main one's
    assert {s for s, flags in build.SOURCES.items() if flags == ["-ffp-contract=off"]} == CONTRACT_OFF
    assert build.SOURCES["blend.hip"] == ["-fno-slp-vectorize"]
    assert all(flags == [] for s, flags in build.SOURCES.items() if s not in CONTRACT_OFF | {"blend.hip"})


@pytest.mark.parametrize("key", list(EXPECTED))
def test_build_table_entry(key):
    header, sources = EXPECTED[key]
    directory, table_sources = build.SIDE_LIBRARIES[key]
    path, accessor_sources = build.side_library(key)
    assert directory == key and table_sources == sources and accessor_sources is table_sources
    assert path == os.path.join(build.HERE, f"libscg_{key}.so") == _binding(key).LIB_PATH
    assert all(os.path.exists(os.path.join(build.CSRC, s)) for s in sources)
    assert os.path.join(build.INCLUDE, directory, header) in build.HEADERS
    assert callable(build.build_side)
    with pytest.raises(KeyError):
        build.side_library(key + "x")


def test_headers_are_the_same_files_as_the_hand_written_list():
    want = sorted(glob.glob(os.path.join(build.CSRC, "*.h"))) + sorted(glob.glob(os.path.join(build.INCLUDE, "*.h")))
    for d in ("io", "img", "mp", "vw", "lp", "png", "jpg", "jpegdec", "camgrad"):
        want += sorted(glob.glob(os.path.join(build.INCLUDE, d, "*.h")))
    assert build.HEADERS == want and len(set(want)) == len(want)
    # ... and no header under include/ or csrc/ is outside it
    everywhere = glob.glob(os.path.join(build.INCLUDE, "**", "*.h"), recursive=True) + glob.glob(os.path.join(build.CSRC, "*.h"))
    assert sorted(everywhere) == sorted(want)
    assert {os.path.basename(h) for h in want} >= {"host_error.h", "host_align.h", "scg_raster.h"} | {h for h, _ in EXPECTED.values()}


def test_all_pairs_share_no_source_path_or_symbol():
    tables = dict({"main": build.SOURCES}, **{k: build.side_library(k)[1] for k in build.SIDE_LIBRARIES})
    paths = [build.LIB_PATH] + [build.side_library(k)[0] for k in build.SIDE_LIBRARIES]
    assert len(tables) == 10 and len(set(paths)) == 10
    everything = [s for t in tables.values() for s in t]
    assert len(set(everything)) == len(everything)                       # every source belongs to exactly one library
    assert sorted(everything) == sorted(os.path.basename(p) for p in glob.glob(os.path.join(build.CSRC, "*.hip")))
    bound = {k: set(_binding(k).SYMBOLS) for k in tables}
    declared = {k: _header_names(k) for k in tables}
    for a, b in itertools.combinations(tables, 2):
        assert not bound[a] & bound[b] and not declared[a] & declared[b] and not bound[a] & declared[b] and not declared[a] & bound[b], (a, b)


# ---- the one loader, on the real libscg_img.so --------------------------------------------------------------------------------
class _OneByte(C.Structure):
    _fields_ = [("b", C.c_uint8)]


class _FourBytes(C.Structure):
    _fields_ = [("w", C.c_uint32)]


def _open(path=_lib_img.LIB_PATH, symbols=_lib_img.SYMBOLS, version=_lib_img.ABI_VERSION, size_checked=None):
    return _lib.open_library(path, symbols, ("scg_img_abi_version", version), size_checked or {}, "libscg_img.so")


def test_loader_opens_a_side_library_and_the_main_one_by_default():
    assert _open().scg_img_abi_version() == _lib_img.ABI_VERSION
    assert _open(size_checked={"scg_img_abi_version": (_OneByte,)}) is not None   # a query without `which`: the version, 1, as a size
    assert _lib.open_library(_lib.LIB_PATH).scg_abi_version() == _lib.ABI_VERSION


def test_loader_missing_path():
    with pytest.raises(_lib.ScgError, match=r"nowhere/libscg_img\.so not found: the HIP extension is required"):
        _open(path=os.path.join(build.HERE, "nowhere", "libscg_img.so"))


def test_loader_symbol_the_library_lacks():
    with pytest.raises(_lib.ScgError, match=r"libscg_img\.so does not export scg_img_absent$"):
        _open(symbols=dict(_lib_img.SYMBOLS, scg_img_absent=(C.c_int, [])))


def test_loader_wrong_version():
    with pytest.raises(_lib.ScgError, match=r"^ABI version mismatch: libscg_img\.so 1 != binding 2$"):
        _open(version=_lib_img.ABI_VERSION + 1)
    with pytest.raises(_lib.ScgError, match=r"^ABI version mismatch: library 1 != binding 10$"):
        _lib.open_library(_lib_img.LIB_PATH, _lib_img.SYMBOLS, ("scg_img_abi_version", _lib.ABI_VERSION), {})


def test_loader_wrong_struct_size():
    with pytest.raises(_lib.ScgError, match=r"^struct layout mismatch: _FourBytes is 1 bytes in the library, 4 in the binding$"):
        _open(size_checked={"scg_img_abi_version": (_FourBytes,)})


# ---- one error text per library -------------------------------------------------------------------------------------------------
def test_a_failing_png_call_leaves_the_scene_files_error_text_alone():
    io, png = _lib_io.load(), _lib_png.load()
    assert io.scg_ply_layout(-1, 0, C.byref(_lib_io.ScgPlyLayout())) == -2
    before = io.scg_io_last_error()
    assert before.startswith(b"scg_ply_layout: -1 ray-bound")
    assert png.scg_png_layout(1, None, 0, None, None, None) == -1
    assert png.scg_png_last_error() == b"scg_png_layout: out is NULL"
    assert io.scg_io_last_error() == before
    with pytest.raises(_lib.ScgError, match=r"^here failed \(code -1\): scg_png_layout: out is NULL$"):
        _lib_png.check(-1, "here")

"""CPU-only checks of the image resize (scgaussian_amd/images.py, libscg_img.so, include/img/scg_resample.h): the numpy restatement
the GPU tests compare against (tests/resize_refs.py) is held to Pillow itself, byte for byte, and to the fixture recorded from the
reference's PILtoTorch; the package's vectorised tables to the restatement's; loadCam's size arithmetic to its literal text; the
third library and its binding to the header's text, and the library's validation to its codes."""
import os

import numpy as np
import pytest
import torch

import resize_refs as R
from abi_compare import VOID, check_side_library
from scgaussian_amd import _lib, _lib_img, images

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "ref_resize.npz")
LIMIT = images.MAX_KSIZE

# ((win, hin), (wout, hout)): 8x, 4x and non-integer reductions, upscales, one axis unchanged, both unchanged, the smallest
# inputs, an output of size 1, a scale whose ksize is the limit (64 -> 2: 129) and one beyond it (66 -> 2: 133)
SIZES = [((64, 48), (8, 6)), ((64, 48), (16, 12)), ((403, 301), (50, 38)), ((7, 5), (20, 9)), ((40, 30), (40, 12)),
         ((40, 30), (13, 30)), ((40, 30), (40, 30)), ((1, 1), (3, 2)), ((5, 1), (2, 1)), ((1, 5), (1, 2)), ((2, 2), (5, 5)),
         ((33, 20), (1, 1)), ((64, 3), (2, 3)), ((66, 3), (2, 3)), ((21, 9), (8, 20))]


# ---- the restatement against Pillow --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("channels", [0, 3], ids=["L", "RGB"])
@pytest.mark.parametrize("sizes", SIZES, ids=lambda s: f"{s[0][0]}x{s[0][1]}to{s[1][0]}x{s[1][1]}")
def test_restatement_is_pillows_resize(sizes, channels):
    Image = pytest.importorskip("PIL.Image")
    (win, hin), size = sizes
    for make in (R.random_image, R.step_image, R.checker_image):
        src = make(hin, win, channels)
        want = np.asarray(Image.fromarray(src).resize(size))
        got = R.resize(src, size)
        assert got.shape == want.shape and np.array_equal(got, want), make.__name__


def test_ksize_limit_cases_and_both_clamps_act():
    assert R.ksize_of(64, 2) == LIMIT == 129 and R.ksize_of(66, 2) == 133 and R.ksize_of(4032, 504) == 33
    assert images.ksize_of(64, 2) == 129 and images.ksize_of(3024, 756) == 17 and images.ksize_of(7, 20) == 5
    assert images.plan_of((64, 3), (2, 3), 3).device_route and not images.plan_of((66, 3), (2, 3), 3).device_route
    # the step image at 8x drives an accumulator below 0 and above 255 << 22: both clamps decide bytes
    bounds, k = R.coefficients(64, 8)
    for make in (R.step_image, R.checker_image):
        src = make(48, 64, 0).astype(np.int64)
        acc = np.array([[(1 << 21) + int((src[y, b:b + c] * k[i, :c]).sum()) for i, (b, c) in enumerate(bounds)] for y in range(48)])
        assert (acc < 0).any() and ((acc >> 22) > 255).any(), make.__name__
        assert (acc[acc < 0] >> 22).max() <= -1                  # the arithmetic shift keeps a negative accumulator negative


def test_float_intermediate_differs_on_a_planted_image():
    Image = pytest.importorskip("PIL.Image")
    src = R.random_image(24, 32, 0, seed=0)
    want = np.asarray(Image.fromarray(src).resize((8, 6)))
    assert np.array_equal(R.resize(src, (8, 6)), want)
    other = R.resize_float_intermediate(src, (8, 6))
    assert (other != want).sum() >= 1 and np.abs(other.astype(int) - want.astype(int)).max() == 1


# ---- the tables ----------------------------------------------------------------------------------------------------------------
AXES = [(64, 8), (64, 16), (403, 50), (301, 38), (7, 20), (5, 9), (1, 3), (5, 2), (2, 5), (33, 1), (64, 2), (66, 2), (30, 30),
        (4032, 504), (3024, 378), (1600, 400), (4032, 1008)]


@pytest.mark.parametrize("axis", AXES, ids=lambda a: f"{a[0]}to{a[1]}")
def test_tables_sum_to_one_lie_inside_and_equal_the_vectorised_ones(axis):
    in_size, out_size = axis
    bounds, k = R.coefficients(in_size, out_size)
    ksize = R.ksize_of(in_size, out_size)
    assert k.shape == (out_size, ksize) and k.dtype == np.int32 and bounds.shape == (out_size, 2)
    assert np.abs(k.astype(np.int64).sum(axis=1) - (1 << 22)).max() <= ksize
    first, count = bounds[:, 0].astype(np.int64), bounds[:, 1].astype(np.int64)
    assert (first >= 0).all() and (count >= 1).all() and (count <= ksize).all() and (first + count <= in_size).all()
    assert (np.diff(first) >= 0).all()
    for i in range(out_size):
        assert not k[i, count[i]:].any()
    # a strip of the horizontal pass spans at most (STRIP - 1) * scale + 2 + ksize source samples (csrc/resample.hip)
    S = images.STRIP
    for j0 in range(0, out_size, S):
        last = min(j0 + S, out_size) - 1
        assert first[last] + count[last] - first[j0] <= int((S - 1) * (in_size / out_size)) + 2 + ksize
    mine_b, mine_k = images.axis_table(in_size, out_size)
    assert mine_b.dtype == np.int32 and mine_k.dtype == np.int32
    assert np.array_equal(mine_b, bounds) and np.array_equal(mine_k, k)


def test_plan_layout():
    p = images.ResizePlan((403, 301), (50, 38), 3)
    assert (p.hksize, p.vksize, p.pitch, p.image_bytes, p.out_bytes) == (35, 33, 160, 403 * 301 * 3, 50 * 38 * 3)
    assert p.pitch % images.PITCH_ALIGN == 0 and p.mid_bytes(2) == 2 * 301 * 160
    off = p.table_offsets
    assert list(off) == ["hbounds", "hcoeffs", "vbounds", "vcoeffs"] and all(v % 16 == 0 for v in off.values())
    hb, hk = R.coefficients(403, 50)
    vb, vk = R.coefficients(301, 38)
    for name, arr in (("hbounds", hb), ("hcoeffs", hk), ("vbounds", vb), ("vcoeffs", vk)):
        assert np.array_equal(p.tables[off[name]:off[name] + arr.nbytes].view(np.int32), arr.reshape(-1)), name
    assert p.tables_offset(3) % 16 == 0 and p.tables_offset(3) >= 3 * p.image_bytes
    assert p.staged_bytes(3) == p.tables_offset(3) + p.tables.size
    one = images.ResizePlan((40, 30), (40, 12), 1)
    assert list(one.table_offsets) == ["vbounds", "vcoeffs"] and one.mid_bytes(5) == 0 and one.hksize == 0
    same = images.ResizePlan((40, 30), (40, 30), 1)
    assert same.tables.size == 0 and same.device_route
    lib = _lib_img.load()
    assert lib.scg_resample_pitch(50, 3) == p.pitch and lib.scg_resample_mid_bytes(2, 301, 403, 3, 50) == p.mid_bytes(2)
    assert lib.scg_resample_mid_bytes(5, 30, 40, 1, 40) == 0 and lib.scg_resample_pitch(0, 3) == 0 and lib.scg_resample_pitch(5, 2) == 0
    with pytest.raises(_lib.ScgError, match="channels"):
        images.ResizePlan((4, 4), (2, 2), 4)


# ---- loadCam's size arithmetic -------------------------------------------------------------------------------------------------
def _loadcam_resolution(orig_w, orig_h, resolution, resolution_scale):
    """utils/camera_utils.py:25-42, literally (the warning left out)."""
    if resolution in [1, 2, 4, 8]:
        return round(orig_w / (resolution_scale * resolution)), round(orig_h / (resolution_scale * resolution))
    if resolution == -1:
        if orig_w > 1600:
            global_down = orig_w / 1600
        else:
            global_down = 1
    else:
        global_down = orig_w / resolution
    scale = float(global_down) * float(resolution_scale)
    return (int(orig_w / scale), int(orig_h / scale))


def test_target_resolution_is_loadcams_arithmetic():
    for w, h in ((4032, 3024), (1600, 1200), (1601, 1201), (1599, 1200), (800, 800), (5, 3), (1, 1), (3001, 2003), (4000, 3000)):
        for res in (1, 2, 4, 8, -1, 400, 1000, 1600.0, 333, 3):
            for rs in (1.0, 2.0, 0.5, 1.5):
                assert images.target_resolution(w, h, res, rs) == _loadcam_resolution(w, h, res, rs), (w, h, res, rs)
        assert images.target_resolution(w, h, 8) == _loadcam_resolution(w, h, 8, 1.0)
    assert images.target_resolution(4032, 3024, 8) == (504, 378) and images.target_resolution(4032, 3024, 4) == (1008, 756)
    assert images.target_resolution(4032, 3024, -1) == (1600, 1200) and images.target_resolution(1600, 1200, 4) == (400, 300)
    assert images.target_resolution(5, 3, 2) == (2, 2)              # round(2.5), round(1.5): half to even


# ---- the fixture ---------------------------------------------------------------------------------------------------------------
def test_fixture_equals_the_restatement():
    z = np.load(GOLDEN)
    names = [str(n) for n in z["names"]]
    assert len(names) >= 12 and os.path.getsize(GOLDEN) < 100 * 1024 and str(z["pillow"])
    modes = set()
    for name in names:
        src, res, out = z[name + "_src"], tuple(int(v) for v in z[name + "_res"]), z[name + "_out"]
        assert src.dtype == np.uint8 and src.shape[0] <= 48 and src.shape[1] <= 64 and out.dtype == np.float32
        modes.add(src.ndim)
        want = R.float_image(R.resize(src, res))
        assert out.shape == want.shape == (1 if src.ndim == 2 else 3, res[1], res[0])
        assert np.array_equal(out.view(np.uint32), want.view(np.uint32)), name
    assert modes == {2, 3}
    # the float rule for all 256 bytes: torch's division of the byte tensor by the Python float
    b = np.arange(256, dtype=np.uint8).reshape(16, 16)
    assert np.array_equal(R.float_image(b)[0].view(np.uint32), (torch.from_numpy(b) / 255.0).numpy().view(np.uint32))


# ---- the third library against its header --------------------------------------------------------------------------------------
def test_third_library_exports_and_binds_exactly_its_header():
    abi = check_side_library(_lib_img, "img", "scg_resample.h", VOID, prefixes=("scg_img_", "scg_resample_"))
    assert len(abi.functions) == 5 and not abi.structs and not abi.enums
    assert sorted(abi.defines) == sorted("SCG_" + n for n in (
        "IMG_ABI_VERSION", "RESAMPLE_MAX_KSIZE", "RESAMPLE_MAX_SIZE", "RESAMPLE_STRIP", "RESAMPLE_STRIP_ROWS", "RESAMPLE_VTILE",
        "RESAMPLE_PITCH_ALIGN"))


def test_validation_returns_codes_without_a_gpu():
    """Every call below fails its validation before anything touches a device: the pointers are never dereferenced."""
    lib = _lib_img.load()
    fake, big = 0x1000, 1 << 30
    NULL, RANGE, SCRATCH, ALIGN = -1, -2, -4, -5

    def call(src=fake, n=2, hin=30, win=40, ch=3, hout=12, wout=13, hb=fake, hk=fake, hks=9, vb=fake, vk=fake, vks=13, mid=fake,
             mid_bytes=big, out=fake, out_bytes=big, fl=None, fl_bytes=0):
        return lib.scg_resample_u8(src, n, hin, win, ch, hout, wout, hb, hk, hks, vb, vk, vks, mid, mid_bytes, out, out_bytes, fl,
                                   fl_bytes, None)

    assert call(src=None) == NULL and b"src is NULL" in lib.scg_img_last_error()
    assert call(out=None) == NULL and b"out is NULL" in lib.scg_img_last_error()
    for name in ("n", "hin", "win", "hout", "wout"):
        assert call(**{name: 0}) == RANGE and call(**{name: -3}) == RANGE and call(**{name: 65536}) == RANGE, name
    for ch in (0, 2, 4):
        assert call(ch=ch) == RANGE and b"channels" in lib.scg_img_last_error()
    # tables: required for an axis that changes, ignored for one that does not
    assert call(hb=None) == NULL and call(hk=None) == NULL and b"width" in lib.scg_img_last_error()
    assert call(vb=None) == NULL and call(vk=None) == NULL and b"height" in lib.scg_img_last_error()
    assert call(hks=0) == RANGE and call(hks=LIMIT + 1) == RANGE and b"hksize 130" in lib.scg_img_last_error()
    assert call(vks=0) == RANGE and call(vks=LIMIT + 1) == RANGE and b"vksize 130" in lib.scg_img_last_error()
    # the intermediate: n * hin * pitch = 2 * 30 * 48
    assert call(mid=None) == NULL and b"mid is NULL" in lib.scg_img_last_error()
    assert call(mid_bytes=2 * 30 * 48 - 1) == SCRATCH and b"mid of 2879 bytes < 2880" in lib.scg_img_last_error()
    assert call(mid=fake + 8) == ALIGN and b"mid not 16-byte aligned" in lib.scg_img_last_error()
    # the outputs: n * hout * wout * channels = 2 * 12 * 13 * 3 bytes, four times as many for the floats
    assert call(out_bytes=935) == SCRATCH and b"out of 935 bytes < 936" in lib.scg_img_last_error()
    assert call(fl=fake, fl_bytes=4 * 936 - 1) == SCRATCH and b"out_float" in lib.scg_img_last_error()
    assert call(fl=fake + 2, fl_bytes=big) == ALIGN and b"out_float not 4-byte aligned" in lib.scg_img_last_error()
    # a table of a strip that no workgroup's LDS holds
    assert call(win=65535, wout=2, hks=5) == RANGE and b"LDS" in lib.scg_img_last_error()


def test_python_entry_points_refuse_what_the_kernels_do_not_take():
    src = np.zeros((4, 5, 3), np.uint8)
    with pytest.raises(_lib.ScgError, match="ROCm GPU"):
        images.resize_u8(src, (2, 2), device="cpu")
    with pytest.raises(_lib.ScgError, match="not uint8"):
        images.resize_u8(src.astype(np.float32), (2, 2))
    with pytest.raises(_lib.ScgError, match="shape"):
        images.resize_u8(np.zeros((4, 5, 4), np.uint8), (2, 2))
    with pytest.raises(_lib.ScgError, match="one size"):
        images.resize_batch([src, np.zeros((4, 6, 3), np.uint8)], (2, 2))
    with pytest.raises(_lib.ScgError, match="no image"):
        images.resize_batch([], (2, 2))

"""The JPEG stream of include/jpg/scg_jpeg.h without a GPU: the numpy restatement (tests/jpeg_refs.py) held to Pillow's
libjpeg whole file by whole file, a mutant per rule that must break the equality, the quality tables, the quantiser's division; then
the eighth library's header text against its exports and its binding, every argument code, the layout's arithmetic, the header
templates, and the AVI writer parsed back.  Nothing here launches a kernel.

What Pillow settled (recorded in the header's text): a one-component file has one DQT, SOF0 of length 000B with 01 11 00, the two
luminance DHTs and SOS 0008 01 01 00 00 3F 00; DRI is written also when the image has a single MCU row."""
import ctypes as C
import os
import struct

import numpy as np
import pytest

import jpeg_refs as R
from abi_compare import TYPED, check_side_library
from scgaussian_amd import _lib, _lib_jpg, jpeg

u8 = np.uint8
needs_pillow_jpeg = pytest.mark.skipif(not R.pillow_has_jpeg(), reason="Pillow has no JPEG codec here")
SIZES = [(1, 1), (7, 9), (8, 8), (16, 16), (17, 33), (8, 24), (24, 8), (9, 9), (150, 17), (17, 150), (40, 56)]
QUALITIES = (1, 20, 50, 75, 95, 100)


def _kinds(H, W, c, seed):
    """noise, near-flat and a ramp of one size."""
    rng = np.random.default_rng(seed)
    sh = (H, W) if c == 1 else (H, W, 3)
    r = (np.arange(H)[:, None] * 3 + np.arange(W)[None, :] * 5) % 256
    return [rng.integers(0, 256, sh, dtype=u8), (128 + rng.integers(-3, 4, sh)).astype(u8),
            r.astype(u8) if c == 1 else np.stack([r, 255 - r, (r * 2) % 256], -1).astype(u8)]


# ---- the restatement against libjpeg ---------------------------------------------------------------------------------------------------
@needs_pillow_jpeg
@pytest.mark.parametrize("channels", (1, 3))
def test_restatement_is_pillows_file(channels):
    """Whole files: sizes 1 x 1 to 150 x 17, noise / near-flat / ramps, quality 1 to 100, both subsamplings, one and three channels."""
    n = 0
    for k, (H, W) in enumerate(SIZES):
        for img in _kinds(H, W, channels, k):
            for q in QUALITIES:
                for sub in (R.SUBSAMPLINGS if channels == 3 else ("4:4:4",)):
                    assert R.encode(img, q, sub) == R.pillow_encode(img, q, sub), (H, W, channels, q, sub)
                    n += 1
    assert n == len(SIZES) * 3 * len(QUALITIES) * (2 if channels == 3 else 1)


@needs_pillow_jpeg
def test_restatement_is_pillows_file_on_planted_blocks_and_bgr():
    st = R.Stats()
    planted = [(R.checkerboard(8, 16), 100), (R.checkerboard(16, 16, 3), 100), (R.dc_swing(8, 32), 100), (R.last_coefficient(2), 75),
               (np.full((8, 24), 77, u8), 90), (np.random.default_rng(5).integers(0, 256, (8, 8), dtype=u8), 100)]
    for img, q in planted:
        for sub in (R.SUBSAMPLINGS if img.ndim == 3 else ("4:4:4",)):
            assert R.encode(img, q, sub, stats=st) == R.pillow_encode(img, q, sub), (img.shape, q, sub)
    assert st["ac_size10"] and st["dc_size11"] and st["zrl"] >= 6 and st["no_eob"] and st["dc_diff0"] and st["code16"] and st["pad_ff"]
    img = np.random.default_rng(2).integers(0, 256, (17, 33, 3), dtype=u8)
    for sub in R.SUBSAMPLINGS:
        assert R.encode(img, 90, sub, bgr=True) == R.pillow_encode(img, 90, sub, bgr=True) != R.pillow_encode(img, 90, sub)


@needs_pillow_jpeg
def test_single_mcu_row_still_has_dri_and_one_component_layout():
    f = R.pillow_encode(np.zeros((8, 40), u8), 90, "4:4:4")
    assert f[:2] == b"\xff\xd8" and f.count(b"\xff\xdb") == 1 and b"\xff\xdd\x00\x04\x00\x05" in f
    assert b"\xff\xc0\x00\x0b\x08\x00\x08\x00\x28\x01\x01\x11\x00" in f and b"\xff\xda\x00\x08\x01\x01\x00\x00\x3f\x00" in f
    f = R.pillow_encode(np.zeros((16, 16, 3), u8), 90, "4:2:0")
    assert b"\xff\xdd\x00\x04\x00\x01" in f and b"\xff\xc0\x00\x11\x08\x00\x10\x00\x10\x03\x01\x22\x00\x02\x11\x01\x03\x11\x01" in f


@needs_pillow_jpeg
@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_a_mutant_of_each_rule_breaks_the_equality(mutant):
    """pad_mcu_first: the H % 16 == 8 rule; constant_bias: the alternating bias; dummy_dc_zero: the dummy DC chain; pad_unstuffed: the
    pad byte's stuffing.  Each must differ from libjpeg somewhere in a small set, and the true rule nowhere."""
    hit = 0
    if mutant == "pad_unstuffed":
        cases = [(np.random.default_rng(s).integers(0, 256, (8, 8), dtype=u8), "4:4:4") for s in (5, 7, 18, 28)]
    elif mutant == "pad_mcu_first":
        cases = [(np.random.default_rng(s).integers(0, 256, (H, 8, 3), dtype=u8), "4:2:0") for s in range(3) for H in (8, 24)]
    else:
        cases = [(np.random.default_rng(s).integers(0, 256, (H, W, 3), dtype=u8), "4:2:0") for s in range(3) for H, W in ((8, 24), (9, 9))]
    for img, sub in cases:
        want = R.pillow_encode(img, 100, sub)
        assert R.encode(img, 100, sub) == want
        hit += R.encode(img, 100, sub, mutant=mutant) != want
    assert hit >= len(cases) // 2, (mutant, hit)


def test_quality_tables():
    assert [R.quality_scale(q) for q in (1, 20, 49, 50, 75, 100)] == [5000, 250, 102, 100, 50, 0]
    assert np.array_equal(R.quant_table(R.BASE_LUMA, 50), R.BASE_LUMA) and np.array_equal(R.quant_table(R.BASE_CHROMA, 50), R.BASE_CHROMA)
    assert set(R.quant_table(R.BASE_LUMA, 100)) == {1} and R.quant_table(R.BASE_LUMA, 1).max() == 255
    assert R.quant_table(R.BASE_LUMA, 1).min() == 255 and R.quant_table(R.BASE_LUMA, 20)[:4].tolist() == [40, 28, 25, 40]
    assert sorted(R.ZIGZAG.tolist()) == list(range(64)) and R.ZIGZAG[:6].tolist() == [0, 1, 8, 16, 9, 2]
    for bits, vals in (R.DC_LUMA, R.DC_CHROMA, R.AC_LUMA, R.AC_CHROMA):
        codes = R.huffman_codes(bits, vals)
        assert sum(bits) == len(vals) == len(codes) and sum(b << (16 - s) for s, b in enumerate(bits, 1)) < 1 << 16     # a prefix code
    assert R.huffman_codes(*R.AC_LUMA)[0xF0] == (0x7F9, 11) and R.huffman_codes(*R.AC_LUMA)[0x00] == (0xA, 4)


def test_the_quantisers_division_is_exact_and_the_dc_is_the_sum():
    """The kernel divides with the integer `/`; the rule is sign(c) * ((|c| + 4 Q) // (8 Q)) for every coefficient the DCT can give
    (|c| <= 8 * 8 * 128 * 8 / 8 = 8192 * 2) and every Q of a table.  The unquantised DC is the sum of the 64 centred samples."""
    c = np.arange(-16384, 16385, dtype=np.int64)
    for q in range(1, 256):
        got = R.quantise(np.broadcast_to(c[:, None, None], (c.size, 8, 8)), np.full(64, q))[:, 0, 0]
        assert np.array_equal(got, np.sign(c) * np.floor(np.abs(c) / (8.0 * q) + 0.5).astype(np.int64)), q
    b = np.random.default_rng(3).integers(-128, 128, (50, 8, 8))
    assert np.array_equal(R.fdct_islow(b)[:, 0, 0], b.sum(axis=(1, 2)))


# ---- the library: header text, exports, binding -----------------------------------------------------------------------------------------
def test_header_text_exports_and_binding_agree():
    abi = check_side_library(_lib_jpg, "jpg", "scg_jpeg.h", TYPED, prefixes=("scg_jpg_", "scg_jpeg_"), constant_prefixes=("JPG_", "JPEG_"))
    lib = _lib_jpg.load()
    assert lib.scg_jpg_abi_version() == _lib_jpg.ABI_VERSION == abi.defines["SCG_JPG_ABI_VERSION"]
    assert [lib.scg_jpg_struct_bytes(i) for i in range(5)] == [C.sizeof(s) for s in _lib_jpg.STRUCTS] + [0]


def _hwc(shapes):
    return np.ascontiguousarray(np.asarray(shapes, dtype=np.int32)).ctypes.data_as(C.POINTER(C.c_int32))


def test_layout_arithmetic_and_header_templates():
    shapes = [(40, 56, 3), (1, 1, 1), (150, 17, 3), (40, 56, 3), (8, 24, 1)]
    for sub, m in (("4:2:0", 16), ("4:4:4", 8)):
        L, images, segments, headers = jpeg.layout(shapes, 75, sub)
        first = 0
        for i, (H, W, c) in enumerate(shapes):
            mm = m if c == 3 else 8
            im = images[i]
            assert (im["H"], im["W"], im["channels"], im["src"], im["reserved"]) == (H, W, c, 0, 0)
            assert (im["first_segment"], im["segments"], im["mcus"]) == (first, -(-H // mm), -(-W // mm))
            assert im["header_bytes"] == (629 if c == 3 else 334) <= _lib_jpg.JPEG_MAX_HEADER and im["capacity"] == im["header_bytes"] + 3 * H * W
            assert [(s["image"], s["row"]) for s in segments[first:first + im["segments"]]] == [(i, r) for r in range(im["segments"])]
            first += int(im["segments"])
            # the template is the restatement's header: the same bytes as libjpeg's
            tpl = bytes(headers[im["header_offset"]:im["header_offset"] + im["header_bytes"]])
            assert tpl == R.header(H, W, c, 75, sub)
        assert L.segments == first == len(segments) and L.images == len(shapes)
        assert images[3]["header_offset"] == images[0]["header_offset"]                   # one template per distinct shape
        assert L.headers_bytes == 629 * 2 + 334 * 2 == len(headers)
        assert L.capacity == sum(-(-int(c) // 16) * 16 for c in images["capacity"])
        assert L.base_offset == 0 and L.scan_offset == -(-4 * (first + 1) // 16) * 16
        assert L.table_offset == L.scan_offset + -(-4 * len(shapes) // 16) * 16 and L.table_bytes == 16 * (len(shapes) + 1)
        assert L.workspace_bytes == L.table_offset + L.table_bytes
    L, images, _s, _h = jpeg.layout(shapes, 75, "4:2:0", capacities=[1000, 5, 0, 2 ** 32 - 1 - 5000, 17])
    assert images["capacity"].tolist() == [1000, 5, 0, 2 ** 32 - 1 - 5000, 17] and L.capacity == 1008 + 16 + 0 + (2 ** 32 - 4992) + 32
    assert jpeg.layout([])[0].segments == 0
    # what it refuses
    lib = _lib_jpg.load()
    err = lib.scg_jpg_last_error
    L = _lib_jpg.ScgJpegLayout()
    one = _hwc([(1, 1, 1)])
    assert lib.scg_jpeg_layout(1, one, 90, 2, None, None, None, None, None) == -1 and b"out is NULL" in err()
    assert lib.scg_jpeg_layout(1, None, 90, 2, None, C.byref(L), None, None, None) == -1
    assert lib.scg_jpeg_layout(-1, one, 90, 2, None, C.byref(L), None, None, None) == -2
    for q in (0, 101, -5):
        assert lib.scg_jpeg_layout(1, one, q, 2, None, C.byref(L), None, None, None) == -2 and b"quality" in err()
    for sub in (1, 3, -1):
        assert lib.scg_jpeg_layout(1, one, 90, sub, None, C.byref(L), None, None, None) == -2 and b"subsampling" in err()
    for bad in ((0, 5, 3), (5, 0, 3), (65536, 1, 1), (1, 65536, 1), (-3, 4, 1), (4, 4, 2), (4, 4, 4), (4, 4, 0)):
        assert lib.scg_jpeg_layout(2, _hwc([(2, 2, 3), bad]), 90, 2, None, C.byref(L), None, None, None) == -2 and b"image 1" in err()
    assert lib.scg_jpeg_layout(1, _hwc([(65535, 65535, 1)]), 90, 2, None, C.byref(L), None, None, None) == -2 and b"pass capacities" in err()
    assert lib.scg_jpeg_layout(3, _hwc([(30000, 15000, 3)] * 4), 90, 2, None, C.byref(L), None, None, None) == 0
    assert lib.scg_jpeg_layout(4, _hwc([(30000, 15000, 3)] * 4), 90, 2, None, C.byref(L), None, None, None) == -2 and b"2^32" in err()
    with pytest.raises(_lib.ScgError, match="capacities"):
        jpeg.layout(shapes, capacities=[1, 2])


def test_validation_returns_codes_without_a_gpu():
    """Every call below fails its validation before anything touches a device: the device pointers are never dereferenced."""
    lib = _lib_jpg.load()
    err = lib.scg_jpg_last_error
    fake, big = 0x10000, 1 << 26
    shapes = [(40, 56, 3), (1, 1, 1), (300, 400, 1)]
    L, images_np, _segments, _headers = jpeg.layout(shapes, 90, "4:2:0")
    images = (_lib_jpg.ScgJpegImage * len(shapes)).from_buffer(images_np)
    for im in images:
        im.src = fake
    a = _lib_jpg.ScgJpegEncode()
    a.struct_bytes, a.images, a.quality, a.subsampling, a.bgr = C.sizeof(a), len(shapes), 90, _lib_jpg.JPEG_420, 1
    a.headers_bytes = L.headers_bytes
    a.images_host, a.images_dev, a.segments_dev, a.headers_dev = C.addressof(images), fake, fake, fake
    call = lambda buf=fake, nbuf=big, ws=fake, nws=big: lib.scg_jpeg_encode(C.byref(a), buf, nbuf, ws, nws, None)      # noqa: E731
    assert lib.scg_jpeg_encode(None, fake, big, fake, big, None) == -1 and b"args is NULL" in err()
    assert call(buf=None) == -1 and call(ws=None) == -1
    assert call(nbuf=L.capacity - 1) == -4 and b"out of" in err()
    assert call(nws=L.workspace_bytes - 1) == -4 and b"workspace of" in err()
    assert call(buf=fake + 8) == -5 and call(ws=fake + 4) == -5
    a.struct_bytes -= 8
    assert call() == -2 and b"struct_bytes" in err()
    a.struct_bytes += 8
    for field, bad in (("images", 0), ("images", -1), ("images", 2 ** 20 + 1), ("quality", 0), ("quality", 101), ("subsampling", 1),
                       ("subsampling", -1), ("bgr", 2), ("bgr", -1)):
        old = getattr(a, field)
        setattr(a, field, bad)
        assert call() == -2, (field, bad)
        setattr(a, field, old)
    for n in ("images_host", "images_dev", "segments_dev", "headers_dev"):
        old = getattr(a, n)
        setattr(a, n, None)
        assert call() == -1, n
        setattr(a, n, old)
    a.images_dev = fake + 4
    assert call() == -5
    a.images_dev = fake
    a.segments_dev = fake + 2
    assert call() == -5 and b"aligned" in err()
    a.segments_dev = fake
    images[1].W = 0
    assert call() == -2 and b"image 1" in err()
    images[1].W = 1
    images[1].channels = 2
    assert call() == -2
    images[1].channels = 1
    for field in ("first_segment", "segments", "mcus"):
        setattr(images[2], field, getattr(images[2], field) + 1)
        assert call() == -2 and b"the layout gives" in err(), field
        setattr(images[2], field, getattr(images[2], field) - 1)
    images[0].H = 400                                                  # a taller first image moves the segments of those behind it
    assert call() == -2 and b"image 0" in err()
    images[0].H = 40
    for field, bad in (("header_offset", -1), ("header_offset", int(L.headers_bytes) - 300), ("header_bytes", 334), ("header_bytes", 700)):
        old = getattr(images[0], field)
        setattr(images[0], field, bad)
        assert call() == -2 and b"its header" in err(), (field, bad)
        setattr(images[0], field, old)
    images[2].src = 0
    assert call() == -1 and b"image 2 has no pixels" in err()
    images[2].src = fake
    images[2].capacity = 1 << 27                                       # a larger capacity needs a larger buffer
    assert call() == -4 and b"out of" in err()
    images[2].capacity = images_np["capacity"][2]
    a.subsampling = _lib_jpg.JPEG_444                                  # at 4:4:4 the same table is another layout
    assert call() == -2 and b"the layout gives" in err()


def test_python_entry_points_refuse_without_a_gpu():
    import torch
    with pytest.raises(_lib.ScgError, match="no CPU path"):
        jpeg.encode([torch.zeros((4, 4), dtype=torch.uint8)])
    for kw in ({"quality": 0}, {"quality": 101}, {"quality": 7.5}, {"quality": True}, {"subsampling": "4:2:2"}, {"subsampling": 2}):
        with pytest.raises(_lib.ScgError):
            jpeg.encode([], **kw)
    with pytest.raises(_lib.ScgError, match=r"\(N, H, W, 3\)"):
        jpeg.encode(torch.zeros((4, 4, 3), dtype=torch.uint8))
    with pytest.raises(ValueError):
        jpeg.check_route("mp4")
    assert jpeg.check_route("mjpeg") and not jpeg.check_route(None)
    with pytest.raises(ValueError):
        jpeg.check_options(90, "4:2:0", 0)
    assert not jpeg.takes(torch.zeros((4, 4), dtype=torch.uint8)) and not jpeg.takes(np.zeros((4, 4), u8))


@needs_pillow_jpeg
def test_save_jpeg_on_the_host_is_pillows_file(tmp_path):
    import torch
    rng = np.random.default_rng(1)
    for k, a in enumerate((rng.integers(0, 256, (9, 13, 3), dtype=u8), rng.integers(0, 256, (9, 13), dtype=u8))):
        p = str(tmp_path / f"a{k}.jpg")
        jpeg.save_jpeg(p, torch.from_numpy(a), quality=80, subsampling="4:4:4", bgr=True)
        assert open(p, "rb").read() == R.encode(a, 80, "4:4:4", bgr=True)


# ---- the AVI writer ------------------------------------------------------------------------------------------------------------------
def test_write_avi_parses_back(tmp_path):
    rng = np.random.default_rng(4)
    frames = [R.encode(rng.integers(0, 256, (24, 40, 3), dtype=u8), q, "4:2:0") for q in (30, 31, 60, 90, 100)]
    assert {len(f) & 1 for f in frames} == {0, 1}, "the set needs odd and even lengths"
    path = str(tmp_path / "v.avi")
    jpeg.write_avi(path, frames, 30, 40, 24)
    data = open(path, "rb").read()
    avi = R.parse_avi(data)
    assert [f for _p, f in avi["frames"]] == frames and avi["avih"]["total_frames"] == avi["strh"]["length"] == len(frames)
    assert (avi["avih"]["width"], avi["avih"]["height"], avi["avih"]["streams"], avi["avih"]["flags"]) == (40, 24, 1, 0x10)
    assert avi["avih"]["us_per_frame"] == 33333 and (avi["strh"]["rate"], avi["strh"]["scale"]) == (30, 1)
    assert (avi["strh"]["type"], avi["strh"]["handler"]) == (b"vids", b"MJPG")
    assert avi["strf"] == {"size": 40, "width": 40, "height": 24, "planes": 1, "bits": 24, "compression": b"MJPG", "image_bytes": 40 * 24 * 3}
    assert len(avi["index"]) == len(frames)
    for (cid, flags, off, size), (pos, f) in zip(avi["index"], avi["frames"]):
        assert cid == b"00dc" and flags == 0x10 and size == len(f) and avi["movi_offset"] + off == pos and pos % 2 == 0
        assert data[pos:pos + 8] == b"00dc" + struct.pack("<I", len(f))
    jpeg.write_avi(path, frames[:1], 29.97, 40, 24)
    avi = R.parse_avi(open(path, "rb").read())
    assert (avi["strh"]["rate"], avi["strh"]["scale"]) == (2997, 100) and avi["avih"]["us_per_frame"] == 33367
    for bad in (dict(files=[]), dict(files=[b"abcd"]), dict(fps=0), dict(width=0), dict(height=70000)):
        kw = dict(files=frames, fps=30, width=40, height=24)
        kw.update(bad)
        with pytest.raises(ValueError):
            jpeg.write_avi(path, **kw)


def test_write_avi_refuses_more_than_4gib(tmp_path, monkeypatch):
    """No OpenDML: the size is computed before a byte is written."""
    monkeypatch.setattr(jpeg, "AVI_MAX_BYTES", 5000)
    f = R.encode(np.random.default_rng(0).integers(0, 256, (24, 40, 3), dtype=u8), 90, "4:2:0")
    path = str(tmp_path / "big.avi")
    with pytest.raises(ValueError, match="OpenDML"):
        jpeg.write_avi(path, [f] * 4, 30, 40, 24)
    assert not os.path.exists(path)
    assert jpeg.AVI_MAX_BYTES == 5000

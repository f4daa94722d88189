"""The JPEG decoder without a GPU: the numpy restatement of its rule (tests/jpegdec_refs.py) against Pillow's pixels and a mutant of
each rule, jpeg_decode.parse, the header's text against the library's exports and the binding, every argument code, read_avi, and
the decoder's entry of the build table."""
import ctypes as C
import io
import os

import numpy as np
import pytest

import abi_compare
import jpegdec_refs as R
from scgaussian_amd import _lib, _lib_jpegdec, build, jpeg, jpeg_decode

needs_pillow_jpeg = pytest.mark.skipif(not R.pillow_has_jpeg(), reason="Pillow without JPEG")

SIZES = [(1, 1), (2, 2), (7, 9), (8, 8), (16, 16), (17, 33), (8, 24), (24, 8), (9, 9), (3, 50), (37, 53), (40, 56), (15, 31), (32, 17)]


def _grid():
    for (H, W) in SIZES:
        for sampling in R.SAMPLINGS:
            for quality in (20, 90, 100):
                for kind in ("noise", "ramp"):
                    for restart_blocks in (0, 1):
                        yield (H, W, sampling, quality, kind, restart_blocks), R.pillow_file(R.image(H, W, 3, kind), quality, sampling, restart_blocks)
        yield (H, W, "one component"), R.pillow_file(R.image(H, W, 1, "noise"), 90)
        yield (H, W, "optimize"), R.pillow_file(R.image(H, W, 3, "noise"), 90, "4:2:0", optimize=True)
        yield (H, W, "optimize, rows"), R.pillow_file(R.image(H, W, 3, "ramp"), 100, "4:2:2", optimize=True, restart_blocks=2)


# ---- the restatement ---------------------------------------------------------------------------------------------------------------
@needs_pillow_jpeg
def test_restatement_gives_pillows_pixels():
    n = 0
    for what, data in _grid():
        assert np.array_equal(R.decode(data), R.pillow_pixels(data)), what
        n += 1
    assert n >= 504 + 14


def _planted(mutant):
    """Files on which the mutant's rule matters."""
    if mutant == "crop_after_upsampling":
        # an encoder pads with the edge sample, which hides the rule: the writer plants chroma that VARIES into the padding columns
        # and rows of the one MCU (a horizontal and a vertical cosine on Cb and Cr).  The rule shows in the LAST column / row of an
        # even size that is no multiple of the MCU: an odd size ends on an even sample, whose neighbour lies inside.
        files = []
        for sampling, per, H in (("4:2:2", 4, 8), ("4:2:0", 6, 10)):
            blocks = np.zeros((per, 64), dtype=np.int64)
            blocks[per - 2, 1], blocks[per - 1, 2], blocks[:, 0] = 200, -160, 40
            files.append(R.write_file(H, 10, blocks, sampling))
        return files
    if mutant == "biases_swapped":
        return [R.pillow_file(R.image(16, 16, 3, "noise"), 90, "4:2:0")]
    if mutant == "ends_filtered":
        return [R.pillow_file(R.image(16, 16, 3, "noise"), 90, "4:2:2")]
    if mutant == "g_rounding":
        return [R.pillow_file(R.image(16, 16, 3, "noise"), 90, "4:4:4")]
    return [R.pillow_file(R.image(16, 32, 3, "noise"), 90, "4:4:4", restart_blocks=1)]


@needs_pillow_jpeg
@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_a_mutant_of_each_rule_breaks_the_equality(mutant):
    files = _planted(mutant)
    for data in files:
        assert np.array_equal(R.decode(data), R.pillow_pixels(data))
    assert any(not np.array_equal(R.decode(data, mutant), R.pillow_pixels(data)) for data in files)


def test_the_writer_and_the_reader_of_the_restatement_agree():
    rng = np.random.default_rng(3)
    for sampling, per in ((None, 1), ("4:4:4", 3), ("4:2:2", 4), ("4:2:0", 6)):
        H, W = 19, 35
        hs, vs = (1, 1) if sampling is None else R.SAMPLINGS[sampling]
        mcus = -(-W // (8 * hs)) * -(-H // (8 * vs))
        blocks = rng.integers(-40, 41, size=(mcus * per, 64)) * (rng.random((mcus * per, 64)) < 0.3)
        for ri in (0, 1, 3):
            data = R.write_file(H, W, blocks, sampling, ri=ri)
            m = R.read_markers(data)
            m["data"] = data
            got = R.entropy_decode(m)
            assert np.array_equal(got[:, R.ZIGZAG], blocks), (sampling, ri)


# ---- parse -------------------------------------------------------------------------------------------------------------------------
@needs_pillow_jpeg
def test_parse_accepts_what_the_rule_names():
    for sampling, (h, v) in R.SAMPLINGS.items():
        for optimize in (False, True):
            data = R.pillow_file(R.image(17, 33, 3, "noise"), 90, sampling, restart_blocks=2, optimize=optimize)
            info = jpeg_decode.parse(data)
            assert info is not None and (info.H, info.W, info.components, info.h, info.v, info.restart_interval) == (17, 33, 3, h, v, 2)
            assert list(info.frame) == [17, 33, 3, h, v, 2, 0, 1, 1, 0, 1, 1, 0, 1, 1, 0]
            m = R.read_markers(data)
            assert (info.segment_start, info.segment_end) == (m["start"], m["end"])
            assert all(np.array_equal(info.quant[k], m["quant"][k]) for k in (0, 1)) and info.huffman == m["huffman"]
    one = jpeg_decode.parse(R.pillow_file(R.image(9, 9, 1, "noise"), 90))
    assert (one.components, one.h, one.v) == (1, 1, 1) and list(one.frame[6:]) == [0] * 10


@needs_pillow_jpeg
def test_parse_bounds_the_segment_with_stuffing_and_restart_markers_inside():
    data = R.pillow_file(R.image(40, 56, 3, "noise"), 100, "4:4:4", restart_blocks=1)
    info = jpeg_decode.parse(data)
    seg = data[info.segment_start:info.segment_end]
    assert data[info.segment_start - 3:info.segment_start] == b"\x00\x3f\x00" and data[info.segment_end:info.segment_end + 2] == b"\xff\xd9"
    assert b"\xff\x00" in seg and b"\xff\xd0" in seg and b"\xff\xd7" in seg
    assert info.segment_end + 2 == len(data)
    # bytes behind EOI change nothing
    assert jpeg_decode.parse(data + b"tail\xff\xd9")[-2:] == info[-2:]


def _patch(data: bytes, marker: int, offset: int, value: int) -> bytes:
    at = data.index(bytes([0xFF, marker]))
    return data[:at + offset] + bytes([value]) + data[at + offset + 1:]


@needs_pillow_jpeg
def test_parse_refuses_what_the_rule_does_not_name():
    from PIL import Image
    img = R.image(16, 16, 3, "noise")
    good = R.pillow_file(img, 90, "4:2:2")
    assert jpeg_decode.parse(good) is not None
    refused = {
        "progressive": R.pillow_file(img, 90, "4:2:0", progressive=True),
        # (Pillow's encoder takes 4:4:4, 4:2:2 and 4:2:0 only — subsampling="4:4:0" raises in 12.2.0 — so the 4:4:0 frame is a 4:2:2
        # file with Y's sampling factors patched to 1 x 2; parse never reads the entropy data, which no longer fits the frame)
        "4:4:0": _patch(good, 0xC0, 11, 0x12),
        "4:1:1": _patch(good, 0xC0, 11, 0x41),
        "chroma 2x1": _patch(good, 0xC0, 14, 0x21),
        "12 bit": _patch(good, 0xC0, 4, 12),
        "16-bit DQT": _patch(good, 0xDB, 4, 0x10),
        "arithmetic": _patch(good, 0xC0, 1, 0xC9),
        "extended": _patch(good, 0xC0, 1, 0xC1),
        "spectral selection": _patch(good, 0xDA, 11, 1),
        "successive approximation": _patch(good, 0xDA, 13, 0x10),
        "Huffman table id 2": _patch(good, 0xC4, 4, 0x02),
        "truncated": good[:len(good) - 20],
        "no EOI": good[:-2],
        "not a JPEG": b"\x89PNG" + good,
        "empty": b"",
    }
    buf = io.BytesIO()
    Image.fromarray(np.zeros((8, 8, 4), dtype=np.uint8), "CMYK").save(buf, format="JPEG")
    refused["CMYK"] = buf.getvalue()
    two_scans = good[:-2] + good[good.index(b"\xff\xda"):]
    refused["two scans"] = two_scans
    for what, data in refused.items():
        assert jpeg_decode.parse(data) is None, what


def test_huffman_table_is_the_header_blocks_and_refuses_a_full_code():
    bits, vals = R.AC_LUMA
    t = jpeg_decode.huffman_table(bits, vals)
    look = t[:512].view(np.uint16)
    maxcode, valoff = t[512:576].view(np.int32), t[576:640].view(np.int32)
    for sym, (code, size) in R.huffman_codes(bits, vals).items():
        if size <= 8:
            assert all(look[(code << (8 - size)) + j] == (size << 8) | sym for j in range(1 << (8 - size)))
        assert code <= maxcode[size - 1] and t[640 + code + valoff[size - 1]] == sym
    assert look[0xFF] == 0 and (maxcode[[0, 12, 13]] == -1).all()                 # no code of 1, 13 or 14 bits
    assert jpeg_decode.huffman_table([2] + [0] * 15, [0, 1]) is None              # 0 and 1: all ones is a code word
    assert jpeg_decode.huffman_table([1, 1] + [0] * 14, [0, 1]) is not None
    assert jpeg_decode.huffman_table([0, 5] + [0] * 14, list(range(5))) is None   # five codes of two bits


# ---- the ABI -----------------------------------------------------------------------------------------------------------------------
def test_header_text_exports_and_binding_agree():
    abi = abi_compare.check_side_library(_lib_jpegdec, "jpegdec", "scg_jpegdec.h", abi_compare.ANY)
    assert not abi.structs
    assert R.SUBSEQ == _lib_jpegdec.JPEGDEC_SUBSEQ and R.THREADS == _lib_jpegdec.JPEGDEC_THREADS


def _frame(**kw):
    words = dict(H=16, W=16, comps=3, h=2, v=2, ri=0, tq=(0, 1, 1), td=(0, 1, 1), ta=(0, 1, 1), last=0)
    words.update(kw)
    arr = np.array([words["H"], words["W"], words["comps"], words["h"], words["v"], words["ri"], *words["tq"], *words["td"], *words["ta"],
                    words["last"]], dtype=np.int32)
    return arr, arr.ctypes.data_as(C.POINTER(C.c_int32))


def test_every_argument_code_without_a_launch():
    lib = _lib_jpegdec.load()
    err = lib.scg_jpegdec_last_error
    ws, ob, mr = C.c_uint64(), C.c_uint64(), C.c_int32()
    keep, good = _frame()
    assert lib.scg_jpegdec_sizes(good, 1000, C.byref(ws), C.byref(ob), C.byref(mr)) == 0
    assert ob.value == 16 * 16 * 3 and mr.value == 1 and ws.value % 256 == 0 and ws.value > 6 * 128 + 3 * 256
    assert lib.scg_jpegdec_sizes(good, 128 * 256 + 1, C.byref(ws), C.byref(ob), C.byref(mr)) == 0 and mr.value == 3
    assert lib.scg_jpegdec_sizes(None, 1000, C.byref(ws), C.byref(ob), C.byref(mr)) == -1 and b"frame is NULL" in err()
    assert lib.scg_jpegdec_sizes(good, 1000, None, C.byref(ob), C.byref(mr)) == -1 and b"output is NULL" in err()
    bad_frames = [dict(H=0), dict(W=65536), dict(comps=2), dict(comps=4), dict(h=3), dict(h=1, v=2), dict(comps=1), dict(ri=-1),
                  dict(ri=65536), dict(tq=(4, 0, 0)), dict(td=(0, 2, 0)), dict(ta=(0, 0, -1)), dict(last=1)]
    for kw in bad_frames:
        k, f = _frame(**kw)
        assert lib.scg_jpegdec_sizes(f, 1000, C.byref(ws), C.byref(ob), C.byref(mr)) == -2, kw
    for seg in (0, _lib_jpegdec.JPEGDEC_MAX_SEGMENT + 1):
        assert lib.scg_jpegdec_sizes(good, seg, C.byref(ws), C.byref(ob), C.byref(mr)) == -2 and b"segment" in err()
    k, f = _frame(H=65535, W=65535, h=1, v=1)
    assert lib.scg_jpegdec_sizes(f, 1000, C.byref(ws), C.byref(ob), C.byref(mr)) == -2 and b"blocks" in err()

    assert lib.scg_jpegdec_sizes(good, 1000, C.byref(ws), C.byref(ob), C.byref(mr)) == 0
    fake = 0x10000

    def call(frame=good, header=fake, seg=fake, nseg=1000, out=fake, nout=None, work=fake, nwork=None, done=0, rounds=1):
        return lib.scg_jpegdec_decode(frame, header, seg, nseg, out, ob.value if nout is None else nout, work,
                                      ws.value if nwork is None else nwork, done, rounds, None)

    assert call(frame=None) == -1
    for kw in bad_frames:
        k, f = _frame(**kw)
        assert call(frame=f) == -2, kw
    assert call(nseg=0) == -2
    assert call(header=None) == -1 and b"header_dev is NULL" in err()
    assert call(header=fake + 8) == -5
    assert call(seg=None) == -1 and b"segment_dev is NULL" in err()
    assert call(out=None) == -1 and call(out=fake + 4) == -5
    assert call(nout=ob.value - 1) == -4 and b"out of" in err()
    assert call(work=None) == -1 and call(work=fake + 8) == -5
    assert call(nwork=ws.value - 1) == -4 and b"workspace of" in err()
    assert call(rounds=0) == -2 and call(done=-1) == -2
    assert call(rounds=2) == -2 and call(done=1, rounds=1) == -2 and b"settle" in err()     # one workgroup: the one launch `sizes` names


def test_python_entry_points_refuse_without_a_gpu():
    with pytest.raises(_lib.ScgError, match="ROCm GPU"):
        jpeg_decode.decode(b"\xff\xd8\xff\xd9", device="cpu")
    with pytest.raises(_lib.ScgError, match="16 int32"):
        jpeg_decode.JpegDecodePlan(np.zeros(3, dtype=np.int32), "cuda")
    from scgaussian_amd import images
    with pytest.raises(_lib.ScgError, match="decode must be"):
        images.install(object(), decode="host")
    keep, f = _frame()
    assert jpeg_decode.sizes(keep, 1000)[1:] == (768, 1)


# ---- read_avi ----------------------------------------------------------------------------------------------------------------------
def test_read_avi_returns_what_write_avi_wrote(tmp_path):
    files = [b"\xff\xd8" + bytes(range(n)) + b"\xff\xd9" for n in (0, 1, 6, 7, 200)]
    path = str(tmp_path / "v.avi")
    jpeg.write_avi(path, files, 24, 32, 16)
    assert jpeg.read_avi(path) == files
    import jpeg_refs
    assert [f for _at, f in jpeg_refs.parse_avi(open(path, "rb").read())["frames"]] == files
    (tmp_path / "not.avi").write_bytes(b"RIFF\x04\x00\x00\x00WAVE")
    with pytest.raises(ValueError, match="not a RIFF AVI"):
        jpeg.read_avi(str(tmp_path / "not.avi"))


# ---- the build ---------------------------------------------------------------------------------------------------------------------
def test_the_decoder_is_one_entry_of_the_side_library_table():
    assert len(build.SOURCES) == 17 and "jpegunpack.hip" not in build.SOURCES
    assert abi_compare.side_header("jpegdec", "scg_jpegdec.h") in build.HEADERS
    assert build.SIDE_LIBRARIES["jpegdec"] == ("jpegdec", {"jpegunpack.hip": ["-ffp-contract=off"]})
    src = open(os.path.join(build.CSRC, "jpegunpack.hip")).read()
    included = {line.split('"')[1] for line in src.splitlines() if line.startswith('#include "')}
    assert included == {"../../include/jpegdec/scg_jpegdec.h", "compact.h", "host_align.h", "host_error.h"}

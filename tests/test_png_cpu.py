"""The PNG stream of include/png/scg_png.h without a GPU: the numpy restatement (tests/png_refs.py) held to zlib and Pillow, the code
lengths to the Kraft sum and to a heapq Huffman tree, the planted histograms, the size bound; then the seventh library's header
text against its exports and its binding, every argument code, and the layout's arithmetic.  Nothing here launches a kernel."""
import ctypes as C
import heapq
import zlib

import numpy as np
import pytest

import png_refs as R
from abi_compare import TYPED, check_side_library
from scgaussian_amd import _lib, _lib_png

CH = R.CHUNK
u8 = np.uint8


def _images():
    """(name, image): random, smooth, constant, step and noise, one and three channels, from 1 x 1 up to three chunks."""
    rng = np.random.default_rng(0)
    yy, xx = np.mgrid[0:150, 0:217]
    smooth = ((np.sin(xx / 23.0) + np.cos(yy / 17.0)) * 60 + 128).astype(u8)
    step = ((xx // 40 + yy // 50) * 37 % 256).astype(u8)
    out = [("1x1", np.array([[7]], u8)), ("1x1x3", np.array([[[0, 255, 3]]], u8)), ("row", rng.integers(0, 256, (1, 300), dtype=u8)),
           ("column", rng.integers(0, 256, (300, 1), dtype=u8)),
           ("random", (rng.integers(0, 6, (90, 110, 3)) * 40).astype(u8)),            # few values, short runs: 3 chunks as RGB
           ("smooth", smooth), ("smooth3", np.stack([smooth, smooth[::-1], 255 - smooth], axis=2)),
           ("constant", np.full((120, 250), 200, u8)), ("constant3", np.full((60, 180, 3), 9, u8)),
           ("step", step), ("noise", rng.integers(0, 256, (100, 109, 3), dtype=u8)), ("noise1", rng.integers(0, 256, (180, 181), dtype=u8))]
    assert max(R.stream_geometry(*R.as_hwc(a).shape, True)[2] for _n, a in out) == 3
    return out


IMAGES = _images()


def _files(filt, gray):
    """Every image of the list through the restatement once per (filter, gray_as_rgb): (name, image, file, chunk dicts)."""
    key = (filt, gray)
    if key not in _files.cache:
        rows = []
        for name, a in IMAGES:
            ch = []
            rows.append((name, a, R.png_file(a, filt, gray, ch), ch))
        _files.cache[key] = rows
    return _files.cache[key]


_files.cache = {}
MODES = [(f, g) for f in R.FILTERS for g in (True, False)]          # one channel with and without gray_as_rgb; three channels in both


@pytest.mark.parametrize("filt,gray", MODES)
def test_zlib_and_pillow_decode_every_stream(filt, gray):
    kinds = set()
    for name, a, f, ch in _files(filt, gray):
        idat = R.idat_of(f)
        assert zlib.decompress(idat) == R.filtered_stream(a, filt, gray).tobytes(), name          # this verifies the Adler-32
        assert np.array_equal(R.decode_with_pillow(f), R.expected_pixels(a, gray)), name
        assert idat[:2] == b"\x78\x01" and len(f) == 41 + len(idat) + 4 + 12
        kinds |= {c["kind"] for c in ch}
    assert kinds == {"stored", "dynamic"}


def _heap_cost(freq):
    heap = [int(f) for f in freq if f]
    heapq.heapify(heap)
    cost = 0
    while len(heap) > 1:
        s = heapq.heappop(heap) + heapq.heappop(heap)
        cost += s
        heapq.heappush(heap, s)
    return cost


@pytest.mark.parametrize("filt,gray", MODES)
def test_code_lengths_kraft_sum_cost_and_size_bound(filt, gray):
    seen = 0
    for name, a, f, ch in _files(filt, gray):
        S = R.stream_geometry(*R.as_hwc(a).shape, gray)[1]
        assert len(R.idat_of(f)) <= S + 5 * len(ch) + 6, name
        assert sum(c["n"] for c in ch) == S and all(c["n"] == CH for c in ch[:-1])
        for c in ch:
            lengths, freq = c["lengths"], c["freq"]
            assert all((l > 0) == (fr > 0) for l, fr in zip(lengths, freq)) and max(lengths) <= 15
            assert sum(1 << (15 - l) for l in lengths if l) == 1 << 15, name                    # Kraft sum exactly 1
            if c["deepest"] <= 15:
                assert sum(l * int(fr) for l, fr in zip(lengths, freq)) == _heap_cost(freq), name
                seen += 1
            assert c["bytes"] <= c["n"] + 5 and (c["kind"] == "stored") == (c["dynamic_bytes"] >= c["n"] + 5)
    assert seen > 10


def test_planted_histograms():
    """The Fibonacci chunk of 28 656 bytes as stated: under "the leaf on a tie" its unlimited tree is 11 deep (every step of the merge
    ties; a rule that took the merged node instead would give 21), so it stays an optimal code.  The Lucas chunk ties nowhere: 19
    deep, limited to 15, repaired to a Kraft sum of 1, dearer than the unlimited code, and it still decodes."""
    d = R.fibonacci_stream()
    ch = []
    f = R.png_file(R.image_of_stream(d), R.NONE, False, ch)
    assert d.size == 28656 and len(set(d.tolist())) == 21 and ch[0]["matches"] == 0 and ch[0]["tokens"] == d.size
    assert sorted(int(x) for x in ch[0]["freq"] if x)[:5] == [1, 1, 1, 2, 3] and ch[0]["deepest"] == 11
    assert zlib.decompress(R.idat_of(f)) == d.tobytes() and np.array_equal(R.decode_with_pillow(f), R.image_of_stream(d))
    d = R.lucas_stream()
    ch = []
    f = R.png_file(R.image_of_stream(d), R.NONE, False, ch)
    c = ch[0]
    assert d.size <= 28656 and c["matches"] == 0 and c["deepest"] == 19 > 15 and max(c["lengths"]) == 15 and c["kind"] == "dynamic"
    assert sum(1 << (15 - l) for l in c["lengths"] if l) == 1 << 15
    assert sum(l * int(fr) for l, fr in zip(c["lengths"], c["freq"])) > _heap_cost(c["freq"])
    assert zlib.decompress(R.idat_of(f)) == d.tobytes() and np.array_equal(R.decode_with_pillow(f), R.image_of_stream(d))


def test_tokens_of_planted_runs():
    """The token rule on runs around its thresholds, position by position."""
    for n, want in ((1, "L"), (3, "LLL"), (4, "L3"), (5, "L4"), (258, "L257"), (259, "L258"), (260, "L258 L"), (261, "L258 LL"),
                    (262, "L258 3"), (1 + 2 * 258, "L258 258"), (1 + 2 * 258 + 2, "L258 258 LL"), (1 + 2 * 258 + 3, "L258 258 3")):
        sym, ebits, evals, is_match = R.chunk_tokens(np.zeros(n, u8))
        got = []
        for s, e, v, m in zip(sym, ebits, evals, is_match):
            got.append(str(R.LEN_BASE[s - 257] + v) if m else "L")
        assert "".join(got) == want.replace(" ", ""), n
    sym, *_ = R.chunk_tokens(R.runs_stream([5, 1, 300]))
    assert list(sym) == [0, 258, 7, 14, 285, 273]                        # 0, match 4, 7, 14, match 258, match 41 (35 + 6)


# ---- the header's text, the library, the binding -----------------------------------------------------------------------------------
def test_seventh_library_exports_and_binds_exactly_its_header():
    abi = check_side_library(_lib_png, "png", "scg_png.h", TYPED)
    assert len(abi.functions) == 5 and len(abi.structs) == 5 and len(abi.defines) == 17
    assert not any(f.array for fields in abi.structs.values() for f in fields)
    assert [_lib_png.load().scg_png_struct_bytes(k) for k in range(-1, 6)] == [0, 80, 32, 8, 16, 40, 0]
    assert [C.sizeof(s) for s in _lib_png.STRUCTS] == [80, 32, 8, 16, 40]
    assert _lib_png.PNG_CHUNK == CH and _lib_png.PNG_HEADER_BITS == R.HEADER_BITS == 17 + 19 * 3 + 288 * 4
    assert (_lib_png.PNG_FILTER_NONE, _lib_png.PNG_FILTER_SUB, _lib_png.PNG_FILTER_UP, _lib_png.PNG_FILTER_PAETH) == R.FILTERS


# ---- the layout ---------------------------------------------------------------------------------------------------------------------
def _hwc(shapes):
    return (C.c_int32 * (3 * len(shapes)))(*[x for s in shapes for x in s])


def _layout(shapes, gray=1, tables=True):
    lib = _lib_png.load()
    L = _lib_png.ScgPngLayout()
    rc = lib.scg_png_layout(len(shapes), _hwc(shapes), gray, C.byref(L), None, None)
    if rc or not tables:
        return rc, L, None, None
    images, chunks = (_lib_png.ScgPngImage * len(shapes))(), (_lib_png.ScgPngChunk * max(int(L.chunks), 1))()
    rc = lib.scg_png_layout(len(shapes), _hwc(shapes), gray, C.byref(L), images, chunks)
    return rc, L, images, chunks


def _a16(v):
    return (v + 15) // 16 * 16


def test_layout_arithmetic():
    lib = _lib_png.load()
    for shapes in ([(1, 1, 1)], [(1, 1, 3)], [(1, 32767, 1)], [(3, 10922, 3), (3, 10923, 3)], [(1200, 1600, 3), (1200, 1600, 1)] * 3,
                   [(1, 1, 1)] * 1025, [(65535, 10922, 3)], [(40, 56, 3), (1, 1, 1), (300, 400, 1)]):
        for gray in (1, 0):
            rc, L, images, chunks = _layout(shapes, gray)
            assert rc == 0
            geo = [R.stream_geometry(h, w, c, bool(gray)) for h, w, c in shapes]
            S, k = [g[1] for g in geo], [g[2] for g in geo]
            n, nc = len(shapes), sum(k)
            assert (L.images, L.chunks) == (n, nc) and L.capacity == 16 * n + sum(s + 5 * kk + 6 for s, kk in zip(S, k))
            assert L.lengths_offset == 0 and L.info_offset == _a16(288 * nc) and L.base_offset == _a16(L.info_offset + 16 * nc)
            assert L.scan_offset == _a16(L.base_offset + 4 * (nc + 1)) and L.table_offset == _a16(L.scan_offset + 4 * n)
            assert L.table_bytes == 8 * (n + 1) and L.workspace_bytes == _a16(L.table_offset + L.table_bytes)
            for i, im in enumerate(images):
                assert (im.src, im.H, im.W, im.channels) == (0,) + tuple(shapes[i])
                assert (im.first_chunk, im.chunks, im.stream_bytes) == (sum(k[:i]), k[i], S[i])
            flat = [(i, j) for i in range(n) for j in range(k[i])]
            assert [(chunks[q].image, chunks[q].index) for q in range(nc)] == flat
    rc, L, _i, _c = _layout([], 1, tables=False)                                      # an empty batch
    assert rc == 0 and (L.images, L.chunks, L.capacity) == (0, 0, 0)
    # what it refuses
    err = lib.scg_png_last_error
    assert lib.scg_png_layout(1, _hwc([(1, 1, 1)]), 1, None, None, None) == -1 and b"out is NULL" in err()
    assert lib.scg_png_layout(1, None, 1, C.byref(L), None, None) == -1
    assert lib.scg_png_layout(-1, _hwc([(1, 1, 1)]), 1, C.byref(L), None, None) == -2
    assert lib.scg_png_layout(1, _hwc([(1, 1, 1)]), 2, C.byref(L), None, None) == -2
    for bad in ((0, 5, 3), (5, 0, 3), (65536, 1, 1), (1, 65536, 1), (-3, 4, 1), (4, 4, 2), (4, 4, 4), (4, 4, 0)):
        assert _layout([(2, 2, 3), bad])[0] == -2 and b"image 1" in err()
    assert _layout([(65535, 65535, 1)], 0)[0] == -2 and b"2^31" in err()               # a stream beyond 2^31 - 1
    assert _layout([(65535, 32767, 1)], 0)[0] == 0 and _layout([(65535, 32767, 1)], 1)[0] == -2
    assert _layout([(65535, 10922, 3)] * 3)[0] == -2 and b"2^32" in err()              # two that overflow the 32-bit offsets together


# ---- validation, without a GPU ------------------------------------------------------------------------------------------------------
def test_validation_returns_codes_without_a_gpu():
    """Every call below fails its validation before anything touches a device: the device pointers are never dereferenced."""
    lib = _lib_png.load()
    err = lib.scg_png_last_error
    fake, big = 0x10000, 1 << 26
    shapes = [(40, 56, 3), (1, 1, 1), (300, 400, 1)]
    rc, L, images, _chunks = _layout(shapes)
    assert rc == 0
    for im in images:
        im.src = fake
    a = _lib_png.ScgPngEncode()
    a.struct_bytes, a.images, a.filter, a.gray_as_rgb = C.sizeof(a), len(shapes), _lib_png.PNG_FILTER_UP, 1
    a.images_host, a.images_dev, a.chunks_dev = C.addressof(images), fake, fake
    call = lambda buf=fake, nbuf=big, ws=fake, nws=big: lib.scg_png_encode(C.byref(a), buf, nbuf, ws, nws, None)      # noqa: E731
    assert lib.scg_png_encode(None, fake, big, fake, big, None) == -1 and b"args is NULL" in err()
    # buffers
    assert call(buf=None) == -1 and call(ws=None) == -1
    assert call(nbuf=L.capacity - 1) == -4 and b"out of" in err()
    assert call(nws=L.workspace_bytes - 1) == -4 and b"workspace of" in err()
    assert call(buf=fake + 8) == -5 and call(ws=fake + 4) == -5
    # the struct and the scalars
    a.struct_bytes -= 8
    assert call() == -2 and b"struct_bytes" in err()
    a.struct_bytes += 8
    for field, bad in (("images", 0), ("images", -1), ("images", 2 ** 20 + 1), ("filter", 3), ("filter", 5), ("filter", -1),
                       ("gray_as_rgb", 2), ("gray_as_rgb", -1)):
        old = getattr(a, field)
        setattr(a, field, bad)
        assert call() == -2, (field, bad)
        setattr(a, field, old)
    # null and misaligned tables
    for n in ("images_host", "images_dev", "chunks_dev"):
        old = getattr(a, n)
        setattr(a, n, None)
        assert call() == -1, n
        setattr(a, n, old)
    a.images_dev = fake + 4
    assert call() == -5
    a.images_dev = fake
    a.chunks_dev = fake + 2
    assert call() == -5 and b"aligned" in err()
    a.chunks_dev = fake
    # the image table: a size out of range, a record that is not the layout's, an image without pixels
    images[1].W = 0
    assert call() == -2 and b"image 1" in err()
    images[1].W = 1
    images[1].channels = 2
    assert call() == -2
    images[1].channels = 1
    for field in ("first_chunk", "chunks", "stream_bytes"):
        setattr(images[2], field, getattr(images[2], field) + 1)
        assert call() == -2 and b"the layout gives" in err(), field
        setattr(images[2], field, getattr(images[2], field) - 1)
    images[0].H = 400                                                  # a taller first image moves the chunks of those behind it
    assert call() == -2 and b"image 0" in err()
    images[0].H = 40
    images[2].src = 0
    assert call() == -1 and b"image 2 has no pixels" in err()
    images[2].src = fake
    # with gray_as_rgb off the same table is another layout
    a.gray_as_rgb = 0
    assert call() == -2 and b"the layout gives" in err()


def test_python_entry_points_refuse_without_a_gpu():
    import torch

    from scgaussian_amd import png
    with pytest.raises(_lib.ScgError, match="no CPU path"):
        png.encode([torch.zeros((4, 4), dtype=torch.uint8)])
    with pytest.raises(ValueError):
        png.check_route("zlib")
    assert png.check_route("device") and not png.check_route("pillow")
    assert not png.takes(torch.zeros((4, 4), dtype=torch.uint8)) and not png.takes(np.zeros((4, 4), u8))
    assert png.file_header(3, 5, 2, 77) == R.png_file(np.zeros((3, 5, 3), u8))[:33] + (77).to_bytes(4, "big") + b"IDAT"


def test_save_png_on_the_host_is_pillows_file(tmp_path):
    """CPU tensors and arrays go to Pillow as before: the file is evaluate._save_png's, byte for byte."""
    import torch

    from scgaussian_amd import evaluate, png
    rng = np.random.default_rng(1)
    for k, a in enumerate((rng.integers(0, 256, (9, 13, 3), dtype=u8), rng.integers(0, 256, (9, 13), dtype=u8))):
        png.save_png(str(tmp_path / f"a{k}.png"), torch.from_numpy(a))
        evaluate._save_png(str(tmp_path / f"b{k}.png"), a)
        assert open(tmp_path / f"a{k}.png", "rb").read() == open(tmp_path / f"b{k}.png", "rb").read()

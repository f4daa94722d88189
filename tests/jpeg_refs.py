"""The JPEG stream of include/jpg/scg_jpeg.h restated in numpy, one function per rule, and a small RIFF parser for the
Motion-JPEG files of jpeg.write_avi.  tests/test_jpeg_cpu.py holds this file to Pillow (libjpeg-turbo) byte for byte; tests/test_gpu_jpeg.py
holds the kernels to it.  `encode(..., mutant=NAME)` breaks one rule on purpose: a test shows that the sweep notices.

A Stats object counts what a stream exercised, so that a test set can assert that every branch of the coder was walked.
"""
from __future__ import annotations

import struct
from collections import Counter

import numpy as np

# natural index of zigzag position k
ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35,
                   42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62,
                   63])
# ITU-T T.81 Annex K.1, natural (row-major) order
BASE_LUMA = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87,
                      80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92,
                      95, 98, 112, 100, 103, 99])
BASE_CHROMA = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99,
                        99, 99, 99] + [99] * 32)
# Annex K.3: (BITS, HUFFVAL) of the four tables
DC_LUMA = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12)))
DC_CHROMA = ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12)))
AC_LUMA = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125],
           [1, 2, 3, 0, 4, 17, 5, 18, 33, 49, 65, 6, 19, 81, 97, 7, 34, 113, 20, 50, 129, 145, 161, 8, 35, 66, 177, 193, 21, 82, 209, 240, 36,
            51, 98, 114, 130, 9, 10, 22, 23, 24, 25, 26, 37, 38, 39, 40, 41, 42, 52, 53, 54, 55, 56, 57, 58, 67, 68, 69, 70, 71, 72, 73, 74,
            83, 84, 85, 86, 87, 88, 89, 90, 99, 100, 101, 102, 103, 104, 105, 106, 115, 116, 117, 118, 119, 120, 121, 122, 131, 132, 133,
            134, 135, 136, 137, 138, 146, 147, 148, 149, 150, 151, 152, 153, 154, 162, 163, 164, 165, 166, 167, 168, 169, 170, 178, 179,
            180, 181, 182, 183, 184, 185, 186, 194, 195, 196, 197, 198, 199, 200, 201, 202, 210, 211, 212, 213, 214, 215, 216, 217, 218,
            225, 226, 227, 228, 229, 230, 231, 232, 233, 234, 241, 242, 243, 244, 245, 246, 247, 248, 249, 250])
AC_CHROMA = ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119],
             [0, 1, 2, 3, 17, 4, 5, 33, 49, 6, 18, 65, 81, 7, 97, 113, 19, 34, 50, 129, 8, 20, 66, 145, 161, 177, 193, 9, 35, 51, 82, 240, 21,
              98, 114, 209, 10, 22, 36, 52, 225, 37, 241, 23, 24, 25, 26, 38, 39, 40, 41, 42, 53, 54, 55, 56, 57, 58, 67, 68, 69, 70, 71, 72,
              73, 74, 83, 84, 85, 86, 87, 88, 89, 90, 99, 100, 101, 102, 103, 104, 105, 106, 115, 116, 117, 118, 119, 120, 121, 122, 130,
              131, 132, 133, 134, 135, 136, 137, 138, 146, 147, 148, 149, 150, 151, 152, 153, 154, 162, 163, 164, 165, 166, 167, 168, 169,
              170, 178, 179, 180, 181, 182, 183, 184, 185, 186, 194, 195, 196, 197, 198, 199, 200, 201, 202, 210, 211, 212, 213, 214, 215,
              216, 217, 218, 226, 227, 228, 229, 230, 231, 232, 233, 234, 242, 243, 244, 245, 246, 247, 248, 249, 250])
SUBSAMPLINGS = ("4:4:4", "4:2:0")
MUTANTS = ("pad_mcu_first", "constant_bias", "dummy_dc_zero", "pad_unstuffed")


class Stats(Counter):
    """ff_stuffed, pad_ff, zrl, code16, ac_size10, dc_size11, dc_diff0, no_eob, dummy_right, dummy_bottom, dummy_corner, segments,
    blocks, window_straddle (code words that cross a multiple of WINDOW_BITS of their segment), long_segments (more than one window)."""


WINDOW_BITS = 8 * 16384            # the kernels' LDS window (SCG_JPEG_WINDOW bytes)


# ---- 2.2 tables --------------------------------------------------------------------------------------------------------------------
def quality_scale(q: int) -> int:
    return 5000 // q if q < 50 else 200 - 2 * q


def quant_table(base: np.ndarray, q: int) -> np.ndarray:
    """Natural order."""
    return np.clip((base.astype(np.int64) * quality_scale(q) + 50) // 100, 1, 255)


def huffman_codes(bits, vals) -> dict:
    """symbol -> (code, size): T.81 Annex C."""
    out, code, k = {}, 0, 0
    for size in range(1, 17):
        for _ in range(bits[size - 1]):
            out[vals[k]] = (code, size)
            code += 1
            k += 1
        code <<= 1
    return out


# ---- 2.3 planes --------------------------------------------------------------------------------------------------------------------
def ycc(rgb: np.ndarray):
    r, g, b = (rgb[..., i].astype(np.int64) for i in range(3))
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + 8388608 + 32767) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + 8388608 + 32767) >> 16
    return y, cb, cr


def full_samples(plane: np.ndarray, rows: int, cols: int) -> np.ndarray:
    """rows x cols samples of a full-resolution plane: outside the image the last row / column."""
    H, W = plane.shape
    return plane[np.minimum(np.arange(rows), H - 1)[:, None], np.minimum(np.arange(cols), W - 1)[None, :]]


def chroma_samples(plane: np.ndarray, rows: int, cols: int, mutant=None) -> np.ndarray:
    """rows x cols samples of a plane downsampled 2 x 2.  Columns: the full plane is padded on the right, then averaged.  Rows: the
    plane is padded to an even count, averaged, and the last AVERAGED row is repeated."""
    H, W = plane.shape
    cy, cx = np.arange(rows), np.arange(cols)
    if mutant != "pad_mcu_first":
        cy = np.minimum(cy, (H + 1) // 2 - 1)
    y0, y1 = np.minimum(2 * cy, H - 1), np.minimum(2 * cy + 1, H - 1)
    x0, x1 = np.minimum(2 * cx, W - 1), np.minimum(2 * cx + 1, W - 1)
    bias = np.full_like(cx, 2) if mutant == "constant_bias" else 1 + (cx & 1)
    s = plane[y0[:, None], x0[None, :]] + plane[y0[:, None], x1[None, :]] + plane[y1[:, None], x0[None, :]] + plane[y1[:, None], x1[None, :]]
    return (s + bias[None, :]) >> 2


# ---- 2.4 blocks --------------------------------------------------------------------------------------------------------------------
def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _dct_pass(d, first: bool):
    """One pass of jfdctint.c over the last axis of d (..., 8)."""
    d = [d[..., i] for i in range(8)]
    t0, t7, t1, t6 = d[0] + d[7], d[0] - d[7], d[1] + d[6], d[1] - d[6]
    t2, t5, t3, t4 = d[2] + d[5], d[2] - d[5], d[3] + d[4], d[3] - d[4]
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    n = 13 - 2 if first else 13 + 2
    o = [None] * 8
    if first:
        o[0], o[4] = (t10 + t11) << 2, (t10 - t11) << 2
    else:
        o[0], o[4] = _descale(t10 + t11, 2), _descale(t10 - t11, 2)
    z1 = (t12 + t13) * 4433
    o[2], o[6] = _descale(z1 + t13 * 6270, n), _descale(z1 - t12 * 15137, n)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * 9633
    t4, t5, t6, t7 = t4 * 2446, t5 * 16819, t6 * 25172, t7 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    o[7], o[5], o[3], o[1] = _descale(t4 + z1 + z3, n), _descale(t5 + z2 + z4, n), _descale(t6 + z2 + z3, n), _descale(t7 + z1 + z4, n)
    return np.stack(o, axis=-1)


def fdct_islow(blocks: np.ndarray) -> np.ndarray:
    """(..., 8, 8) centred samples -> 8 x the DCT, libjpeg's jfdctint.c: rows first, then columns."""
    a = _dct_pass(blocks.astype(np.int64), True)
    return np.swapaxes(_dct_pass(np.swapaxes(a, -1, -2), False), -1, -2)


def quantise(coef: np.ndarray, q: np.ndarray) -> np.ndarray:
    """coef (..., 8, 8), q natural order: sign(c) * ((|c| + 4 Q) // (8 Q))."""
    q = q.reshape(8, 8).astype(np.int64)
    return np.sign(coef) * ((np.abs(coef) + 4 * q) // (8 * q))


def plane_blocks(samples: np.ndarray, q: np.ndarray) -> np.ndarray:
    """(8 hb, 8 wb) samples -> (hb, wb, 64) quantised coefficients in zigzag order."""
    hb, wb = samples.shape[0] // 8, samples.shape[1] // 8
    b = samples.reshape(hb, 8, wb, 8).swapaxes(1, 2) - 128
    return quantise(fdct_islow(b), q).reshape(hb, wb, 64)[..., ZIGZAG]


def geometry(H: int, W: int, channels: int, subsampling: str):
    """(MCU rows, MCUs per row, [(h, v) per component])."""
    if channels == 1:
        return (H + 7) // 8, (W + 7) // 8, [(1, 1)]
    if subsampling == "4:4:4":
        return (H + 7) // 8, (W + 7) // 8, [(1, 1)] * 3
    return (H + 15) // 16, (W + 15) // 16, [(2, 2), (1, 1), (1, 1)]


def mcu_blocks(img: np.ndarray, quality: int, subsampling: str, stats: Stats, mutant=None):
    """[MCU row][block in MCU order] -> (component, 64 zigzag coefficients); dummy blocks by jccoefct.c's rule."""
    H, W = img.shape[:2]
    channels = 1 if img.ndim == 2 else img.shape[2]
    rows, cols, comps = geometry(H, W, channels, subsampling)
    ql, qc = quant_table(BASE_LUMA, quality), quant_table(BASE_CHROMA, quality)
    planes = [img.reshape(H, W).astype(np.int64)] if channels == 1 else list(ycc(img))
    out = []
    if len(comps) == 3 and comps[0] == (2, 2):
        hb, wb = (H + 7) // 8, (W + 7) // 8                        # the real luminance blocks
        yb = plane_blocks(full_samples(planes[0], 8 * hb, 8 * wb), ql)
        cb = plane_blocks(chroma_samples(planes[1], 8 * rows, 8 * cols, mutant), qc)
        cr = plane_blocks(chroma_samples(planes[2], 8 * rows, 8 * cols, mutant), qc)
        for my in range(rows):
            seg = []
            for mx in range(cols):
                first = len(seg)
                for v in range(2):
                    for h in range(2):
                        by, bx = 2 * my + v, 2 * mx + h
                        if by < hb and bx < wb:
                            seg.append((0, yb[by, bx]))
                            continue
                        stats["dummy_corner" if by >= hb and bx >= wb else "dummy_bottom" if by >= hb else "dummy_right"] += 1
                        d = np.zeros(64, dtype=np.int64)
                        if mutant != "dummy_dc_zero":
                            d[0] = seg[-1][1][0]                    # the block before it in MCU order (len(seg) > first: Y00 is real)
                        assert len(seg) > first
                        seg.append((0, d))
                seg.append((1, cb[my, mx]))
                seg.append((2, cr[my, mx]))
            out.append(seg)
        return out
    qs = [ql, qc, qc]
    blocks = [plane_blocks(full_samples(p, 8 * rows, 8 * cols), qs[c]) for c, p in enumerate(planes)]
    for my in range(rows):
        out.append([(c, blocks[c][my, mx]) for mx in range(cols) for c in range(len(planes))])
    return out


# ---- 2.5 entropy coding ------------------------------------------------------------------------------------------------------------
def _size(v: int) -> int:
    return int(abs(int(v))).bit_length()


class BitWriter:
    def __init__(self, stats: Stats):
        self.acc, self.n, self.out, self.stats, self.pos = 0, 0, bytearray(), stats, 0

    def _byte(self, b: int, stuff: bool = True):
        self.out.append(b)
        if b == 0xFF and stuff:
            self.out.append(0)
            self.stats["ff_stuffed"] += 1

    def put(self, code: int, size: int):
        if size and self.pos // WINDOW_BITS != (self.pos + size - 1) // WINDOW_BITS:
            self.stats["window_straddle"] += 1
        self.pos += size
        self.acc = (self.acc << size) | code
        self.n += size
        while self.n >= 8:
            self.n -= 8
            self._byte((self.acc >> self.n) & 0xFF)
        self.acc &= (1 << self.n) - 1

    def flush(self, stuff_pad: bool = True):
        if self.n:
            b = ((self.acc << (8 - self.n)) | ((1 << (8 - self.n)) - 1)) & 0xFF
            if b == 0xFF:
                self.stats["pad_ff"] += 1
            self._byte(b, stuff_pad)
            self.acc = self.n = 0


def encode_segment(blocks, tables, stats: Stats, mutant=None) -> bytes:
    """One restart interval: DC predictors from 0, T.81 F.1.2, 1-padding, FF 00."""
    w = BitWriter(stats)
    pred = [0, 0, 0]
    for comp, z in blocks:
        dc_t, ac_t = tables[0 if comp == 0 else 1]
        stats["blocks"] += 1
        diff = int(z[0]) - pred[comp]
        pred[comp] = int(z[0])
        s = _size(diff)
        stats["dc_size11"] += s == 11
        stats["dc_diff0"] += s == 0
        w.put(*dc_t[s])
        if s:
            w.put((diff if diff > 0 else diff - 1) & ((1 << s) - 1), s)
        run = 0
        for k in range(1, 64):
            v = int(z[k])
            if v == 0:
                run += 1
                continue
            while run > 15:
                w.put(*ac_t[0xF0])
                stats["zrl"] += 1
                stats["code16"] += ac_t[0xF0][1] == 16
                run -= 16
            s = _size(v)
            stats["ac_size10"] += s == 10
            stats["code16"] += ac_t[(run << 4) | s][1] == 16
            code, size = ac_t[(run << 4) | s]
            w.put((code << s) | ((v if v > 0 else v - 1) & ((1 << s) - 1)), size + s)      # one word: code and value
            run = 0
        if run:
            w.put(*ac_t[0])
        else:
            stats["no_eob"] += 1
    stats["long_segments"] += w.pos > WINDOW_BITS
    w.flush(mutant != "pad_unstuffed")
    return bytes(w.out)


# ---- 2.1 the file ------------------------------------------------------------------------------------------------------------------
def _dht(cls_id: int, table) -> bytes:
    bits, vals = table
    return b"\xff\xc4" + struct.pack(">HB", 3 + 16 + len(vals), cls_id) + bytes(bits) + bytes(vals)


def header(H: int, W: int, channels: int, quality: int, subsampling: str) -> bytes:
    rows, cols, comps = geometry(H, W, channels, subsampling)
    out = b"\xff\xd8\xff\xe0\x00\x10JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00"
    out += b"\xff\xdb\x00\x43\x00" + bytes(quant_table(BASE_LUMA, quality)[ZIGZAG].astype(np.uint8))
    if channels == 3:
        out += b"\xff\xdb\x00\x43\x01" + bytes(quant_table(BASE_CHROMA, quality)[ZIGZAG].astype(np.uint8))
    out += b"\xff\xc0" + struct.pack(">HBHHB", 8 + 3 * len(comps), 8, H, W, len(comps))
    for i, (h, v) in enumerate(comps):
        out += bytes([i + 1, (h << 4) | v, 0 if i == 0 else 1])
    out += _dht(0x00, DC_LUMA) + _dht(0x10, AC_LUMA)
    if channels == 3:
        out += _dht(0x01, DC_CHROMA) + _dht(0x11, AC_CHROMA)
    out += b"\xff\xdd\x00\x04" + struct.pack(">H", cols)
    if channels == 3:
        out += b"\xff\xda\x00\x0c\x03\x01\x00\x02\x11\x03\x11\x00\x3f\x00"
    else:
        out += b"\xff\xda\x00\x08\x01\x01\x00\x00\x3f\x00"
    return out


_TABLES = None


def tables():
    global _TABLES
    if _TABLES is None:
        _TABLES = [(huffman_codes(*DC_LUMA), huffman_codes(*AC_LUMA)), (huffman_codes(*DC_CHROMA), huffman_codes(*AC_CHROMA))]
    return _TABLES


def encode(img: np.ndarray, quality: int = 90, subsampling: str = "4:2:0", bgr: bool = False, stats: Stats = None, mutant=None) -> bytes:
    """The complete file of an (H, W), (H, W, 1) or (H, W, 3) uint8 image."""
    assert mutant is None or mutant in MUTANTS
    stats = Stats() if stats is None else stats
    img = np.asarray(img)
    assert img.dtype == np.uint8
    if img.ndim == 3 and img.shape[2] == 1:
        img = img[:, :, 0]
    if img.ndim == 3 and bgr:
        img = img[:, :, ::-1]
    H, W = img.shape[:2]
    channels = 1 if img.ndim == 2 else 3
    out = bytearray(header(H, W, channels, quality, subsampling))
    segs = mcu_blocks(img, quality, subsampling, stats, mutant)
    for i, seg in enumerate(segs):
        out += encode_segment(seg, tables(), stats, mutant)
        stats["segments"] += 1
        out += b"\xff\xd9" if i == len(segs) - 1 else bytes([0xFF, 0xD0 + (i & 7)])
    return bytes(out)


def pillow_encode(img: np.ndarray, quality: int, subsampling: str, bgr: bool = False) -> bytes:
    """The same image through Pillow (libjpeg): the outside authority."""
    import io

    from PIL import Image
    img = np.asarray(img)
    if img.ndim == 3 and img.shape[2] == 1:
        img = img[:, :, 0]
    if img.ndim == 3 and bgr:
        img = np.ascontiguousarray(img[:, :, ::-1])
    b = io.BytesIO()
    kw = {} if img.ndim == 2 else {"subsampling": {"4:4:4": 0, "4:2:0": 2}[subsampling]}
    Image.fromarray(img).save(b, format="JPEG", quality=quality, optimize=False, restart_marker_rows=1, **kw)
    return b.getvalue()


def pillow_has_jpeg() -> bool:
    try:
        from PIL import features
        return bool(features.check("jpg"))
    except Exception:
        return False


# ---- planted images ----------------------------------------------------------------------------------------------------------------
def checkerboard(H: int, W: int, channels: int = 1) -> np.ndarray:
    """0 / 255 per pixel: after the level shift the largest AC magnitudes (size-10 values at quality 100)."""
    a = (((np.arange(H)[:, None] + np.arange(W)[None, :]) & 1) * 255).astype(np.uint8)
    return a if channels == 1 else np.repeat(a[:, :, None], 3, axis=2)


def dc_swing(H: int, W: int) -> np.ndarray:
    """Flat 8 x 8 blocks alternating 0 and 255: DC differences of +-2040 at quality 100 (size 11)."""
    return ((((np.arange(H)[:, None] // 8) + (np.arange(W)[None, :] // 8)) & 1) * 255).astype(np.uint8)


def last_coefficient(n_blocks: int = 1, amplitude: float = 100.0) -> np.ndarray:
    """One-channel 8 x 8 n blocks whose only AC energy is the (7, 7) basis function: at quality 50 to 90 the single non-zero AC is
    zigzag 63 (three ZRLs, no EOB; the rounding of the pixels quantises to zero everywhere else)."""
    c = np.cos((2 * np.arange(8) + 1) * 7 * np.pi / 16)
    b = np.clip(np.rint(128 + amplitude * np.outer(c, c)), 0, 255).astype(np.uint8)
    return np.tile(b, (1, n_blocks))


# ---- RIFF ---------------------------------------------------------------------------------------------------------------------------
def parse_avi(data: bytes) -> dict:
    """A Motion-JPEG AVI as jpeg.write_avi writes it -> {avih, strh, strf, frames, index, movi_offset}."""
    assert data[:4] == b"RIFF" and data[8:12] == b"AVI ", "not a RIFF AVI"
    assert struct.unpack("<I", data[4:8])[0] == len(data) - 8, "RIFF size"
    out = {"frames": [], "index": []}

    def walk(lo, hi):
        p = lo
        while p < hi:
            cid, size = data[p:p + 4], struct.unpack("<I", data[p + 4:p + 8])[0]
            body = p + 8
            assert body + size <= hi, f"chunk {cid!r} runs past its parent"
            if cid == b"LIST":
                kind = data[body:body + 4]
                if kind == b"movi":
                    out["movi_offset"] = body            # of the 'movi' fourcc: idx1 offsets count from here
                walk(body + 4, body + size)
            elif cid == b"avih":
                f = struct.unpack("<14I", data[body:body + 56])
                out["avih"] = {"us_per_frame": f[0], "flags": f[3], "total_frames": f[4], "streams": f[6], "width": f[8], "height": f[9]}
            elif cid == b"strh":
                out["strh"] = {"type": data[body:body + 4], "handler": data[body + 4:body + 8],
                               "scale": struct.unpack("<I", data[body + 20:body + 24])[0],
                               "rate": struct.unpack("<I", data[body + 24:body + 28])[0],
                               "length": struct.unpack("<I", data[body + 32:body + 36])[0]}
            elif cid == b"strf":
                f = struct.unpack("<IiiHH4sI", data[body:body + 24])
                out["strf"] = {"size": f[0], "width": f[1], "height": f[2], "planes": f[3], "bits": f[4], "compression": f[5],
                               "image_bytes": f[6]}
            elif cid == b"00dc":
                out["frames"].append((p, data[body:body + size]))
            elif cid == b"idx1":
                for q in range(body, body + size, 16):
                    out["index"].append((data[q:q + 4],) + struct.unpack("<III", data[q + 4:q + 16]))
            p = body + size + (size & 1)
        assert p == hi, "chunks do not tile their parent"

    walk(12, len(data))
    return out

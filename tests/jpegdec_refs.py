"""The JPEG decoder's rule restated in numpy (include/jpegdec/scg_jpegdec.h states it; the kernels of csrc/jpegunpack.hip
are held to this file byte for byte, and this file to np.asarray(Image.open(...)) of Pillow on libjpeg-turbo).

    decode(data, mutant=None)          the pixels of a baseline file: uint8 (H, W, 3) or (H, W)
    write_file(...), Scan              the restatement's own entropy WRITER: files with planted streams, and counters (Stats) that
                                       say which of the planted situations occurred, relative to the kernels' subsequence borders

The rule:
  entropy decoding   T.81 F.2.2; FF 00 is one FF byte; at RSTn the reader skips behind the marker, the DC predictors become 0, a
                     new MCU starts
  dequantisation     coefficient * table entry
  inverse DCT        jidctint "islow": FIX(x) = round(x * 8192), PASS1_BITS = 2; columns with a rounded shift by 11, rows with a
                     rounded shift by 18, + 128, clamp (libjpeg's C table wraps outside an encoder's range, its SIMD code and the
                     kernel saturate: equality with Pillow is claimed only where those agree); (x + (1 << (s - 1))) >> s
  chroma planes      cropped to ceil(W / 2) columns (2x1, 2x2) and ceil(H / 2) rows (2x2) BEFORE upsampling; a neighbour beyond an
                     edge is the edge sample
  2x1                out[2i] = (3 c[i] + c[i-1] + 1) >> 2, out[2i+1] = (3 c[i] + c[i+1] + 2) >> 2; first and last output sample are
                     the first and last input sample
  2x2                s[i] = 3 near[i] + far[i] (far: the row above for even output rows, below for odd ones);
                     out[2i] = (3 s[i] + s[i-1] + 8) >> 4, out[2i+1] = (3 s[i] + s[i+1] + 7) >> 4; a missing neighbour is s[i]
  colour             R = Y + ((91881 (Cr-128) + 32768) >> 16), B = Y + ((116130 (Cb-128) + 32768) >> 16),
                     G = Y + ((-22554 (Cb-128) - 46802 (Cr-128) + 32768) >> 16), clamped
"""
import functools
import io
from collections import Counter

import numpy as np

import jpeg_refs
from jpeg_refs import AC_CHROMA, AC_LUMA, DC_CHROMA, DC_LUMA, ZIGZAG, huffman_codes

SUBSEQ = 128                   # SCG_JPEGDEC_SUBSEQ
THREADS = 256                  # SCG_JPEGDEC_THREADS
MUTANTS = ("crop_after_upsampling", "biases_swapped", "ends_filtered", "g_rounding", "predictors_kept")
SAMPLINGS = {"4:4:4": (1, 1), "4:2:2": (2, 1), "4:2:0": (2, 2)}
STD_TABLES = {(0, 0): DC_LUMA, (1, 0): AC_LUMA, (0, 1): DC_CHROMA, (1, 1): AC_CHROMA}


class Stats(Counter):
    pass


# ---- reading -----------------------------------------------------------------------------------------------------------------------
def _u16(b, at):
    return (b[at] << 8) | b[at + 1]


def read_markers(data: bytes) -> dict:
    """The tables, the frame and the entropy-coded segment of a baseline file with one scan (no checks beyond what decode needs)."""
    assert data[:2] == b"\xff\xd8"
    at, out = 2, {"quant": {}, "huffman": {}, "ri": 0}
    while True:
        assert data[at] == 0xFF
        marker, length = data[at + 1], _u16(data, at + 2)
        body = data[at + 4:at + 2 + length]
        if marker == 0xC0:
            out["H"], out["W"] = _u16(body, 1), _u16(body, 3)
            out["comps"] = [(body[6 + 3 * i], body[7 + 3 * i] >> 4, body[7 + 3 * i] & 15, body[8 + 3 * i]) for i in range(body[5])]
        elif marker == 0xC4:
            p = 0
            while p < len(body):
                bits = list(body[p + 1:p + 17])
                out["huffman"][(body[p] >> 4, body[p] & 15)] = (bits, list(body[p + 17:p + 17 + sum(bits)]))
                p += 17 + sum(bits)
        elif marker == 0xDB:
            p = 0
            while p < len(body):
                q = np.zeros(64, dtype=np.int64)
                q[ZIGZAG] = list(body[p + 1:p + 65])
                out["quant"][body[p] & 15] = q
                p += 65
        elif marker == 0xDD:
            out["ri"] = _u16(body, 0)
        elif marker == 0xDA:
            ns = body[0]
            out["scan"] = [(body[1 + 2 * i], body[2 + 2 * i] >> 4, body[2 + 2 * i] & 15) for i in range(ns)]
            out["start"] = at + 2 + length
            break
        at += 2 + length
    end = out["start"]
    while not (data[end] == 0xFF and data[end + 1] != 0 and not 0xD0 <= data[end + 1] <= 0xD7):
        end += 1
    out["end"] = end
    return out


class _Bits:
    def __init__(self, chunk: bytes):
        chunk = chunk.replace(b"\xff\x00", b"\xff")
        self.total = 8 * len(chunk)
        self.value = int.from_bytes(chunk, "big") << 32           # zero bits behind the end
        self.at = 0

    def peek(self, n: int) -> int:
        return (self.value >> (self.total + 32 - self.at - n)) & ((1 << n) - 1)

    def take(self, n: int) -> int:
        v = self.peek(n) if n else 0
        self.at += n
        assert self.at <= self.total, "the segment ends inside a symbol"
        return v


def _symbol(bits: _Bits, codes: dict) -> int:
    for ln in range(1, 17):
        sym = codes.get((ln, bits.peek(ln)))
        if sym is not None:
            bits.take(ln)
            return sym
    raise ValueError("a code no table holds")


def _extend(v: int, size: int) -> int:
    return v - (1 << size) + 1 if size and v < (1 << (size - 1)) else v


def entropy_decode(m: dict, mutant=None) -> np.ndarray:
    """(blocks, 64) int64 quantised coefficients in NATURAL order, blocks in stream (MCU) order."""
    comps = m["comps"]
    hs, vs = (comps[0][1], comps[0][2]) if len(comps) == 3 else (1, 1)
    per_mcu = [0] * (hs * vs) + ([1, 2] if len(comps) == 3 else [])
    mcus = -(-m["W"] // (8 * hs)) * -(-m["H"] // (8 * vs))
    decode_tables = {k: {(size, code): s for s, (code, size) in huffman_codes(*t).items()} for k, t in m["huffman"].items()}
    seg = m["data"][m["start"]:m["end"]]
    chunks, at = [], 0
    while True:                                        # split at the restart markers
        nxt = at
        while True:
            nxt = seg.find(b"\xff", nxt)
            if nxt < 0 or (nxt + 1 < len(seg) and 0xD0 <= seg[nxt + 1] <= 0xD7):
                break
            nxt += 2
        chunks.append(seg[at:] if nxt < 0 else seg[at:nxt])
        if nxt < 0:
            break
        at = nxt + 2
    ri = m["ri"] or mcus
    assert len(chunks) == -(-mcus // ri), (len(chunks), mcus, ri)
    out = np.zeros((mcus * len(per_mcu), 64), dtype=np.int64)
    pred = [0, 0, 0]
    b = 0
    for ci, chunk in enumerate(chunks):
        bits = _Bits(chunk)
        if mutant != "predictors_kept":
            pred = [0, 0, 0]
        for _ in range(min(ri, mcus - ci * ri)):
            for comp in per_mcu:
                _cid, td, ta = m["scan"][comp]
                size = _symbol(bits, decode_tables[(0, td)])
                pred[comp] += _extend(bits.take(size), size)
                out[b, 0] = pred[comp]
                k = 1
                while k < 64:
                    sym = _symbol(bits, decode_tables[(1, ta)])
                    run, size = sym >> 4, sym & 15
                    if size == 0:
                        if run != 15:
                            break
                        k += 16
                        continue
                    k += run
                    assert k < 64, "a run past coefficient 63"
                    out[b, ZIGZAG[k]] = _extend(bits.take(size), size)
                    k += 1
                b += 1
    return out


def _fits(*values):
    """The kernel computes in int32: an input that leaves it (no encoder's output does) is no test of the rule."""
    for v in values:
        assert np.abs(v).max(initial=0) < 2 ** 31, "the inverse DCT leaves int32"


def _idct_1d(d, shift):
    """d: (..., 8) along the last axis; libjpeg's jidctint.c, one pass."""
    d = [d[..., i] for i in range(8)]
    z2, z3 = d[2], d[6]
    z1 = (z2 + z3) * 4433
    tmp2, tmp3 = z1 + z3 * -15137, z1 + z2 * 6270
    tmp0, tmp1 = (d[0] + d[4]) * 8192, (d[0] - d[4]) * 8192
    tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    tmp0, tmp1, tmp2, tmp3 = d[7], d[5], d[3], d[1]
    z1, z2, z3, z4 = tmp0 + tmp3, tmp1 + tmp2, tmp0 + tmp2, tmp1 + tmp3
    z5 = (z3 + z4) * 9633
    tmp0, tmp1, tmp2, tmp3 = tmp0 * 2446, tmp1 * 16819, tmp2 * 25172, tmp3 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    tmp0, tmp1, tmp2, tmp3 = tmp0 + z1 + z3, tmp1 + z2 + z4, tmp2 + z2 + z3, tmp3 + z1 + z4
    _fits(z5, z1, z2, z3, z4, tmp0, tmp1, tmp2, tmp3, tmp10, tmp11, tmp12, tmp13, d[7] * 2446, d[5] * 16819, d[3] * 25172, d[1] * 12299)
    half = 1 << (shift - 1)
    outs = [tmp10 + tmp3, tmp11 + tmp2, tmp12 + tmp1, tmp13 + tmp0, tmp13 - tmp0, tmp12 - tmp1, tmp11 - tmp2, tmp10 - tmp3]
    _fits(*[np.abs(o) + half for o in outs])
    return np.stack([(o + half) >> shift for o in outs], axis=-1)


def idct_islow(coef: np.ndarray) -> np.ndarray:
    """(n, 64) dequantised int64, natural order -> (n, 8, 8) uint8 samples.  int32 wrap-around does not occur below the sizes a
    baseline stream can carry; the kernel computes in int32."""
    blocks = coef.reshape(-1, 8, 8)
    cols = _idct_1d(blocks.transpose(0, 2, 1), 11).transpose(0, 2, 1)        # along the columns
    rows = _idct_1d(cols, 18)
    return np.clip(rows + 128, 0, 255).astype(np.uint8)


def upsample_h2v1(c: np.ndarray, mutant=None) -> np.ndarray:
    c = c.astype(np.int64)
    left = np.concatenate([c[:, :1], c[:, :-1]], axis=1)
    right = np.concatenate([c[:, 1:], c[:, -1:]], axis=1)
    even, odd = (3 * c + left + 1) >> 2, (3 * c + right + 2) >> 2
    out = np.stack([even, odd], axis=2).reshape(c.shape[0], -1)
    if mutant != "ends_filtered":
        out[:, 0], out[:, -1] = c[:, 0], c[:, -1]
    else:                                              # the mutant takes a zero beyond the edge
        out[:, 0], out[:, -1] = (3 * c[:, 0] + 1) >> 2, (3 * c[:, -1] + 2) >> 2
    return out


def upsample_h2v2(c: np.ndarray, mutant=None) -> np.ndarray:
    c = c.astype(np.int64)
    above = np.concatenate([c[:1], c[:-1]], axis=0)
    below = np.concatenate([c[1:], c[-1:]], axis=0)
    s = np.stack([3 * c + above, 3 * c + below], axis=1).reshape(-1, c.shape[1])          # output rows 2r, 2r + 1
    left = np.concatenate([s[:, :1], s[:, :-1]], axis=1)
    right = np.concatenate([s[:, 1:], s[:, -1:]], axis=1)
    b_even, b_odd = (7, 8) if mutant == "biases_swapped" else (8, 7)
    even, odd = (3 * s + left + b_even) >> 4, (3 * s + right + b_odd) >> 4
    return np.stack([even, odd], axis=2).reshape(s.shape[0], -1)


def ycc_to_rgb(y, cb, cr, mutant=None) -> np.ndarray:
    y, cb, cr = y.astype(np.int64), cb.astype(np.int64) - 128, cr.astype(np.int64) - 128
    r = y + ((91881 * cr + 32768) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    if mutant == "g_rounding":                         # each product rounded on its own
        g = y + ((-22554 * cb + 32768) >> 16) + ((-46802 * cr + 32768) >> 16)
    else:
        g = y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    return np.clip(np.stack([r, g, b], axis=2), 0, 255).astype(np.uint8)


def planes_of(m: dict, coef: np.ndarray):
    """The padded component planes from the blocks in stream order."""
    comps = m["comps"]
    hs, vs = (comps[0][1], comps[0][2]) if len(comps) == 3 else (1, 1)
    mx, my = -(-m["W"] // (8 * hs)), -(-m["H"] // (8 * vs))
    bpm = hs * vs + (2 if len(comps) == 3 else 0)
    qs = [m["quant"][c[3]] for c in comps]
    blocks = coef.reshape(my, mx, bpm, 64)
    y = idct_islow((blocks[:, :, :hs * vs] * qs[0]).reshape(-1, 64)).reshape(my, mx, vs, hs, 8, 8)
    planes = [y.transpose(0, 2, 4, 1, 3, 5).reshape(my * vs * 8, mx * hs * 8)]
    for c in range(1, len(comps)):
        p = idct_islow((blocks[:, :, hs * vs + c - 1] * qs[c]).reshape(-1, 64)).reshape(my, mx, 8, 8)
        planes.append(p.transpose(0, 2, 1, 3).reshape(my * 8, mx * 8))
    return planes, (hs, vs)


def decode(data: bytes, mutant=None) -> np.ndarray:
    m = read_markers(data)
    m["data"] = data
    planes, (hs, vs) = planes_of(m, entropy_decode(m, mutant))
    H, W = m["H"], m["W"]
    if len(planes) == 1:
        return planes[0][:H, :W].copy()
    chroma = []
    for p in planes[1:]:
        if mutant != "crop_after_upsampling":
            p = p[:-(-H // vs), :-(-W // hs)]
        if (hs, vs) == (2, 1):
            p = upsample_h2v1(p, mutant)
        elif (hs, vs) == (2, 2):
            p = upsample_h2v2(p, mutant)
        chroma.append(p[:H, :W])
    return ycc_to_rgb(planes[0][:H, :W], chroma[0], chroma[1], mutant)


# ---- writing -----------------------------------------------------------------------------------------------------------------------
def _size(v: int) -> int:
    return int(abs(int(v))).bit_length()


class Scan:
    """The entropy writer: blocks of quantised coefficients in ZIGZAG order, in stream order, become the stuffed segment.  `stats`
    counts, relative to the borders of the SUBSEQ-byte subsequences, what the tests plant."""

    def __init__(self, tables=None, stats: Stats = None):
        self.tables = {k: {s: format(code, f"0{size}b") for s, (code, size) in huffman_codes(*t).items()} for k, t in (tables or STD_TABLES).items()}
        self.stats = Stats() if stats is None else stats
        self.out = bytearray()
        self.acc, self.nacc = 0, 0
        self.pred = [0, 0, 0]
        self.restarts = 0

    def position(self) -> int:
        """The next bit's position in the stuffed stream."""
        return 8 * len(self.out) + self.nacc

    def _put(self, bits: str, what: str):
        first = self.position()
        for ch in bits:
            self.acc = (self.acc << 1) | (ch == "1")
            self.nacc += 1
            if self.nacc == 8:
                self.out.append(self.acc)
                if self.acc == 0xFF:
                    if len(self.out) % SUBSEQ == 0:
                        self.stats["ff00_across_border"] += 1
                    self.out.append(0)
                self.acc = self.nacc = 0
        last = self.position()
        border = (first // (8 * SUBSEQ) + 1) * 8 * SUBSEQ
        if first < border < last:
            self.stats[what + "_across_border"] += 1

    def block(self, zz, comp: int, td: int, ta: int):
        start = self.position()
        dc, ac = self.tables[(0, td)], self.tables[(1, ta)]
        diff = int(zz[0]) - self.pred[comp]
        self.pred[comp] = int(zz[0])
        s = _size(diff)
        if s == 11:
            self.stats["dc_size_11"] += 1
        self._put(dc[s], "code")
        if s:
            self._put(format(diff if diff >= 0 else diff + (1 << s) - 1, f"0{s}b"), "value")
        run = 0
        nonzero = [k for k in range(1, 64) if zz[k]]
        for k in range(1, 64):
            v = int(zz[k])
            if v == 0:
                run += 1
                continue
            while run > 15:
                self._put(ac[0xF0], "code")
                run -= 16
            s = _size(v)
            code = ac[(run << 4) | s]
            if len(code) == 16:
                self.stats["code_16_bits"] += 1
            self._put(code, "code")
            self._put(format(v if v >= 0 else v + (1 << s) - 1, f"0{s}b"), "value")
            run = 0
        if run:
            self._put(ac[0x00], "code")
        if nonzero == [63]:
            self.stats["only_zigzag_63"] += 1
        end = self.position()
        if end % (8 * SUBSEQ) == 0:
            self.stats["block_ends_on_border"] += 1
        if (end - 1) // (8 * SUBSEQ) - start // (8 * SUBSEQ) >= 2:
            self.stats["block_over_two_subsequences"] += 1

    def _flush(self):
        if self.nacc:
            self._put("1" * (8 - self.nacc), "pad")

    def restart(self):
        self._flush()
        if len(self.out) % SUBSEQ == 0:
            self.stats["restart_at_border"] += 1
        if self.restarts and self.restarts % 8 == 7:
            self.stats["restart_index_wraps"] += 1
        self.out += bytes([0xFF, 0xD0 + self.restarts % 8])
        self.restarts += 1
        self.pred = [0, 0, 0]

    def finish(self) -> bytes:
        self._flush()
        return bytes(self.out)


def _dht(tables) -> bytes:
    out = b""
    for (tc, th), (bits, vals) in sorted(tables.items()):
        out += b"\xff\xc4" + (19 + len(vals)).to_bytes(2, "big") + bytes([(tc << 4) | th]) + bytes(bits) + bytes(vals)
    return out


def write_file(H: int, W: int, blocks, sampling=None, quant=None, tables=None, ri: int = 0, stats: Stats = None, jfif: bool = True) -> bytes:
    """A complete baseline file around the writer's segment.  blocks: (MCUs * blocks per MCU, 64) quantised coefficients in ZIGZAG
    order, stream order.  sampling None: one component; else "4:4:4" / "4:2:2" / "4:2:0".  quant: one 64-entry table in zigzag
    order per table id 0 / 1 (default: all ones).  Table ids: Y 0, chroma 1."""
    tables = tables or STD_TABLES
    ncomp = 1 if sampling is None else 3
    hs, vs = (1, 1) if sampling is None else SAMPLINGS[sampling]
    per_mcu = [0] * (hs * vs) + ([1, 2] if ncomp == 3 else [])
    mcus = -(-W // (8 * hs)) * -(-H // (8 * vs))
    blocks = np.asarray(blocks).reshape(-1, 64)
    assert len(blocks) == mcus * len(per_mcu), (len(blocks), mcus, len(per_mcu))
    quant = quant or [[1] * 64, [1] * 64]
    scan = Scan(tables, stats)
    b = 0
    for mcu in range(mcus):
        if ri and mcu and mcu % ri == 0:
            scan.restart()
        for comp in per_mcu:
            t = 0 if comp == 0 else 1
            scan.block(blocks[b], comp, t, t)
            b += 1
    seg = scan.finish()
    out = b"\xff\xd8" + (b"\xff\xe0\x00\x10JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00" if jfif else b"")
    for t in range(2 if ncomp == 3 else 1):
        out += b"\xff\xdb\x00\x43" + bytes([t]) + bytes(int(x) for x in quant[t])
    out += b"\xff\xc0" + (8 + 3 * ncomp).to_bytes(2, "big") + b"\x08" + H.to_bytes(2, "big") + W.to_bytes(2, "big") + bytes([ncomp])
    out += bytes([1, (hs << 4) | vs, 0]) + (bytes([2, 0x11, 1, 3, 0x11, 1]) if ncomp == 3 else b"")
    out += _dht({k: v for k, v in tables.items() if ncomp == 3 or k[1] == 0})
    if ri:
        out += b"\xff\xdd\x00\x04" + ri.to_bytes(2, "big")
    out += b"\xff\xda" + (6 + 2 * ncomp).to_bytes(2, "big") + bytes([ncomp]) + bytes([1, 0x00]) + (bytes([2, 0x11, 3, 0x11]) if ncomp == 3 else b"")
    out += b"\x00\x3f\x00" + seg + b"\xff\xd9"
    return out


def segment_bytes(data: bytes) -> int:
    m = read_markers(data)
    return m["end"] - m["start"]


# ---- inputs ------------------------------------------------------------------------------------------------------------------------
def image(H: int, W: int, channels: int, kind: str, seed: int = 0) -> np.ndarray:
    rng = np.random.default_rng(seed + 1000 * H + W)
    if kind == "noise":
        img = rng.integers(0, 256, size=(H, W, channels), dtype=np.uint8)
    else:
        yy, xx = np.mgrid[0:H, 0:W]
        img = np.stack([(xx * 255 // max(W - 1, 1)), (yy * 255 // max(H - 1, 1)), ((xx + yy) * 37 % 256)][:channels], axis=2).astype(np.uint8)
    return img[:, :, 0] if channels == 1 else img


def pillow_file(img: np.ndarray, quality: int, sampling: str = "4:2:0", restart_blocks: int = 0, optimize: bool = False,
                progressive: bool = False) -> bytes:
    from PIL import Image
    buf = io.BytesIO()
    kw = {"subsampling": sampling} if img.ndim == 3 else {}
    if restart_blocks:
        kw["restart_marker_blocks"] = restart_blocks
    Image.fromarray(img).save(buf, format="JPEG", quality=quality, optimize=optimize, progressive=progressive, **kw)
    return buf.getvalue()


def pillow_pixels(data: bytes) -> np.ndarray:
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)))


pillow_has_jpeg = jpeg_refs.pillow_has_jpeg


# ---- planted streams ---------------------------------------------------------------------------------------------------------------
def random_blocks(rng, n: int, density: float = 0.25, amplitude: int = 6) -> np.ndarray:
    """n blocks in zigzag order: small values at `density` of the places, a slowly moving DC."""
    blocks = rng.integers(-amplitude, amplitude + 1, size=(n, 64)) * (rng.random((n, 64)) < density)
    blocks[:, 0] = np.cumsum(rng.integers(-8, 9, size=n))
    return blocks


def search(make, wanted, tries: int = 4000):
    """The first k for which make(k) -> (data, stats) shows every counter of `wanted`; the planted files are found, not hoped for."""
    for k in range(tries):
        data, stats = make(k)
        if all(stats[w] for w in wanted):
            decode(data)                              # inside the rule's int32 range
            return data, stats
    raise AssertionError(f"no stream with {wanted} in {tries} tries")


def _one_component(blocks, **kw):
    stats = Stats()
    return write_file(8, 8 * len(blocks), blocks, None, stats=stats, **kw), stats


@functools.lru_cache(maxsize=None)
def planted() -> dict:
    """name -> (file, stats): the streams the GPU tests plant, each with the counter that proves the situation occurred."""
    out = {}

    def ff00(k):
        rng = np.random.default_rng(k)
        blocks = random_blocks(rng, 9)
        blocks[6:, 1:3] = 1023                        # 0/A is a 16-bit code of nine ones, 1023 is ten ones
        return _one_component(blocks)
    out["ff00_across_border"] = search(ff00, ["ff00_across_border", "code_16_bits"])

    def straddle(k):
        return _one_component(random_blocks(np.random.default_rng(100 + k), 24))
    out["symbols_across_borders"] = search(straddle, ["code_across_border", "value_across_border"])
    out["block_ends_on_border"] = search(lambda k: _one_component(random_blocks(np.random.default_rng(200 + k), 12)), ["block_ends_on_border"])

    def long_block(k):
        rng = np.random.default_rng(300 + k)
        blocks = random_blocks(rng, 8)
        blocks[5, 1:] = rng.choice([-1, 1], size=63) * rng.integers(512, 1024, size=63)
        try:
            data, stats = _one_component(blocks)
            decode(data)
        except AssertionError:                        # this one leaves int32
            return b"", Stats()
        return data, stats
    out["block_over_two_subsequences"] = search(long_block, ["block_over_two_subsequences", "code_16_bits"])

    blocks = random_blocks(np.random.default_rng(5), 6)
    blocks[2, 1:] = 0
    blocks[2, 63] = 5
    blocks[3:, 0] += 1100
    blocks[4:, 0] -= 2000                             # a DC difference of -2000: size 11
    out["zigzag_63_and_dc_size_11"] = _one_component(blocks)
    assert out["zigzag_63_and_dc_size_11"][1]["only_zigzag_63"] and out["zigzag_63_and_dc_size_11"][1]["dc_size_11"]

    out["restart_at_border"] = search(lambda k: _one_component(random_blocks(np.random.default_rng(400 + k), 30, 0.5, 40), ri=3),
                                      ["restart_at_border"])
    out["restart_every_mcu"] = _one_component(random_blocks(np.random.default_rng(6), 20), ri=1)
    assert out["restart_every_mcu"][1]["restart_index_wraps"] == 2
    stats = Stats()
    rows = random_blocks(np.random.default_rng(7), 2 * 10 * 6, 0.3, 20)
    out["restart_every_mcu_row"] = (write_file(160, 32, rows, "4:2:0", ri=2, stats=stats), stats)
    assert stats["restart_index_wraps"] == 1
    for sampling in ("4:4:4", "4:2:2"):
        stats = Stats()
        hs, vs = SAMPLINGS[sampling]
        n = -(-50 // (8 * hs)) * -(-21 // (8 * vs)) * (hs * vs + 2)
        out["three_components_" + sampling] = (write_file(21, 50, random_blocks(np.random.default_rng(8), n, 0.3, 20), sampling, ri=4,
                                                          stats=stats), stats)
    return out


@functools.lru_cache(maxsize=None)
def segment_of_length(target: int) -> bytes:
    """A one-component file whose entropy-coded segment has exactly `target` bytes."""
    if target == 1:
        data = write_file(8, 8, np.zeros((1, 64), dtype=np.int64))
        assert segment_bytes(data) == 1
        return data
    def length(blocks):
        data = write_file(8, 8 * len(blocks), np.array(blocks))
        return segment_bytes(data), data

    for k in range(50):
        rng = np.random.default_rng(500 + 64 * target + k)
        blocks, tune = [], np.zeros(64, dtype=np.int64)
        while True:                                   # random blocks up to a little below the target ...
            more = random_blocks(rng, 1, 0.15, 30)[0]
            if length(blocks + [more, tune])[0] >= target:
                break
            blocks.append(more)
            tune[0] = more[0]
        for m in range(64):                           # ... then a block that grows by three bits a step
            tune[1:1 + m] = 1
            got, data = length(blocks + [tune])
            if got >= target:
                break
        if got == target:
            return data
    raise AssertionError(f"no segment of {target} bytes")

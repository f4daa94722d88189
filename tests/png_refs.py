"""A numpy restatement of the PNG stream of include/png/scg_png.h for the tests.  Own code, no kernel: the filter, the run tokens
(vectorised over a chunk's positions), the length-limited Huffman code, the block's bits, the zlib stream and the file.

    filtered_stream(img, filter, gray_as_rgb)   the S bytes that the deflate blocks carry
    chunk_tokens(d)                             (symbols, extra bit counts, extra values) of a chunk's tokens, in stream order
    code_lengths(freq)                          (lengths[286], the deepest leaf of the unlimited tree)
    encode_chunk(d, final)                      (the block's bytes, a dict of what the tests look at)
    zlib_stream(img, ...) / png_file(img, ...)  the whole stream / file; `chunks` receives the dicts
"""
import struct
import zlib

import numpy as np

CHUNK = 32768
NONE, SUB, UP, PAETH = 0, 1, 2, 4
FILTERS = (NONE, SUB, UP, PAETH)
HEADER_BITS = 1226
CLC_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
# RFC 1951 3.2.5: the first length and the extra bits of the symbols 257 .. 285
LEN_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LEN_EXTRA = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
_LEN_SYM = np.zeros(259, dtype=np.int64)
for _k, (_b, _e) in enumerate(zip(LEN_BASE, LEN_EXTRA)):
    _LEN_SYM[_b:min(_b + (1 << _e), 259)] = 257 + _k
_LEN_SYM[258] = 285
_BASE = np.array(LEN_BASE)
_EXTRA = np.array(LEN_EXTRA)


def as_hwc(img):
    a = np.ascontiguousarray(img, dtype=np.uint8)
    if a.ndim == 2:
        a = a[:, :, None]
    assert a.ndim == 3 and a.shape[2] in (1, 3)
    return a


def stream_geometry(H, W, C, gray_as_rgb):
    """(bpp, S, chunks, colour type)."""
    bpp = 3 if (C == 3 or gray_as_rgb) else 1
    S = H * (1 + W * bpp)
    return bpp, S, -(-S // CHUNK), 2 if bpp == 3 else 0


def filtered_stream(img, filt=UP, gray_as_rgb=True):
    a = as_hwc(img)
    H, W, C = a.shape
    bpp = stream_geometry(H, W, C, gray_as_rgb)[0]
    if C == 1 and bpp == 3:
        a = np.repeat(a, 3, axis=2)
    x = a.reshape(H, W * bpp).astype(np.int32)
    left, up, ul = np.zeros_like(x), np.zeros_like(x), np.zeros_like(x)
    left[:, bpp:] = x[:, :-bpp]
    up[1:] = x[:-1]
    ul[1:, bpp:] = x[:-1, :-bpp]
    if filt == NONE:
        pred = 0
    elif filt == SUB:
        pred = left
    elif filt == UP:
        pred = up
    elif filt == PAETH:
        p = left + up - ul
        pa, pb, pc = np.abs(p - left), np.abs(p - up), np.abs(p - ul)
        pred = np.where((pa <= pb) & (pa <= pc), left, np.where(pb <= pc, up, ul))
    else:
        raise ValueError(filt)
    out = np.empty((H, 1 + W * bpp), dtype=np.uint8)
    out[:, 0] = filt
    out[:, 1:] = ((x - pred) & 255).astype(np.uint8)
    return out.reshape(-1)


def chunk_tokens(d):
    """The tokens of one chunk: per token its symbol (a literal's byte, or a length's symbol), the number of its extra bits and their
    value, and whether it is a match (then one distance bit follows).  Every position decides its role from its run alone."""
    d = np.asarray(d, dtype=np.uint8)
    n = d.size
    starts = np.flatnonzero(np.r_[True, d[1:] != d[:-1]])
    lens = np.diff(np.r_[starts, n])
    rid = np.repeat(np.arange(starts.size), lens)
    j = np.arange(n) - starts[rid]
    L = lens[rid]
    m = L - 1
    jj = j - 1
    q, i = jj // 258, jj % 258
    full, r = m // 258, m % 258
    long_run = L >= 4
    match258 = long_run & (j > 0) & (q < full) & (i == 0)
    in_rest = long_run & (j > 0) & (q == full)
    match_r = in_rest & (r >= 3) & (i == 0)
    literal = ~long_run | (j == 0) | (in_rest & (r < 3))
    is_match = match258 | match_r
    keep = literal | is_match
    mlen = np.where(match258, 258, r)[keep]
    is_match = is_match[keep]
    sym = np.where(is_match, _LEN_SYM[np.where(is_match, mlen, 3)], d[keep].astype(np.int64))
    k = np.where(is_match, sym - 257, 0)
    ebits = np.where(is_match, _EXTRA[k], 0)
    evals = np.where(is_match, mlen - _BASE[k], 0)
    return sym, ebits, evals, is_match


def code_lengths(freq, limit=15):
    """Steps 1 to 5 of the header's rule.  Returns (lengths, deepest leaf of the unlimited tree)."""
    freq = [int(f) for f in freq]
    order = sorted((f, s) for s, f in enumerate(freq) if f)            # 1. by (frequency, symbol)
    n = len(order)
    assert n >= 2
    weight = [f for f, _ in order]                                       # 2. leaves 0 .. n-1, merged nodes behind them
    parent = [0] * (2 * n - 1)
    li, ni = 0, n
    for _ in range(n - 1):
        pick = []
        for _q in range(2):
            if li < n and (ni >= len(weight) or weight[li] <= weight[ni]):      # the leaf on a tie
                pick.append(li)
                li += 1
            else:
                pick.append(ni)
                ni += 1
        for p in pick:
            parent[p] = len(weight)
        weight.append(weight[pick[0]] + weight[pick[1]])
    depth = [0] * (2 * n - 1)
    for k in range(2 * n - 3, -1, -1):
        depth[k] = depth[parent[k]] + 1
    count = [0] * (limit + 1)                                            # 3. and 4.
    for k in range(n):
        count[min(depth[k], limit)] += 1
    total = sum(count[l] << (limit - l) for l in range(1, limit + 1))
    while total != 1 << limit:
        count[limit] -= 1
        for l in range(limit - 1, 0, -1):
            if count[l]:
                count[l] -= 1
                count[l + 1] += 2
                break
        total -= 1
    lengths = [0] * len(freq)                                            # 5. the most frequent first
    at = n
    for l in range(1, limit + 1):
        for _ in range(count[l]):
            at -= 1
            lengths[order[at][1]] = l
    assert at == 0
    return lengths, max(depth[:n])


def canonical_codes(lengths):
    """RFC 1951 3.2.2."""
    lengths = list(lengths)
    bl = [0] * 17
    for l in lengths:
        bl[l] += 1
    bl[0] = 0
    nxt, code = [0] * 17, 0
    for bits in range(1, 16):
        code = (code + bl[bits - 1]) << 1
        nxt[bits] = code
    codes = [0] * len(lengths)
    for s, l in enumerate(lengths):
        if l:
            codes[s] = nxt[l]
            nxt[l] += 1
    return codes


def _reverse(code, bits):
    return int(format(code, f"0{bits}b")[::-1], 2) if bits else 0


def _pack(values, nbits):
    """Values of nbits each, the first bit of each its lowest, into a little-endian bit array."""
    values, nbits = np.asarray(values, dtype=np.int64), np.asarray(nbits, dtype=np.int64)
    width = int(nbits.max()) if nbits.size else 0
    k = np.arange(width)
    bits = ((values[:, None] >> k[None, :]) & 1).astype(np.uint8)
    return bits[k[None, :] < nbits[:, None]]


def encode_chunk(d, final):
    d = np.asarray(d, dtype=np.uint8)
    n = d.size
    sym, ebits, evals, is_match = chunk_tokens(d)
    freq = np.bincount(sym, minlength=286)
    freq[256] += 1
    lengths, deepest = code_lengths(freq)
    codes = canonical_codes(lengths)
    rev = np.array([_reverse(c, l) for c, l in zip(codes, lengths)], dtype=np.int64)
    lens = np.array(lengths, dtype=np.int64)
    # BFINAL, BTYPE, HLIT, HDIST, HCLEN; the code-length code (CLC_ORDER: 16, 17, 18 unused, 0 .. 15 of 4 bits, so a length L has
    # the code L); the 286 lengths and the two distance codes of length 1
    head_v = [1 if final else 0, 2, 29, 1, 15] + [0 if s >= 16 else 4 for s in CLC_ORDER] + [_reverse(l, 4) for l in lengths + [1, 1]]
    head_n = [1, 2, 5, 5, 4] + [3] * 19 + [4] * 288
    tok_v = rev[sym] | (evals << lens[sym])                               # code, extra bits, then the distance bit 0
    tok_n = lens[sym] + ebits + is_match
    bits = np.concatenate([_pack(head_v, head_n), _pack(tok_v, tok_n), _pack([rev[256]], [lens[256]])])
    assert _pack(head_v, head_n).size == HEADER_BITS
    if final:
        body = np.packbits(bits, bitorder="little").tobytes()
    else:
        bits = np.concatenate([bits, np.zeros(3, dtype=np.uint8)])
        body = np.packbits(bits, bitorder="little").tobytes() + b"\x00\x00\xff\xff"
    info = {"n": n, "freq": freq, "lengths": lengths, "deepest": deepest, "tokens": int(sym.size), "matches": int(is_match.sum()),
            "dynamic_bytes": len(body)}
    if len(body) >= n + 5:
        info["kind"] = "stored"
        body = bytes([1 if final else 0]) + struct.pack("<HH", n & 0xFFFF, ~n & 0xFFFF) + d.tobytes()
    else:
        info["kind"] = "dynamic"
    info["bytes"] = len(body)
    return body, info


def adler32_from_chunks(parts):
    """The Adler-32 of a stream from (n, sum d[i], sum (n - i) d[i]) per chunk, exact integers modulo 65521."""
    a, b = 1, 0
    for n, sa, sb in parts:
        b = (b + n * a + sb) % 65521
        a = (a + sa) % 65521
    return (b << 16) | a


def zlib_stream(img, filt=UP, gray_as_rgb=True, chunks=None):
    s = filtered_stream(img, filt, gray_as_rgb)
    out, parts = [b"\x78\x01"], []
    count = -(-s.size // CHUNK)
    for c in range(count):
        d = s[c * CHUNK:(c + 1) * CHUNK]
        body, info = encode_chunk(d, c == count - 1)
        out.append(body)
        w = np.arange(d.size, 0, -1, dtype=np.int64)
        parts.append((d.size, int(d.sum(dtype=np.int64)), int((w * d).sum())))
        if chunks is not None:
            chunks.append(info)
    out.append(struct.pack(">I", adler32_from_chunks(parts)))
    return b"".join(out)


def _png_chunk(kind, data):
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data))


def png_file(img, filt=UP, gray_as_rgb=True, chunks=None):
    a = as_hwc(img)
    H, W, C = a.shape
    ctype = stream_geometry(H, W, C, gray_as_rgb)[3]
    return (b"\x89PNG\r\n\x1a\n" + _png_chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, ctype, 0, 0, 0)) +
            _png_chunk(b"IDAT", zlib_stream(a, filt, gray_as_rgb, chunks)) + _png_chunk(b"IEND", b""))


def idat_of(file_bytes):
    """The data of the file's one IDAT chunk; asserts the file's shape: signature, IHDR, ONE IDAT, IEND, every CRC right."""
    assert file_bytes[:8] == b"\x89PNG\r\n\x1a\n"
    at, kinds, idat = 8, [], None
    while at < len(file_bytes):
        n, = struct.unpack(">I", file_bytes[at:at + 4])
        kind, data = file_bytes[at + 4:at + 8], file_bytes[at + 8:at + 8 + n]
        assert struct.unpack(">I", file_bytes[at + 8 + n:at + 12 + n])[0] == zlib.crc32(kind + data)
        kinds.append(kind)
        if kind == b"IDAT":
            idat = data
        at += 12 + n
    assert kinds == [b"IHDR", b"IDAT", b"IEND"] and at == len(file_bytes)
    return idat


# ---- images the tests plant ------------------------------------------------------------------------------------------------------
def image_of_stream(d):
    """The one-channel 1 x W image whose filtered stream under filter None (gray_as_rgb off) is d: d[0] is the filter byte 0."""
    d = np.asarray(d, dtype=np.uint8)
    assert d[0] == 0 and d.size >= 2
    return np.ascontiguousarray(d[1:].reshape(1, -1))


def runs_stream(lengths, first=0):
    """A stream of runs of the given lengths; neighbouring runs differ, the first has the value `first` (0: it holds the filter byte)."""
    vals = (first + np.arange(len(lengths)) * 7) % 251
    vals[1:] = np.where(vals[1:] == vals[:-1], vals[1:] + 1, vals[1:])
    return np.repeat(vals.astype(np.uint8), lengths)


def _spread(counts):
    """A stream in which value v occurs counts[v] times (falling with v) and no two neighbours are equal; its first byte is 0."""
    n = sum(counts)
    order = np.repeat(np.arange(len(counts)), counts)
    d = np.empty(n, dtype=np.uint8)
    half = (n + 1) // 2
    d[0::2] = order[:half]                                    # the classic spread: no value holds more than half of the places
    d[1::2] = order[half:]
    assert d[0] == 0 and (d[1:] != d[:-1]).all()
    return d


def fibonacci_stream():
    """21 literal values with the counts 1, 1, 2, 3, ... 10946 and no equal neighbours: 28 656 bytes, the first of them 0.  With
    end-of-block's 1 every step of the merge meets a tie; the rule's "leaf on a tie" then grows two interleaved chains and the
    unlimited tree is 11 deep, not 21: this chunk does not reach the length limit (lucas_stream does)."""
    counts = [1, 1]
    while len(counts) < 21:
        counts.append(counts[-1] + counts[-2])
    assert sum(counts) == 28656
    return _spread(counts[::-1])


def lucas_stream():
    """19 literal values with the counts 1, then the Lucas numbers 1, 3, 4, 7, 11, ... 5778, no equal neighbours: 15 125 bytes.  With
    end-of-block's 1 every leaf but the first three is one more than the sum of all before it, so no step of the merge meets a tie,
    the tree is one chain and its deepest leaf lies at 19: the length limit and miniz's repair act."""
    counts = [1, 1, 3]
    while len(counts) < 19:
        counts.append(counts[-1] + counts[-2])
    assert counts[-1] == 5778 and sum(counts) == 15125
    return _spread(counts[::-1])


def decode_with_pillow(file_bytes):
    import io

    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(file_bytes)))


def expected_pixels(img, gray_as_rgb):
    """What a decoder must give back for the source image."""
    a = as_hwc(img)
    if a.shape[2] == 3:
        return a
    return np.repeat(a, 3, axis=2) if gray_as_rgb else a[:, :, 0]

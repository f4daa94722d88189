"""Frames of the test's own making for the binning stage ALONE (csrc/binning_tiles.hip, csrc/binning.hip, csrc/tile_sort.h) and
the exact reference of its output.

A frame is what scg_binning reads (include/scg_raster.h): the image size, `rects` (P, 2) uint32 = {min_x | min_y << 16,
width | height << 16} in tiles, `depth_keys` (P,) uint32 (a culled Gaussian: rect (0, 0), key 0xFFFFFFFF) and, optionally, a
bound that stands in for num_rendered.  No geometry, no blend: a list has exactly the length, the ties and the ids at which the
kernels branch.  Live keys stay inside the stage's contract: bit patterns of finite floats above 0.2.

The reference is plain numpy: every rectangle expanded into (tile, key, id), one sort on that triple, the ranges [start, end) per
tile ((0, 0) for an empty tile), and with a bound B < R every range clipped to [min(start, B), min(end, B)).  The output of the
stage is integers: `compare` knows no tolerance, and it leaves no tile and no list entry out.

check_frame asserts what keeps the kernels in bounds (every rectangle inside the tile grid, every culled Gaussian empty); every
runner calls it before anything is launched.  The runners import torch and the package inside themselves.
"""
from __future__ import annotations

import functools

import numpy as np

import blend_refs as B

TILE = 16
CULLED = 0xFFFFFFFF
KEY_LO, KEY_HI = 0x3E4CCCCE, 0x7F7FFFFF                 # the smallest float above 0.2f, FLT_MAX
GUARD, PATTERN = 64, 0xA5C3E17B                         # guard words behind every output, and what they (and the outputs) start as
PATTERN64 = (PATTERN << 32) | PATTERN
AUTO, GLOBAL_SORT = 0, 1
# the constants of the kernels that the frames are planted around (asserted against nothing: a changed constant moves an edge
# away from a planted length, it cannot make a test pass that should fail)
BUCKET_MAX, LONG_BUCKET_MAX, DENSE_MEAN, COOP, TILE_PATH_MAX_TILES, LARGE_FRAME, LARGE_SCENE = 24, 1024, 1100, 48, 38400, 1 << 20, 100000
LENGTHS = (0, 1, 2, 3, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 1535, 1536, 1537, 2047, 2048, 2049, 3583, 3584, 3585,
           4095, 4096, 4097, 8191, 8192, 8193, 16383, 16384, 16385, 20000)


def bits(x) -> int:
    return int(np.float32(x).view(np.uint32))


class Frame:
    def __init__(self, name, W, H, rects, keys, bound=None, **tags):
        self.name, self.W, self.H = name, int(W), int(H)
        self.gx, self.gy = (self.W + TILE - 1) // TILE, (self.H + TILE - 1) // TILE
        self.T = self.gx * self.gy
        self.rects = np.ascontiguousarray(rects, np.uint32).reshape(-1, 2)
        self.keys = np.ascontiguousarray(keys, np.uint32).reshape(-1)
        self.P = len(self.keys)
        self.bound = bound
        self.tags = tags
        check_frame(self)

    def with_bound(self, bound):
        return Frame(f"{self.name}@{bound}", self.W, self.H, self.rects, self.keys, int(bound), **self.tags)

    def unpacked(self):
        """x, y, w, h of every rectangle (int64)."""
        r = self.rects.astype(np.int64)
        return r[:, 0] & 0xFFFF, r[:, 0] >> 16, r[:, 1] & 0xFFFF, r[:, 1] >> 16


def check_frame(fr):
    """What keeps the kernels in bounds."""
    assert fr.P >= 1 and fr.rects.shape == (fr.P, 2) and fr.keys.shape == (fr.P,)
    assert 1 <= fr.gx < 65536 and 1 <= fr.gy < 65536
    x, y, w, h = fr.unpacked()
    live = (w * h) > 0
    assert ((w > 0) == (h > 0)).all(), "a rectangle is empty in both directions or in none"
    assert (x[live] + w[live] <= fr.gx).all() and (y[live] + h[live] <= fr.gy).all(), "every rectangle inside the tile grid"
    assert not fr.rects[~live].any() and (fr.keys[~live] == CULLED).all(), "a culled Gaussian: rect (0, 0), key 0xFFFFFFFF"
    assert ((fr.keys[live] >= KEY_LO) & (fr.keys[live] <= KEY_HI)).all(), "live keys: finite floats above 0.2"
    R = int((w * h).sum())
    assert 1 <= R < (1 << 22), R
    assert fr.bound is None or 1 <= fr.bound <= 4 * R + 1024


# ------------------------------------------------------------------------------------------------------------- the reference

def expand(fr):
    """(tile, key, id) of every instance, in id, row, column order (int64)."""
    x, y, w, h = fr.unpacked()
    cnt = w * h
    owner = np.repeat(np.arange(fr.P), cnt)
    local = np.arange(int(cnt.sum())) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    tile = (y[owner] + local // np.maximum(w[owner], 1)) * fr.gx + x[owner] + local % np.maximum(w[owner], 1)
    return tile, fr.keys.astype(np.int64)[owner], owner


def reference_of(fr, bound=None):
    """The stage's exact output.  `bound` (default: the frame's): what the caller passes as num_rendered."""
    bound = fr.bound if bound is None else bound
    tile, key, gid = expand(fr)
    o = np.lexsort((gid, key, tile))
    tile, key, gid = tile[o], key[o], gid[o]
    R = len(tile)
    lens = np.bincount(tile, minlength=fr.T).astype(np.int64)
    end = np.cumsum(lens)
    start = end - lens
    cap = R if bound is None else int(bound)
    lo, hi = np.minimum(start, cap), np.minimum(end, cap)
    ranges = np.where((hi > lo)[:, None], np.stack([lo, hi], 1), 0).astype(np.uint32)
    return dict(frame=fr, R=R, cap=cap, lens=lens, start=start, end=end, lo=lo, hi=hi, ranges=ranges,
                tile=tile, key=key, ids=gid.astype(np.uint32), keys_sorted=(tile.astype(np.uint64) << np.uint64(32)) | key.astype(np.uint64))


def ranges_words(T):
    per = (T + 7) // 8
    return 2 * T + 5 * 8 * per


def check_order_bands(words, T):
    """The two launch-order tables: blend_refs.check_order_tables (permutations + padding), and every tile / quadrant inside the
    band of ceil(T / 8) slots that holds its index."""
    B.check_order_tables(words, T)
    per = (T + 7) // 8
    tile_o = words[2 * T: 2 * T + 8 * per].astype(np.int64).reshape(8, per)
    quad_o = words[2 * T + 8 * per:].astype(np.int64).reshape(8, 4 * per)
    band = np.arange(8)[:, None]
    assert ((tile_o == T) | (tile_o // per == band)).all(), "a tile outside its band"
    assert ((quad_o == 4 * T) | (quad_o // (4 * per) == band)).all(), "a quadrant outside its band"


def compare(ref, point_list, words, keys_sorted=None, num_rendered_out=None):
    """The stage's buffers as the GPU left them — each GUARD words longer than the stage may write, filled with PATTERN before
    the call — against the reference.  point_list: cap + GUARD uint32; words: ranges_words(T) + GUARD uint32; keys_sorted
    (optional): cap + GUARD uint64; num_rendered_out (optional): the word the stage wrote."""
    fr, R, cap, T = ref["frame"], ref["R"], ref["cap"], ref["frame"].T
    nw = ranges_words(T)
    point_list, words = np.asarray(point_list, np.uint32), np.asarray(words, np.uint32)
    assert len(point_list) == cap + GUARD and len(words) == nw + GUARD
    assert (point_list[cap:] == PATTERN).all(), "a guard word behind point_list[bound] was written"
    assert (words[nw:] == PATTERN).all(), "a guard word behind the ranges words was written"
    got = words[:2 * T].reshape(T, 2)
    bad = np.nonzero((got != ref["ranges"]).any(1))[0]
    assert len(bad) == 0, f"ranges differ in {len(bad)} tiles, first {bad[0]}: {got[bad[0]]} != {ref['ranges'][bad[0]]}"
    n = min(R, cap)
    whole = np.repeat(ref["end"] <= cap, ref["lens"])[:n]                       # position belongs to a list that fits below the bound
    wrong = np.nonzero(whole & (point_list[:n] != ref["ids"][:n]))[0]
    assert len(wrong) == 0, (f"{len(wrong)} list entries differ, first at {wrong[0]} (tile {ref['tile'][wrong[0]]}): "
                             f"{point_list[wrong[0]]} != {ref['ids'][wrong[0]]}")
    for t in np.nonzero((ref["start"] < cap) & (ref["end"] > cap))[0]:           # the tile the bound cuts (at most one)
        lo, hi, s, e = int(ref["lo"][t]), int(ref["hi"][t]), int(ref["start"][t]), int(ref["end"][t])
        got_ids = point_list[lo:hi].astype(np.int64)
        assert np.isin(got_ids, ref["ids"][s:e]).all(), f"cut tile {t}: an entry that is not in its list"
        k = fr.keys[np.minimum(got_ids, fr.P - 1)].astype(np.int64)
        comp = (k << 32) | got_ids
        assert (comp[1:] > comp[:-1]).all(), f"cut tile {t}: not strictly increasing in (key, id)"
    if keys_sorted is not None:
        keys_sorted = np.asarray(keys_sorted, np.uint64)
        assert len(keys_sorted) == cap + GUARD
        assert (keys_sorted[cap:] == np.uint64(PATTERN64)).all(), "a guard word behind keys_sorted was written"
        if cap >= R:
            wrong = np.nonzero(keys_sorted[:R] != ref["keys_sorted"])[0]
            assert len(wrong) == 0, f"{len(wrong)} sorted keys differ, first at {wrong[0]}"
    if num_rendered_out is not None:
        assert int(num_rendered_out) == R, f"num_rendered_out {int(num_rendered_out)} != {R}"
    check_order_bands(words[:nw], T)


def perfect_output(ref, rng=None):
    """Buffers that `compare` accepts: the reference itself, the guards, identity order tables; in the tile the bound cuts a
    random subset of its list."""
    fr, cap, R, T = ref["frame"], ref["cap"], ref["R"], ref["frame"].T
    rng = rng or np.random.default_rng(0)
    pl = np.full(cap + GUARD, PATTERN, np.uint32)
    n = min(R, cap)
    pl[:n] = ref["ids"][:n]
    for t in np.nonzero((ref["start"] < cap) & (ref["end"] > cap))[0]:
        s, e, lo, hi = int(ref["start"][t]), int(ref["end"][t]), int(ref["lo"][t]), int(ref["hi"][t])
        pl[lo:hi] = ref["ids"][s:e][np.sort(rng.choice(e - s, hi - lo, replace=False))]
    per = (T + 7) // 8
    words = np.full(ranges_words(T) + GUARD, PATTERN, np.uint32)
    words[:2 * T] = ref["ranges"].reshape(-1)
    words[2 * T: 2 * T + 8 * per] = np.minimum(np.arange(8 * per), T)
    words[2 * T + 8 * per: 2 * T + 40 * per] = np.minimum(np.arange(32 * per), 4 * T)
    ks = np.full(cap + GUARD, PATTERN64, np.uint64)
    ks[:n] = ref["keys_sorted"][:n]
    return dict(point_list=pl, words=words, keys_sorted=ks, num_rendered_out=R)


# ------------------------------------------------------------------------------------------------------------ key patterns

def spread(n, lo=1.0, hi=100.0):
    """n distinct, evenly spaced bit patterns of floats in [lo, hi], ascending."""
    k = np.linspace(bits(lo), bits(hi), n).astype(np.uint64).astype(np.uint32) if n else np.zeros(0, np.uint32)
    assert len(np.unique(k)) == n
    return k


def _with_groups(n, groups):
    """Spread keys (at least 2 bit patterns apart) plus tie groups: groups = [(size, sorted position of its first member)]."""
    base = spread(n - sum(g for g, _ in groups))
    assert len(base) < 2 or int(np.diff(base.astype(np.int64)).min()) >= 2
    out, shift = [base], 0
    for size, at in groups:                                  # a value of its own just above base[at - shift - 1]
        i = at - shift
        assert 1 <= i <= len(base)
        out.append(np.full(size, base[i - 1] + 1, np.uint32))
        shift += size
    return np.concatenate(out)


KEY_PATTERNS = ("spread", "equal", "few", "bucket_ties", "long_ties", "outliers")


def pattern_keys(kind, n, rng, salt=0):
    """n keys of one list, in random order."""
    if n == 0:
        return np.zeros(0, np.uint32)
    if kind == "equal":
        k = np.full(n, bits(2.5) + 977 * salt, np.uint32)
    elif kind == "few":
        k = rng.choice(spread(37, 2.0, 50.0), n)
    elif kind == "long_ties" and n > 8192:
        # a tie group of exactly kLongBucketMax and one of kLongBucketMax + 1 entries, each straddling a multiple of 1 024 in
        # sorted order: [1536, 2560) and [6024, 7049)
        k = _with_groups(n, [(LONG_BUCKET_MAX, 1536), (LONG_BUCKET_MAX + 1, 6024)])
    elif kind in ("bucket_ties", "long_ties") and n >= 100:
        k = _with_groups(n, [(BUCKET_MAX, n // 3), (BUCKET_MAX + 1, (2 * n) // 3)])
    elif kind == "outliers" and n >= 3:                      # a narrow range beside one key near 0.2 and one near FLT_MAX
        k = np.concatenate([bits(5.0) + 3 * np.arange(n - 2, dtype=np.uint32), np.asarray([KEY_LO, KEY_HI], np.uint32)])
    else:
        k = spread(n)
    return rng.permutation(k.astype(np.uint32))


def tie_groups(keys):
    """Sizes of the groups of equal keys (descending)."""
    _, c = np.unique(keys, return_counts=True)
    return np.sort(c)[::-1]


# ------------------------------------------------------------------------------------------------------------------ planting

class Planter:
    """Collects live Gaussians (a rectangle and a key each) and culled ones; finish() deals the ids out at random, so that the
    order of the ids says nothing about tiles or depths."""

    def __init__(self, name, W, H, seed=0):
        self.name, self.W, self.H = name, W, H
        self.gx, self.gy = (W + TILE - 1) // TILE, (H + TILE - 1) // TILE
        self.rng = np.random.default_rng(seed)
        self.rows = []                                       # arrays (n, 5): x, y, w, h, key

    def rect(self, x, y, w, h, key):
        self.rows.append(np.asarray([[x, y, w, h, key]], np.int64))

    def fill(self, t, keys):
        """len(keys) Gaussians on tile t alone."""
        n = len(keys)
        a = np.empty((n, 5), np.int64)
        a[:, 0], a[:, 1], a[:, 2], a[:, 3], a[:, 4] = t % self.gx, t // self.gx, 1, 1, keys
        self.rows.append(a)

    def finish(self, culled=0, bound=None, **tags):
        live = np.concatenate(self.rows) if self.rows else np.zeros((0, 5), np.int64)
        P = len(live) + culled
        ids = self.rng.permutation(P)[:len(live)]
        rects, keys = np.zeros((P, 2), np.uint32), np.full(P, CULLED, np.uint32)
        rects[ids, 0] = live[:, 0] | (live[:, 1] << 16)
        rects[ids, 1] = live[:, 2] | (live[:, 3] << 16)
        keys[ids] = live[:, 4]
        return Frame(self.name, self.W, self.H, rects, keys, bound, **tags)


def _from_live(name, W, H, P, live, **tags):
    """live: {id: (x, y, w, h, key)}; every other id is culled."""
    rects, keys = np.zeros((P, 2), np.uint32), np.full(P, CULLED, np.uint32)
    for i, (x, y, w, h, k) in live.items():
        assert 0 <= i < P
        rects[i] = (x | (y << 16), w | (h << 16))
        keys[i] = k
    return Frame(name, W, H, rects, keys, **tags)


def length_frame(kind, dense):
    """Every length of LENGTHS in a tile of its own, keys of pattern `kind`.  sparse: 256 x 192 px, 192 tiles, R // tiles < 1 100;
    dense: 128 x 64 px, 32 tiles, R // tiles >= 1 100 — the host picks other kernels either side of kDenseMeanList."""
    W, H = (128, 64) if dense else (256, 192)
    p = Planter(f"lengths-{kind}-{'dense' if dense else 'sparse'}", W, H, seed=len(kind) + 100 * dense)
    T = p.gx * p.gy
    stride = T // len(LENGTHS)
    planted = {}
    for i, n in enumerate(LENGTHS):
        t = (i * stride + (3 if stride > 1 else 0)) % T
        planted[t] = n
        p.fill(t, pattern_keys(kind, n, p.rng, salt=i))
    return p.finish(culled=777, planted=planted, kind=kind, dense=dense)


def mean_edge_frame(R):
    """64 tiles, R = 64 x 1 100 or one less: R // tiles exactly at kDenseMeanList or one below."""
    p = Planter(f"mean-{R // 64}", 128, 128, seed=R)
    lens = [2047, 2048, 2049, 1535, 1536, 1537, 3583, 3584, 3585, 4095, 4096, 4097, 8191, 8192, 8193]
    lens.append(R - sum(lens))
    assert lens[-1] > 8192
    planted = {}
    for i, n in enumerate(lens):
        planted[4 * i + 1] = n
        p.fill(4 * i + 1, pattern_keys("bucket_ties" if i % 2 else "spread", n, p.rng, salt=i))
    return p.finish(culled=100, planted=planted)


def id_width_frame(P):
    """Almost everything culled; one tile holds a tie group of more than kBucketMax live entries with id P - 1 and the pairs of
    ids that differ only in the next byte up (255 / 256, 65 535 / 65 536) where P has them."""
    rng = np.random.default_rng(P)
    special = [i for i in (0, 1, 254, 255, 256, 257, 65534, 65535, 65536, P - 2, P - 1) if 0 <= i < P]
    ids = set(special) | set(int(i) for i in rng.choice(P, 50, replace=False))
    ids = sorted(ids)
    tied = set(special) | set(ids[::2]) | set(ids[:8])
    assert len(tied) > BUCKET_MAX + 4
    live = {}
    for i in ids:
        if i in tied:
            live[i] = (1, 1, 1, 1, bits(3.25))                   # one tile, one depth
        else:
            live[i] = (int(rng.integers(0, 3)), int(rng.integers(0, 2)), 2, 2, int(spread(64)[i % 64]))
    return _from_live(f"idwidth-{P}", 64, 48, P, live, tied=sorted(tied), tied_tile=1 * 4 + 1)


SLICE_PS = (1, 15, 16, 17, 127, 128, 129, 2047, 2048, 2049, 99999, 100000)


def slice_frame(P):
    """Live Gaussians at the very first and the very last ids (and a handful in the middle of a large P), long culled runs
    between them: whole slices of the 128 (P < 100 000) or 256 slices are empty."""
    rng = np.random.default_rng(P + 5)
    ids = sorted(set([0, P - 1] + [i for i in (1, 2, P - 3, P - 2, P // 2, P // 2 + 1) if 0 <= i < P and P > 16]))
    keys = spread(8, 1.5, 9.0)
    live = {i: (int(rng.integers(0, 3)), int(rng.integers(0, 3)), int(rng.integers(1, 3)), int(rng.integers(1, 3)), int(keys[j % 5]))
            for j, i in enumerate(ids)}
    return _from_live(f"slices-{P}", 64, 64, P, live, live_ids=ids)


def large_frame(R):
    """kLargeFrame: R = 2^20 or one less from a small P — full-image rectangles on a 64 x 64-tile grid."""
    p = Planter(f"large-{R}", 1024, 1024, seed=R)
    keys = p.rng.permutation(spread(300, 1.0, 30.0))
    full, rest = divmod(R, 4096)
    for j in range(full):
        p.rect(0, 0, 64, 64, keys[j])
    if rest:                                                 # 4 095 = 64 x 63 + 63 x 1
        assert rest == 4095
        p.rect(0, 1, 64, 63, keys[full])
        p.rect(1, 0, 63, 1, keys[full + 1])
    return p.finish(culled=300 - len(p.rows))


def grid_frame(gx, gy, seed=0, n_random=40, long_tiles=()):
    """Rectangles at the edges of a gx x gy-tile grid, wherever they fit: 1 x 1 at the four corners, the full image, 48 and 49
    tiles (6 x 8, 48 x 1, 7 x 7, 49 x 1 and transposed: either side of the cooperative walk), rectangles across every boundary of
    the 8 bands of tile rows (rows gy b / 8) and across three of them, widths 3, 7 and 240 (the reciprocal divide's fix-up needs
    more than 48 tiles: heights that make it so), random ones; a few entries on each tile of `long_tiles`."""
    p = Planter(f"grid-{gx}x{gy}", TILE * gx - 5, TILE * gy - 9, seed=seed + gx * 1000 + gy)     # (partial tiles on both edges)
    assert (p.gx, p.gy) == (gx, gy)
    rng = p.rng
    keys = spread(23, 0.75, 400.0)                           # few values: overlapping rectangles tie, the id decides
    nxt = iter(range(10 ** 9))
    key = lambda: int(keys[(7 * next(nxt)) % 23])
    shapes = []

    def put(w, h, x=None, y=None):
        if w > gx or h > gy or w < 1 or h < 1:
            return
        x = int(rng.integers(0, gx - w + 1)) if x is None else x
        y = int(rng.integers(0, gy - h + 1)) if y is None else y
        if x < 0 or y < 0 or x + w > gx or y + h > gy:
            return
        p.rect(x, y, w, h, key())
        shapes.append((x, y, w, h))

    for (x, y) in ((0, 0), (gx - 1, 0), (0, gy - 1), (gx - 1, gy - 1)):
        put(1, 1, x, y)
    put(gx, gy, 0, 0)
    put(gx, gy, 0, 0)                                        # twice: every list has a neighbour in depth
    for (w, h) in ((6, 8), (8, 6), (48, 1), (1, 48), (7, 7), (49, 1), (1, 49)):
        put(w, h)
        put(w, h, gx - w, gy - h)
    rows = sorted(set(gy * b // 8 for b in range(1, 8)) - {0})
    for r in rows:
        put(min(3, gx), 2, None, r - 1)
        put(1, 2, gx - 1, r - 1)
    if len(rows) >= 3:
        put(min(2, gx), rows[2] - rows[0] + 2, None, rows[0] - 1)
    for w in (3, 7, 240):
        for h in (COOP // w + 1, COOP // w + 2, min(gy, 3 * (COOP // w + 1))):
            put(w, h)
            put(w, h, gx - w, None)
    for _ in range(n_random):
        w, h = int(rng.integers(1, min(gx, 12) + 1)), int(rng.integers(1, min(gy, 12) + 1))
        put(w, h)
    for t in long_tiles:
        p.fill(t, pattern_keys("bucket_ties", 100, rng, salt=t))
    return p.finish(culled=50, shapes=shapes, long_tiles=tuple(long_tiles))


GRIDS = ((1, 1), (7, 1), (8, 1), (9, 1), (3, 3), (9, 7), (8, 8), (13, 5), (10, 2), (1, 10), (60, 51))
BIG_GRIDS = {"128x128": (128, 128, (255, 256, 2047, 2048 + 255, 2048 + 256, 2 * 2048 - 1, 7 * 2048 + 2047)),
             "129x128": (129, 128, (255, 256, 2048, 2063, 2064 + 255, 2064 + 256, 2064 + 2050, 7 * 2064 + 2063)),
             "240x160": (240, 160, (0, 4799, 4800, 4800 + 2050, 38399)),
             "241x160": (241, 160, (0, 4819, 4820, 38559))}


def bound_base_frame():
    """Mixed lengths with long lists, for the bounds: 48 tiles."""
    p = Planter("bounds", 128, 96, seed=11)
    planted = {0: 5, 2: 700, 5: 9000, 9: 1537, 17: 20000, 18: 1, 30: 3000, 47: 5000}
    for i, (t, n) in enumerate(planted.items()):
        p.fill(t, pattern_keys("bucket_ties" if i % 2 else "spread", n, p.rng, salt=i))
    return p.finish(culled=321, planted=planted)


def bounds_of(ref):
    """The bounds of the issue for the bound frame's exact reference: name -> bound."""
    R, start = ref["R"], ref["start"]
    return {"R+1": R + 1, "R": R, "R-1": R - 1, "4R": 4 * R, "1": 1, "tile_start": int(start[17]), "mid_long": int(start[17]) + 10000}


@functools.lru_cache(maxsize=None)
def frame(name):
    kind, _, arg = name.partition(":")
    if kind == "lengths":
        pat, dens = arg.split("/")
        return length_frame(pat, dens == "dense")
    if kind == "mean":
        return mean_edge_frame(int(arg))
    if kind == "idwidth":
        return id_width_frame(int(arg))
    if kind == "slices":
        return slice_frame(int(arg))
    if kind == "large":
        return large_frame(int(arg))
    if kind == "grid":
        if arg in BIG_GRIDS:
            gx, gy, lt = BIG_GRIDS[arg]
            return grid_frame(gx, gy, n_random=60, long_tiles=lt)
        gx, gy = map(int, arg.split("x"))
        return grid_frame(gx, gy)
    if kind == "bounds":
        return bound_base_frame()
    raise KeyError(name)


@functools.lru_cache(maxsize=8)
def reference(name, bound=None):
    fr = frame(name)
    return reference_of(fr if bound is None else fr.with_bound(bound))


LENGTH_FRAMES = tuple(f"lengths:{k}/{d}" for k in KEY_PATTERNS for d in ("sparse", "dense"))
MEAN_FRAMES = (f"mean:{64 * DENSE_MEAN - 1}", f"mean:{64 * DENSE_MEAN}")
IDWIDTH_FRAMES = tuple(f"idwidth:{P}" for P in (256, 257, 65536, 65537))
SLICE_FRAMES = tuple(f"slices:{P}" for P in SLICE_PS) + (f"large:{LARGE_FRAME - 1}", f"large:{LARGE_FRAME}")
GRID_FRAMES = tuple(f"grid:{gx}x{gy}" for gx, gy in GRIDS) + tuple(f"grid:{k}" for k in BIG_GRIDS)
HINT_FRAMES = ("lengths:bucket_ties/sparse", "grid:13x5", f"mean:{64 * DENSE_MEAN}")
ALL_FRAMES = LENGTH_FRAMES + MEAN_FRAMES + IDWIDTH_FRAMES + SLICE_FRAMES + GRID_FRAMES + ("bounds",)


def slice_count(P, R):
    return 256 if (R >= LARGE_FRAME or P >= LARGE_SCENE) else 128


def hint_fill(kind, n, edges, seed=0):
    """n hint words: zeros | ones (all bits) | random (half of them inside the classes' range, half anywhere) | edges (cycled)."""
    rng = np.random.default_rng(seed)
    if kind == "zeros":
        return np.zeros(n, np.uint32)
    if kind == "ones":
        return np.full(n, 0xFFFFFFFF, np.uint32)
    if kind == "random":
        a = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
        small = rng.random(n) < 0.5
        a[small] = rng.integers(0, 600, int(small.sum()))
        return a
    assert kind == "edges"
    return np.asarray(edges, np.uint32)[rng.integers(0, len(edges), n)]


HINT_FILLS = ("zeros", "ones", "random", "edges")
TILE_COST_EDGES, BWD_COST_EDGES = (31, 32, 512, 513), (15, 16, 256, 257)


def check_cost_order(words, T, cost, lens):
    """With a tile_cost_in hint: inside a band, consecutive real tiles whose cost is at least 32 satisfy c[i+1] <= 1.07 c[i] + 1
    (the rule of test_tile_cost_hint_reorders_the_launch_and_changes_no_result).  The kernel's classes are 16 per octave over
    32 .. 512 with everything above in the top class, and it never reads the hint of a tile whose list is empty (such a tile goes
    last whatever the hint says): the rule is stated over the tiles with a list and a hint inside the classes' range, up to
    544 = one class step above 512."""
    per = (T + 7) // 8
    order = words[2 * T: 2 * T + 8 * per].astype(np.int64).reshape(8, per)
    for b in range(8):
        t = order[b][order[b] < T]
        c = cost[t].astype(np.float64)
        c = c[(lens[t] > 0) & (c >= 32) & (c <= 544)]
        assert (c[1:] <= c[:-1] * 1.07 + 1).all(), f"band {b}: the launch order does not follow the cost classes"


# --------------------------------------------------------------------------------------------------- scg_binning, called directly

def _sync_or_exit(what):
    import torch
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:                             # a GPU fault: nothing more is started on the card by this session
        import pytest
        pytest.exit(f"GPU fault in {what}: {e}", returncode=3)


def run_binning(fr, algo=AUTO, keys=True, tile_cost_in=None, bwd_cost_in=None, scratch_byte=0x5A):
    """lib.scg_binning on the frame's buffers, pointers passed the way the binding passes them.  Every output starts as PATTERN
    and is GUARD words longer than the stage may write; every byte of the scratch starts as `scratch_byte` (the binding hands over
    whatever torch.empty gave it).  The frame's bound (if any) is passed as num_rendered and sizes point_list, keys_sorted and the
    scratch.  Returns numpy arrays + `accepts` (scg_binning_accepts_bound)."""
    import torch
    from scgaussian_amd import _lib
    from scgaussian_amd import rasterizer as R
    check_frame(fr)
    lib = _lib.load()
    dev = torch.device("cuda", torch.cuda.current_device())
    ref_R = int((fr.unpacked()[2] * fr.unpacked()[3]).sum())
    cap = ref_R if fr.bound is None else int(fr.bound)
    accepts = int(lib.scg_binning_accepts_bound(cap, fr.W, fr.H, algo))
    assert cap == ref_R or (algo == AUTO and accepts == 1), "only the tile-first path takes a bound"
    nw = int(lib.scg_ranges_words(fr.W, fr.H))
    assert nw == ranges_words(fr.T)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    pat32 = int(np.uint32(PATTERN).view(np.int32))
    rects, dkeys = up(fr.rects.view(np.int32)), up(fr.keys.view(np.int32))
    plist = torch.full((cap + GUARD,), pat32, dtype=torch.int32, device=dev)
    words = torch.full((nw + GUARD,), pat32, dtype=torch.int32, device=dev)
    ks = torch.full((cap + GUARD,), int(np.uint64(PATTERN64).view(np.int64)), dtype=torch.int64, device=dev) if keys else None
    nr = torch.full((1 + GUARD,), pat32, dtype=torch.int32, device=dev)
    sbytes = int(lib.scg_binning_scratch_bytes(fr.P, cap, fr.W, fr.H, algo))
    scratch = torch.full((sbytes + 256,), int(scratch_byte), dtype=torch.uint8, device=dev)
    tci = None if tile_cost_in is None else up(np.asarray(tile_cost_in, np.uint32).view(np.int32))
    bci = None if bwd_cost_in is None else up(np.asarray(bwd_cost_in, np.uint32).view(np.int32))
    assert tci is None or tci.numel() == fr.T
    assert bci is None or bci.numel() == 4 * fr.T
    st = R.GaussianRasterizationSettings(fr.H, fr.W, 1.0, 1.0, torch.zeros(3, device=dev), 1.0, torch.eye(4, device=dev),
                                         torch.eye(4, device=dev), 0, torch.zeros(3, device=dev), False, False)
    frame_ = R._frame_for(st, fr.P, 0, dev)
    c = frame_.c
    saved = (c.tile_cost_in, c.tile_cost_out, c.bwd_cost_in, c.bwd_cost_out, c.long_lists_out, c.num_rendered_out)
    try:
        c.tile_cost_out = c.bwd_cost_out = c.long_lists_out = None
        c.tile_cost_in, c.bwd_cost_in, c.num_rendered_out = R.ptr(tci), R.ptr(bci), R.ptr(nr)
        R.check(lib.scg_binning(frame_.ref, cap, R.ptr(rects), R.ptr(dkeys), R.ptr(plist), R.ptr(words), R.ptr(ks), algo,
                                R.ptr(scratch), sbytes, R._stream(dev)), "scg_binning")
        _sync_or_exit(f"scg_binning on frame {fr.name} (algo {algo})")
    finally:
        (c.tile_cost_in, c.tile_cost_out, c.bwd_cost_in, c.bwd_cost_out, c.long_lists_out, c.num_rendered_out) = saved
    nr_np = nr.cpu().numpy().view(np.uint32)
    assert (nr_np[1:] == PATTERN).all(), "a word behind num_rendered_out was written"
    return dict(point_list=plist.cpu().numpy().view(np.uint32), words=words.cpu().numpy().view(np.uint32),
                keys_sorted=None if ks is None else ks.cpu().numpy().view(np.uint64), num_rendered_out=int(nr_np[0]), accepts=accepts)


def run_empty(W, H, P, algo):
    """scg_binning with num_rendered = 0 (every Gaussian culled): the ranges words and num_rendered_out, guards included."""
    import torch
    from scgaussian_amd import _lib
    from scgaussian_amd import rasterizer as R
    lib = _lib.load()
    dev = torch.device("cuda", torch.cuda.current_device())
    nw = int(lib.scg_ranges_words(W, H))
    pat32 = int(np.uint32(PATTERN).view(np.int32))
    words = torch.full((nw + GUARD,), pat32, dtype=torch.int32, device=dev)
    nr = torch.full((1 + GUARD,), pat32, dtype=torch.int32, device=dev)
    rects = torch.zeros((P, 2), dtype=torch.int32, device=dev)
    dkeys = torch.full((P,), -1, dtype=torch.int32, device=dev)
    st = R.GaussianRasterizationSettings(H, W, 1.0, 1.0, torch.zeros(3, device=dev), 1.0, torch.eye(4, device=dev),
                                         torch.eye(4, device=dev), 0, torch.zeros(3, device=dev), False, False)
    frame_ = R._frame_for(st, P, 0, dev)
    c = frame_.c
    saved = (c.tile_cost_in, c.tile_cost_out, c.bwd_cost_in, c.bwd_cost_out, c.long_lists_out, c.num_rendered_out)
    try:
        c.tile_cost_in = c.tile_cost_out = c.bwd_cost_in = c.bwd_cost_out = c.long_lists_out = None
        c.num_rendered_out = R.ptr(nr)
        R.check(lib.scg_binning(frame_.ref, 0, R.ptr(rects), R.ptr(dkeys), None, R.ptr(words), None, algo, None, 0,
                                R._stream(dev)), "scg_binning")
        _sync_or_exit(f"scg_binning on an empty {W} x {H} frame")
    finally:
        (c.tile_cost_in, c.tile_cost_out, c.bwd_cost_in, c.bwd_cost_out, c.long_lists_out, c.num_rendered_out) = saved
    return words.cpu().numpy().view(np.uint32), nr.cpu().numpy().view(np.uint32)


def compare_run(ref, out):
    compare(ref, out["point_list"], out["words"], out["keys_sorted"], out["num_rendered_out"])


# ------------------------------------------------------------------------------------------- the same edges through scg_forward

FWD_W, FWD_H = 256, 192                                  # 192 tiles: a capacity of R is sparse, one of 192 x 1 100 dense
FWD_LENGTHS = (1535, 1536, 1537, 3583, 3584, 3585, 4095, 4096, 4097, 8191, 8192, 8193, 16383, 16384, 16385, 20000)
FWD_PATTERNS = ("spread", "equal", "ties")
SKIP_RARE_SORT, RARE_8WAVE, SPLIT_LONG_LISTS, DEBUG_SEPARATE_SORT, DEBUG_SEPARATE_HIST = 8, 16, 32, 1, 2
FWD_OPTIONS = (0, SKIP_RARE_SORT, RARE_8WAVE, RARE_8WAVE | SPLIT_LONG_LISTS, DEBUG_SEPARATE_SORT, DEBUG_SEPARATE_HIST)
NEAR_FAR = (0.3, 0.31, 0.32, 900.0, 950.0, 1000.0)       # beside the 20 000-entry list's depths of 1 .. 100


class Scene:
    """Tiny isotropic Gaussians at tile centres under synthetic.default_camera(FWD_W, FWD_H) (R = I, T = 0: view depth = z):
    means (P, 3) fp32, the tile and the planted key (float bits of z) of every Gaussian."""

    def __init__(self, name, means, tile, key):
        self.name, self.means, self.tile, self.key, self.P = name, means, tile, key, len(tile)
        self.gx, self.gy = FWD_W // TILE, FWD_H // TILE
        self.T = self.gx * self.gy
        self.lens = np.bincount(tile, minlength=self.T)


@functools.lru_cache(maxsize=None)
def forward_scene(kind):
    import math
    rng = np.random.default_rng(sum(map(ord, kind)))
    gx, gy = FWD_W // TILE, FWD_H // TILE
    tiles, keys = [], []
    for i, n in enumerate(FWD_LENGTHS):
        t = 11 * i + 7
        if kind == "spread" and n == 20000:              # three much nearer and three much farther entries: the split's key range
            k = np.concatenate([spread(n - 6), np.asarray([bits(z) for z in NEAR_FAR], np.uint32)])     # comes from 1 024 samples
            k = rng.permutation(k)
        else:
            k = pattern_keys({"spread": "spread", "equal": "equal", "ties": "long_ties"}[kind], n, rng, salt=i)
        tiles.append(np.full(n, t))
        keys.append(k)
    tile, key = np.concatenate(tiles), np.concatenate(keys).astype(np.uint32)
    o = rng.permutation(len(tile))
    tile, key = tile[o], key[o]
    z = key.view(np.float32).astype(np.float64)
    px, py = TILE * (tile % gx) + 7.5, TILE * (tile // gx) + 7.5
    tany = math.tan(math.radians(50.0) / 2)
    tanx = tany * FWD_W / FWD_H                          # (default_camera: fovx = 2 atan(tan(fovy / 2) W / H))
    x = ((2 * px + 1) / FWD_W - 1) * tanx * z
    y = ((2 * py + 1) / FWD_H - 1) * tany * z
    means = np.stack([x, y, z], 1).astype(np.float32)
    assert np.array_equal(means[:, 2].view(np.uint32), key)
    return Scene(f"forward-{kind}", means, tile, key)


def scene_inputs(sc):
    """numpy inputs of the operator for a Scene: precomputed colours, scales of 1e-4, identity rotations, opacity 0.02."""
    P = sc.P
    rot = np.zeros((P, 4), np.float32)
    rot[:, 0] = 1
    col = np.linspace(0.1, 0.9, 3 * P, dtype=np.float32).reshape(P, 3)
    return dict(means3D=sc.means, opacities=np.full((P, 1), 0.02, np.float32), colors_precomp=col,
                scales=np.full((P, 3), 1e-4, np.float32), rotations=rot)


def oracle_rects(sc):
    """oracle.torch_rasterizer.preprocess on the CPU: the (x0, y0, x1, y1) tile rectangle and the depth of every Gaussian."""
    import torch
    from oracle import torch_rasterizer as orc
    from scgaussian_amd import synthetic as syn
    import parity_utils as pu
    cam = syn.default_camera(FWD_W, FWD_H)
    st = pu.oracle_settings(cam, 0, (0.0, 0.0, 0.0))
    a = {k: torch.from_numpy(v) for k, v in scene_inputs(sc).items()}
    with torch.no_grad():
        pre = orc.preprocess(a["means3D"], torch.zeros(sc.P, 3), a["opacities"], st, colors_precomp=a["colors_precomp"],
                             scales=a["scales"], rotations=a["rotations"])
    return pre["rect"].numpy().astype(np.int64), pre["depth"].numpy().astype(np.float32), pre["visible"].numpy()


def run_forward(sc, capacity, options, ws_byte=None):
    """lib.scg_forward through ctypes on a Scene: the workspace starts as PATTERN words (ws_byte: every byte of it as that byte
    instead); rects, depth_keys, point_list (up to the next buffer of the workspace), the ranges words (likewise) are read back
    through scg_workspace_layout."""
    import ctypes as C
    import torch
    from scgaussian_amd import _lib
    from scgaussian_amd import rasterizer as R
    from scgaussian_amd import synthetic as syn
    import parity_utils as pu
    lib = _lib.load()
    dev = torch.device("cuda", torch.cuda.current_device())
    assert lib.scg_binning_accepts_bound(capacity, FWD_W, FWD_H, AUTO) == 1 and 1 <= capacity < (1 << 22)
    st = pu.hip_settings(syn.default_camera(FWD_W, FWD_H), 0, (0.0, 0.0, 0.0))
    inp = {k: torch.from_numpy(v).to(dev) for k, v in scene_inputs(sc).items()}
    P, H, W = sc.P, FWD_H, FWD_W
    L = _lib.ScgWorkspaceLayout()
    R.check(lib.scg_workspace_layout(P, capacity, W, H, C.byref(L)), "scg_workspace_layout")
    ws = torch.empty(int(L.total) + 256, dtype=torch.uint8, device=dev)
    if ws_byte is None:
        ws.view(torch.int32)[:] = int(np.uint32(PATTERN).view(np.int32))
    else:
        ws.fill_(int(ws_byte))
    radii = torch.zeros(P, dtype=torch.int32, device=dev)
    color, depth, alpha = (torch.zeros(n, H, W, device=dev) for n in (3, 1, 1))
    sums = torch.zeros(int(L.partial_words) + 8, dtype=torch.int32, device=dev)
    long_words = torch.full((2,), -1, dtype=torch.int32).pin_memory()
    nr = torch.full((2,), -1, dtype=torch.int32, device=dev)
    frame_ = R._frame_for(st, P, 0, dev)
    c = frame_.c
    saved = (c.tile_cost_in, c.tile_cost_out, c.bwd_cost_in, c.bwd_cost_out, c.long_lists_out, c.num_rendered_out)
    try:
        c.tile_cost_in = c.tile_cost_out = c.bwd_cost_in = c.bwd_cost_out = None
        c.long_lists_out, c.num_rendered_out = long_words.data_ptr(), R.ptr(nr)
        R.check(lib.scg_forward(frame_.ref, R.ptr(inp["means3D"]), R.ptr(inp["opacities"]), None, R.ptr(inp["colors_precomp"]),
                                R.ptr(inp["scales"]), R.ptr(inp["rotations"]), None, capacity, ws.data_ptr(), int(L.total),
                                R.ptr(radii), R.ptr(color), R.ptr(depth), R.ptr(alpha), R.ptr(sums), None, None, options, None,
                                R._stream(dev)), "scg_forward")
        _sync_or_exit(f"scg_forward on scene {sc.name} (capacity {capacity}, options {options})")
    finally:
        (c.tile_cost_in, c.tile_cost_out, c.bwd_cost_in, c.bwd_cost_out, c.long_lists_out, c.num_rendered_out) = saved
    w32 = ws.cpu().numpy().view(np.uint32)
    at = lambda off, n: w32[int(off) // 4: int(off) // 4 + n]
    nw = ranges_words(sc.T)
    assert (int(L.ranges) - int(L.point_list)) // 4 >= capacity and (int(L.final_T) - int(L.ranges)) // 4 >= nw
    image = {k: v.cpu().numpy() for k, v in (("color", color), ("depth", depth), ("alpha", alpha), ("radii", radii))}
    return dict(image, rects=at(L.rects, 2 * P).reshape(P, 2).copy(), depth_keys=at(L.depth_keys, P).copy(),
                point_list=at(L.point_list, (int(L.ranges) - int(L.point_list)) // 4).copy(),
                words=at(L.ranges, (int(L.final_T) - int(L.ranges)) // 4).copy(),
                long_lists=long_words.numpy().copy(), num_rendered_out=int(nr.cpu().numpy().view(np.uint32)[0]),
                sorts_in_blend=int(lib.scg_forward_sorts_in_blend(capacity, W, H, options)))


def compare_forward(ref, out):
    """compare() on what scg_forward left in its workspace: the words between point_list[capacity] (the ranges words) and the next
    buffer of the workspace are the guards (the layout pads every buffer to 256 bytes)."""
    cap, nw = ref["cap"], ranges_words(ref["frame"].T)
    pl, words = out["point_list"], out["words"]
    assert (pl[cap:] == PATTERN).all() and (words[nw:] == PATTERN).all(), "the workspace's padding behind a buffer was written"
    pad = lambda a, n: np.concatenate([a[:n], np.full(GUARD, PATTERN, np.uint32)])
    compare(ref, pad(pl, cap), pad(words, nw), None, out["num_rendered_out"])

"""Frames of the test's own making for the blend stage ALONE (csrc/blend.hip) and plain references of both directions.

A frame is everything scg_blend_forward / scg_blend_backward read (include/scg_raster.h): the 12-float splat records, the tile
lists (`point_list`, `ranges` followed by the tile and the (tile, quadrant) launch-order tables in the layout of
scg_ranges_words) and the upstream gradients.  No geometry, no binning: a list entry sits exactly where the kernels branch.

The builder guarantees what keeps the kernels in bounds: every id < P, every range inside point_list, an id at most once per
tile, both order tables permutations plus padding (check_frame asserts all of it, and every GPU test calls it).

References, per tile, vectorised over its 256 pixels (numpy):
  evaluate(frame, float64, "classic")   the fp64 restatement: forward as the oracle states it (cumprod), backward raw sums
                                        [0..6], [8..10] of the gradient record with (dx, dy) = centre - pixel and
                                        q = opacity G dL/dalpha (unclamped opacity G: the oracle's decision D1)
  evaluate(frame, float32, "classic")   the same at fp32: forward cumprod for T, suffix sums for the colour behind
  evaluate(frame, float32, "kernel")    the kernel's formulation at fp32: conic pre-multiplied by 0.5 log2 e, exp2, the B
                                        recurrence of the comment in front of backward_walk, T recovered by division
The constants are the kernel's fp32 values (0.99f, 1.0f/255.0f, 1e-4f) cast up.  Every output comes with the sum of the
absolute values of its terms; errors are normalised by it (normalised_error).  Splat centres, and nothing else, lie on
multiples of 1/64 px: centre - pixel is exact in fp32, and a pattern shifted by 8 or 16 px gives the same bits.
"""
from __future__ import annotations

import functools

import numpy as np

TILE = 16
F32, F64 = np.float32, np.float64
A_MAX, A_MIN, T_EPS = F32(0.99), F32(1.0) / F32(255.0), F32(1e-4)
HALF_LOG2E = F32(0.72134752044448170)
USED = (0, 1, 2, 3, 4, 5, 6, 8, 9, 10)                   # slots of the 16-float record the backward writes
REC_NAMES = ("S_x", "S_y", "ddepth", "S_q", "S_xx", "S_xy", "S_yy", "dr", "dg", "db")
REL = 1e-3                                               # planted threshold members sit this far (relative) from their threshold


# ---------------------------------------------------------------------------------------------------------------- members

def member(x, y, conic, op, tag="", rgb=None, depth=None):
    """One splat, coordinates local to its TILE (the builder adds the tile's origin)."""
    return dict(x=float(x), y=float(y), ca=float(conic[0]), cb=float(conic[1]), cc=float(conic[2]), op=float(op), tag=tag,
                rgb=rgb, depth=depth)


def qxy(q, px, py):
    """Tile-local coordinates of pixel (px, py) of quadrant q."""
    return 8 * (q & 1) + px, 8 * (q >> 1) + py


def dot(q, px, py, op, off=(0, 0), c=24.0, tag="dot"):
    """Blends pixel (px, py) of quadrant q and no other: at c = 24 a neighbour sees alpha <= op e^-9."""
    x, y = qxy(q, px, py)
    return member(x + off[0] / 64.0, y + off[1] / 64.0, (c, 0.0, c), op, tag)


def exact(q, px, py, op, tag):
    """Centred on the pixel: G = 1 exactly in every formulation, alpha = min(0.99f, opacity) to the bit."""
    return dot(q, px, py, op, tag=tag)


def blob(q, rng, op=None, tag="blob"):
    """Covers a good part of quadrant q and nothing outside it: the conic's smaller eigenvalue is >= 0.75, the centre within
    3/8 px of the quadrant's centre, so alpha at the nearest outside pixel (4.1 px away) is below 0.9 e^-6.3 < 1/255 / 2."""
    lam1, lam2 = rng.uniform(0.75, 1.1), rng.uniform(0.8, 3.0)
    th = rng.uniform(0, np.pi)
    c, s = np.cos(th), np.sin(th)
    ca, cb, cc = lam1 * c * c + lam2 * s * s, (lam1 - lam2) * c * s, lam1 * s * s + lam2 * c * c
    x, y = qxy(q, 3.5, 3.5)
    ox, oy = rng.integers(-24, 25, 2) / 64.0
    return member(x + ox, y + oy, (ca, cb, cc), rng.uniform(0.3, 0.9) if op is None else op, tag)


def reach(q, centre, conic, pixels, tag):
    """A member centred at `centre` (quadrant-local) whose opacity puts alpha REL above 1/255 at the pixel of `pixels` (quadrant-
    local) where it is weakest — and nowhere else in the quadrant within 1 % of the threshold (asserted)."""
    ca, cb, cc = conic
    gx, gy = np.meshgrid(np.arange(8.0), np.arange(8.0))
    dx, dy = centre[0] - gx, centre[1] - gy
    form = ca * dx * dx + 2 * cb * dx * dy + cc * dy * dy
    sel = np.zeros((8, 8), bool)
    for (px, py) in pixels:
        sel[py, px] = True
    op = float(A_MIN) * (1 + REL) * np.exp(0.5 * form[sel].max())
    assert op <= 1.0, (tag, op)
    alpha_out = op * np.exp(-0.5 * form[~sel])
    assert alpha_out.max() < float(A_MIN) * 0.99, (tag, alpha_out.max() / float(A_MIN))
    x, y = qxy(q, *centre)
    return member(x, y, conic, op, tag)


def cull_edge_members(q):
    """Edge class 5: centres outside the quadrant (or on its border pixel) that reach one corner pixel or one edge row."""
    out = []
    r = np.sqrt(0.999)
    for kx, ky in ((0, 0), (7, 0), (0, 7), (7, 7)):
        sx, sy = (-1 if kx == 0 else 1), (-1 if ky == 0 else 1)
        name = f"corner{kx}{ky}"
        c1 = (kx + sx, ky + sy)
        out += [reach(q, c1, (1.5, 0.0, 1.5), [(kx, ky)], f"cull:{name}:iso"),
                reach(q, c1, (3.0, 0.0, 0.75), [(kx, ky)], f"cull:{name}:aniso"),
                # cb^2 = 0.999 ca cc, the ridge of the form pointing away from the quadrant: cb > 0 at two corners, < 0 at the others
                reach(q, c1, (0.6, 0.6 * r * sx * sy, 0.6), [(kx, ky)], f"cull:{name}:neardeg{'+' if sx * sy > 0 else '-'}"),
                reach(q, (kx, ky), (4.0, 0.0, 4.0), [(kx, ky)], f"cull:{name}:onborder"),
                reach(q, (kx + 0.5 * sx, ky + 0.5 * sy), (4.0, 0.0, 4.0), [(kx, ky)], f"cull:{name}:half")]
    row = lambda y: [(x, y) for x in range(8)]
    col = lambda x: [(x, y) for y in range(8)]
    out += [reach(q, (3.5, -1.0), (0.02, 0.0, 5.0), row(0), "cull:edge_top:aniso"),
            reach(q, (3.5, 8.0), (0.02, 0.0, 5.0), row(7), "cull:edge_bottom:aniso"),
            reach(q, (-1.0, 3.5), (5.0, 0.0, 0.02), col(0), "cull:edge_left:aniso"),
            reach(q, (8.0, 3.5), (5.0, 0.0, 0.02), col(7), "cull:edge_right:aniso"),
            reach(q, (3.0, -1.0), (1e-6, 9e-4, 5.0), row(0), "cull:edge_top:tiny_ca"),
            reach(q, (4.0, 8.0), (1e-6, -9e-4, 5.0), row(7), "cull:edge_bottom:tiny_ca")]
    return out


# ------------------------------------------------------------------------------------------------------------------ frames

class Frame:
    """W, H, bg (3,), splats (P, 12) with the cull fields as geometry.hip writes them, point_list (R,) uint32, ranges (T, 2)
    uint32, dL_dcolor (3, H, W), dL_ddepth (H, W), dL_dalpha (H, W), tags (P,) — all numpy, fp32 / uint32."""

    def __init__(self, name, W, H, bg):
        self.name, self.W, self.H = name, int(W), int(H)
        self.bg = np.asarray(bg, F32)
        self.gx, self.gy = (W + TILE - 1) // TILE, (H + TILE - 1) // TILE
        self.T = self.gx * self.gy
        self._rec, self.tags, self._lists = [], [], [[] for _ in range(self.T)]
        self._rng = np.random.default_rng(sum(map(ord, name)) * 7919 + W * 131 + H)       # colours and depths

    # -- building
    def add(self, t, m):
        """A new Gaussian from member m (tile-local coordinates, relative to tile t); returns its id."""
        rng = self._rng
        tx, ty = t % self.gx, t // self.gx
        rgb = m["rgb"] if m["rgb"] is not None else rng.uniform(0.05, 1.0, 3)
        depth = m["depth"] if m["depth"] is not None else rng.uniform(1.0, 5.0)
        self._rec.append([m["x"] + TILE * tx, m["y"] + TILE * ty, m["ca"], m["cb"], m["cc"], m["op"], 0.0, 0.0, *rgb, depth])
        self.tags.append(m["tag"])
        return len(self._rec) - 1

    def set_list(self, t, entries):
        """entries: members (a new Gaussian each) or ints (ids of Gaussians that exist already)."""
        ids = [e if isinstance(e, (int, np.integer)) else self.add(t, e) for e in entries]
        assert len(set(ids)) == len(ids), "an id appears at most once per tile"
        self._lists[t] = [int(i) for i in ids]

    def finish(self, upstream="all", seed=0, upstream_pattern=None):
        rec = np.asarray(self._rec, F64).reshape(-1, 12)
        assert np.array_equal(rec[:, :2] * 64, np.round(rec[:, :2] * 64)), "centres on multiples of 1/64 px"
        self.splats = rec.astype(F32)
        op, cb, cc = self.splats[:, 5], self.splats[:, 3], self.splats[:, 4]
        with np.errstate(divide="ignore", invalid="ignore"):
            self.splats[:, 6] = F32(2.0) * np.log(F32(255.0) * op).astype(F32) * F32(1.001) + F32(0.01)
            self.splats[:, 7] = -cb / cc
        self.P = len(rec)
        self.point_list = np.asarray([i for l in self._lists for i in l], np.uint32)
        ends = np.cumsum([len(l) for l in self._lists])
        self.ranges = np.zeros((self.T, 2), np.uint32)
        for t, l in enumerate(self._lists):
            if l:                                                       # (untouched tiles: 0, 0 — as the binning stage writes them)
                self.ranges[t] = (ends[t] - len(l), ends[t])
        g = np.random.default_rng(seed + 1000)
        H, W = self.H, self.W
        if upstream_pattern is not None:                                # the same 8 x 8 upstream in every quadrant
            reps = ((H + 7) // 8, (W + 7) // 8)
            dC = np.stack([np.tile(upstream_pattern[c], reps)[:H, :W] for c in range(3)])
            dD, dA = np.tile(upstream_pattern[3], reps)[:H, :W], np.tile(upstream_pattern[4], reps)[:H, :W]
        else:
            dC, dD, dA = g.standard_normal((3, H, W)), g.standard_normal((H, W)), g.standard_normal((H, W))
        if upstream == "depth_only":
            dC, dA = np.zeros_like(dC), np.zeros_like(dA)
        elif upstream == "alpha_only":
            dC, dD = np.zeros_like(dC), np.zeros_like(dD)
        self.dL_dcolor, self.dL_ddepth, self.dL_dalpha = (np.ascontiguousarray(a, F32) for a in (dC, dD, dA))
        self.tags = np.asarray(self.tags, dtype=object)
        check_frame(self)
        return self

    # -- what the kernels read
    def splats_for(self, cull=True):
        """cull=False: cull_thr = +inf — every quadrant walks every entry of its tile's list."""
        s = self.splats.copy()
        if not cull:
            s[:, 6] = np.inf
        return s

    def ranges_words(self, order="identity", seed=0):
        """ranges | tile launch order (8 bands of ceil(T/8) slots, padded with T) | (tile, quadrant) launch order (4 entries per
        slot, padded with 4 T) — the layout of scg_ranges_words.  order: identity | reversed | shuffled (within every band)."""
        T, per = self.T, (self.T + 7) // 8
        rng = np.random.default_rng(seed + 77)
        tile_o, quad_o = [], []
        for band in range(8):
            tiles = [t for t in range(band * per, min((band + 1) * per, T))]
            ts = tiles + [T] * (per - len(tiles))
            qs = [4 * t + q for t in tiles for q in range(4)] + [4 * T] * (4 * (per - len(tiles)))
            if order == "reversed":
                ts, qs = ts[::-1], qs[::-1]
            elif order == "shuffled":
                ts, qs = list(rng.permutation(ts)), list(rng.permutation(qs))
            else:
                assert order == "identity", order
            tile_o += ts
            quad_o += qs
        words = np.concatenate([self.ranges.reshape(-1), np.asarray(tile_o, np.uint32), np.asarray(quad_o, np.uint32)]).astype(np.uint32)
        assert len(words) == 2 * T + 5 * 8 * per
        check_order_tables(words, T)
        return words

    def tile_ids(self, t):
        s, e = self.ranges[t]
        return self.point_list[s:e].astype(np.int64)

    def tile_pixels(self, t):
        tx, ty = t % self.gx, t // self.gx
        loc = np.arange(TILE * TILE)
        px, py = TILE * tx + loc % TILE, TILE * ty + loc // TILE
        return px, py, (px < self.W) & (py < self.H)


def check_order_tables(words, T):
    per = (T + 7) // 8
    tile_o, quad_o = words[2 * T: 2 * T + 8 * per], words[2 * T + 8 * per:]
    assert len(quad_o) == 32 * per
    assert sorted(tile_o.tolist()) == list(range(T)) + [T] * (8 * per - T)
    assert sorted(quad_o.tolist()) == list(range(4 * T)) + [4 * T] * (32 * per - 4 * T)


def check_frame(fr):
    """What keeps the kernels in bounds."""
    assert fr.splats.shape == (fr.P, 12) and fr.splats.dtype == F32 and fr.P >= 1
    assert fr.point_list.dtype == np.uint32 and (len(fr.point_list) == 0 or int(fr.point_list.max()) < fr.P)
    assert fr.ranges.shape == (fr.T, 2) and fr.T <= 18
    for t in range(fr.T):
        s, e = int(fr.ranges[t, 0]), int(fr.ranges[t, 1])
        assert 0 <= s <= e <= len(fr.point_list) and e - s <= 400
        ids = fr.point_list[s:e]
        assert len(np.unique(ids)) == len(ids)
    assert fr.dL_dcolor.shape == (3, fr.H, fr.W) and fr.dL_ddepth.shape == (fr.H, fr.W) == fr.dL_dalpha.shape
    finite = fr.splats[:, [0, 1, 2, 3, 4, 5, 8, 9, 10, 11]]
    assert np.isfinite(finite).all()


# -------------------------------------------------------------------------------------------------------------- references

def _fma(a, b, c, dtype):
    if dtype == F32:                                # the product is exact in fp64; one more rounding than the hardware's, rarely
        return (a.astype(F64) * b.astype(F64) + c.astype(F64)).astype(F32)
    return a * b + c


def _tile_terms(fr, t, dtype, form, splats):
    ids = fr.tile_ids(t)
    S = splats[ids].astype(dtype)
    px, py, inside = fr.tile_pixels(t)
    x, y, ca, cb, cc, op = (S[:, k][None, :] for k in range(6))
    dx, dy = x - px.astype(dtype)[:, None], y - py.astype(dtype)[:, None]
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        if form == "kernel":
            k = dtype(HALF_LOG2E)
            ca_, cb2_, cc_ = k * ca, (dtype(2.0) * k) * cb, k * cc
            u = _fma(np.broadcast_to(cb2_, dy.shape), dy, ca_ * dx, dtype)
            tt = _fma(u, dx, (cc_ * dy) * dy, dtype)
            G, tge0 = np.exp2(-tt), tt >= 0
        else:
            power = dtype(-0.5) * (ca * dx * dx + cc * dy * dy) - cb * dx * dy
            G, tge0 = np.exp(power), power <= 0
        oG = op * G
    alpha = np.minimum(dtype(A_MAX), oG)
    valid0 = tge0 & (alpha >= dtype(A_MIN)) & inside[:, None]
    return dict(ids=ids, S=S, dx=dx, dy=dy, oG=oG, alpha=alpha, tge0=tge0, age=alpha >= dtype(A_MIN), valid0=valid0, inside=inside)


def _forward_classic(tm, bg, dtype):
    alpha, valid0 = tm["alpha"], tm["valid0"]
    npx, n = alpha.shape
    a_eff = np.where(valid0, alpha, dtype(0))
    T_after = np.cumprod(dtype(1) - a_eff, axis=1, dtype=dtype)
    T_before = np.concatenate([np.ones((npx, 1), dtype), T_after[:, :-1]], 1)[:, :n]
    live = T_after >= dtype(T_EPS)
    contrib = valid0 & live
    stop = valid0 & ~live
    term = np.where(stop.any(1), stop.argmax(1), -1) if n else np.full(npx, -1)
    n_live = live.sum(1)
    Tf = np.where(n_live > 0, np.take_along_axis(T_after, np.maximum(n_live - 1, 0)[:, None], 1)[:, 0], dtype(1)) if n else np.ones(npx, dtype)
    w = np.where(contrib, alpha * T_before, dtype(0))
    return contrib, term, T_before, Tf.astype(dtype), w, T_after


def _forward_kernel(tm, bg, dtype):
    alpha, valid0 = tm["alpha"], tm["valid0"]
    npx, n = alpha.shape
    T, live = np.ones(npx, dtype), tm["inside"].copy()
    contrib, T_before, T_test = np.zeros((npx, n), bool), np.ones((npx, n), dtype), np.ones((npx, n), dtype)
    term = np.full(npx, -1)
    w = np.zeros((npx, n), dtype)
    for i in range(n):
        a = alpha[:, i]
        valid = live & valid0[:, i]
        test = _fma(-T, a, T, dtype)
        c = valid & (test >= dtype(T_EPS))
        stop = valid & ~c
        term[stop] = i
        live &= ~stop
        contrib[:, i], T_before[:, i], T_test[:, i] = c, T, test
        w[:, i] = np.where(c, T * a, dtype(0))
        T = np.where(c, test, T)
    return contrib, term, T_before, T, w, T_test


def evaluate(fr, dtype=F64, form="classic", cull=True):
    """Both directions of one frame.  `cull` only picks which splat table is read (the references never look at the cull
    fields).  Returns images, state, records (P, 10) in the order of USED, the sums of absolute terms of everything, and the
    per-tile decision arrays."""
    assert form in ("classic", "kernel") and (form == "classic" or dtype == F32)
    H, W, P = fr.H, fr.W, fr.P
    splats = fr.splats_for(cull)
    bg = fr.bg.astype(dtype)
    img = {k: np.zeros((H, W), dtype) for k in ("r", "g", "b", "depth", "alpha", "final_T", "n_r", "n_g", "n_b", "n_depth", "n_alpha")}
    n_contrib = np.zeros((H, W), np.int64)
    rec, rec_abs = np.zeros((P, 10), dtype), np.zeros((P, 10), dtype)
    blended_in = np.zeros((P, fr.T, 4), bool)                            # id blended by a pixel of (tile, quadrant)
    tiles = []
    gup = np.concatenate([fr.dL_dcolor, fr.dL_ddepth[None], fr.dL_dalpha[None]]).astype(dtype)      # (5, H, W)
    for t in range(fr.T):
        tm = _tile_terms(fr, t, dtype, form, splats)
        px, py, inside = fr.tile_pixels(t)
        n = len(tm["ids"])
        fw = (_forward_kernel if form == "kernel" else _forward_classic)(tm, bg, dtype)
        contrib, term, T_before, Tf, w, T_aux = fw
        col = tm["S"][:, 8:12]                                           # r, g, b, depth
        if form == "kernel":
            acc = np.zeros((TILE * TILE, 4), dtype)
            for i in range(n):
                acc = _fma(np.broadcast_to(col[i][None, :], acc.shape), np.broadcast_to(w[:, i:i + 1], acc.shape), acc, dtype)
        else:
            acc = (w[:, :, None] * col[None, :, :]).sum(1, dtype=dtype) if n else np.zeros((TILE * TILE, 4), dtype)
        acc_abs = (w[:, :, None] * np.abs(col)[None, :, :]).sum(1, dtype=dtype) if n else np.zeros((TILE * TILE, 4), dtype)
        idx = np.arange(1, n + 1)[None, :]
        last = np.where(contrib, idx, 0).max(1) if n else np.zeros(TILE * TILE, np.int64)
        ii = inside
        yy, xx = py[ii], px[ii]
        for c, k in enumerate("rgb"):
            img[k][yy, xx] = (acc[:, c] + Tf * bg[c])[ii]
            img["n_" + k][yy, xx] = (acc_abs[:, c] + Tf * np.abs(bg[c]))[ii]
        img["depth"][yy, xx], img["n_depth"][yy, xx] = acc[ii, 3], acc_abs[ii, 3]
        img["alpha"][yy, xx], img["n_alpha"][yy, xx] = (dtype(1) - Tf)[ii], (dtype(1) + Tf)[ii]
        img["final_T"][yy, xx] = Tf[ii]
        n_contrib[yy, xx] = last[ii]
        # ---- backward raw sums
        g = np.zeros((TILE * TILE, 5), dtype)
        g[ii] = gup[:, yy, xx].T
        bgdot = bg[0] * g[:, 0] + bg[1] * g[:, 1] + bg[2] * g[:, 2]
        oG = np.where(contrib, tm["oG"], dtype(0))
        if form == "kernel":
            q = np.zeros_like(w)
            wb = np.zeros_like(w)
            T, behind = Tf.copy(), bgdot.copy()
            for i in range(n - 1, -1, -1):
                if not contrib[:, i].any():
                    continue
                a = np.clip(oG[:, i], dtype(0), dtype(A_MAX))
                one_m = dtype(1) - a
                T = T / one_m
                d = g[:, 4]
                for c in (3, 2, 1, 0):
                    d = _fma(np.broadcast_to(col[i, c], d.shape), g[:, c], d, dtype)
                q[:, i] = oG[:, i] * ((d - behind) * T)
                behind = _fma(a, d, behind * one_m, dtype)
                wb[:, i] = a * T
        else:
            d = g[:, :4] @ col.T + g[:, 4:5] if n else np.zeros((TILE * TILE, 0), dtype)
            wd = w * d
            suffix = np.cumsum(wd[:, ::-1], axis=1, dtype=dtype)[:, ::-1] - wd + (Tf * bgdot)[:, None]
            with np.errstate(invalid="ignore", divide="ignore"):
                dlda = T_before * d - suffix / (dtype(1) - np.where(contrib, tm["alpha"], dtype(0)))
            q = np.where(contrib, oG * dlda, dtype(0))
            wb = w
        dx, dy = tm["dx"], tm["dy"]
        terms = [q * dx, q * dy, wb * g[:, 3:4], q, q * dx * dx, q * dx * dy, q * dy * dy, wb * g[:, 0:1], wb * g[:, 1:2], wb * g[:, 2:3]]
        for k, term_k in enumerate(terms):
            if n:
                np.add.at(rec[:, k], tm["ids"], term_k.sum(0, dtype=dtype))
                np.add.at(rec_abs[:, k], tm["ids"], np.abs(term_k).sum(0, dtype=dtype))
        quad = ((np.arange(256) % 16) >= 8) + 2 * ((np.arange(256) // 16) >= 8)
        for qd in range(4):
            if n:
                blended_in[tm["ids"], t, qd] = contrib[quad == qd].any(0)
        tiles.append(dict(ids=tm["ids"], contrib=contrib, term=term, tge0=tm["tge0"], age=tm["age"], oG=tm["oG"], alpha=tm["alpha"],
                          T_before=T_before, T_aux=T_aux, last=last, inside=inside, quad=quad, n=n, w=w))
    return dict(color=np.stack([img["r"], img["g"], img["b"]]), depth=img["depth"], alpha=img["alpha"], final_T=img["final_T"],
                n_contrib=n_contrib, norm=dict(color=np.stack([img["n_r"], img["n_g"], img["n_b"]]), depth=img["n_depth"],
                                               alpha=img["n_alpha"], final_T=img["final_T"]),
                rec=rec, rec_abs=rec_abs, blended_in=blended_in, tiles=tiles)


def normalised_error(x, ref, norm):
    """|x - ref| / norm element-wise in fp64; 0 where the two are equal (a norm of 0 with a difference is inf: it fails)."""
    d = np.abs(np.asarray(x, F64) - np.asarray(ref, F64))
    with np.errstate(divide="ignore", invalid="ignore"):
        e = d / np.asarray(norm, F64)
    return np.where(d == 0, 0.0, e)


@functools.lru_cache(maxsize=None)
def reference(frame_key):
    """Per frame, once: the fp64 reference, e32 per output (the larger of the two fp32 evaluations' normalised errors) and the
    decision-margin verdict."""
    fr = frame(frame_key)
    r64 = evaluate(fr, F64, "classic")
    r32 = [evaluate(fr, F32, "classic"), evaluate(fr, F32, "kernel")]
    e32 = {}
    for k in ("color", "depth", "alpha", "final_T"):
        e32[k] = max(float(normalised_error(r[k], r64[k], r64["norm"][k]).max()) for r in r32)
    for j, nm in enumerate(REC_NAMES):
        e32[nm] = max(float(normalised_error(r["rec"][:, j], r64["rec"][:, j], r64["rec_abs"][:, j]).max()) for r in r32)
    return dict(frame=fr, r64=r64, r32=r32, e32=e32, same_decisions=same_decisions(r64, r32))


def same_decisions(r64, r32s):
    """The condition: for every (pixel, entry) the fp32 restatements decide as fp64 on t >= 0, alpha >= 1/255 and
    T (1 - alpha) >= 1e-4 (the last wherever it is asked: contributors and the terminating entry)."""
    for r in r32s:
        if not np.array_equal(r["n_contrib"], r64["n_contrib"]):
            return False
        for a, b in zip(r["tiles"], r64["tiles"]):
            ins = a["inside"]
            if not (np.array_equal(a["tge0"][ins], b["tge0"][ins]) and np.array_equal(a["age"][ins], b["age"][ins]) and
                    np.array_equal(a["contrib"], b["contrib"]) and np.array_equal(a["term"], b["term"])):
                return False
    return True


# ------------------------------------------------------------------------------------------------------ the planted frames

def _fill(n, hits, filler):
    """A list of n entries: hits {position: member}, every other position filler(position)."""
    assert all(0 <= p < n for p in hits)
    return [hits[p] if p in hits else filler(p) for p in range(n)]


def far(p):
    """Fails every quadrant's cull and blends nowhere (the centre is 40 px away from the tile)."""
    return member(-40.0 - (p % 7), -40.0, (24.0, 0.0, 24.0), 0.5, "pad:far")


def passing(q):
    """Passes quadrant q's cull (the centre lies inside its rectangle) and blends nowhere: half-way between four pixels,
    alpha = 0.5 e^-10 there."""
    def f(p):
        x, y = qxy(q, (p % 7) + 0.5, ((p // 7) % 7) + 0.5)
        return member(x, y, (40.0, 0.0, 40.0), 0.5, "pad:pass")
    return f


def faint(q, op):
    """Opacity 0 or 0.003 on a pixel of quadrant q: passes only a cull that is switched off, and then nobody blends it."""
    def f(p):
        return dot(q, p % 8, (p // 8) % 8, op, tag="pad:faint")
    return f


def mixed(q):
    return lambda p: (far, passing(q), faint(q, 0.0), faint(q, 0.003))[p % 4](p)


def pattern(rng, q=0):
    """The single-quadrant pattern of the bit-exact properties: 13 members inside quadrant q, stacks on shared pixels,
    a clamped one, one either side of the 1/255 cut."""
    ms = [blob(q, rng) for _ in range(6)]
    ms += [dot(q, 1, 1, 0.7, (5, -3)), dot(q, 1, 1, 0.6, (-8, 2)), dot(q, 6, 2, 0.995, (0, 0), tag="clamped"),
           dot(q, 6, 2, 0.4, (3, 3)), exact(q, 2, 6, float(A_MIN) * (1 + REL), "amin+"), exact(q, 3, 6, float(A_MIN) * (1 - REL), "amin-"),
           blob(q, rng, 0.95)]
    return ms


def _shift(m, q):
    """Member m of quadrant 0 moved to quadrant q (8 px steps: the same bits)."""
    m = dict(m)
    m["x"], m["y"] = m["x"] + 8 * (q & 1), m["y"] + 8 * (q >> 1)
    return m


def _pattern_members(seed=5):
    """The pattern with colours and depths fixed (every copy carries the same record but for the centre)."""
    rng = np.random.default_rng(seed)
    ms = pattern(rng)
    for m in ms:
        m["rgb"], m["depth"] = rng.uniform(0.05, 1.0, 3), rng.uniform(1.0, 5.0)
    up = rng.standard_normal((5, 8, 8))
    return ms, up


def translation_frame(key):
    """Frames (d) / (e) with a copy of the pattern in every quadrant of every tile; a tile's list interleaves its four copies,
    starting with a different quadrant in every tile."""
    W, H = {"d": (40, 25), "e": (129, 17)}[key]
    fr = Frame("translation-" + key, W, H, (0.3, 0.6, 0.1))
    ms, up = _pattern_members()
    fr.copy_ids = {}
    for t in range(fr.T):
        ids = {q: [fr.add(t, _shift(m, q)) for m in ms] for q in range(4)}
        order = [(q + t) % 4 for q in range(4)]
        fr.set_list(t, [ids[q][j] for j in range(len(ms)) for q in order])
        for q in range(4):
            fr.copy_ids[(t, q)] = ids[q]
    return fr.finish(upstream_pattern=up)


PAD_KS = (1, 61, 62, 63, 64, 65, 127)


def padding_frame(k):
    """One 16 x 16 tile: the pattern in quadrant 0, k padding entries in front (k = 0: none anywhere) and, for k > 0, padding
    interleaved between the hits: entries that fail the cull, entries that pass it and blend nowhere, entries that blend in a
    sibling quadrant only (a copy of the pattern in quadrant 3)."""
    fr = Frame(f"padding-{k}", 16, 16, (0.3, 0.6, 0.1))
    ms, up = _pattern_members()
    ids = [fr.add(0, m) for m in ms]
    fr.pattern_ids = ids
    entries = []
    if k:
        sib = [fr.add(0, _shift(m, 3)) for m in ms]
        pads = [far, passing(0), None]
        front = []
        for p in range(k):
            kind = pads[p % 3]
            front.append(sib.pop(0) if (kind is None and sib) else fr.add(0, (kind or far)(p)))
        entries += front
        for j, i in enumerate(ids):
            entries.append(i)
            for p in range(j % 4):
                kind = pads[(p + j) % 3]
                entries.append(sib.pop(0) if (kind is None and sib) else fr.add(0, (kind or passing(0))(p + 3 * j)))
        entries += sib
    else:
        entries = ids
    fr.set_list(0, entries)
    return fr.finish(upstream_pattern=up)


PHASE_KS = (1, 2, 3)


def phase_frame(k):
    """padding-0 with k more list entries in front that quadrant 0 DOES blend — dots on its corner pixels, which no member of
    the pattern reaches: every member's per-pixel weights stay what they were, but it sits k rows further in the backward's
    four-row block, so members move between rows and between the full and the partial flush."""
    fr = Frame(f"phase-{k}", 16, 16, (0.3, 0.6, 0.1))
    ms, up = _pattern_members()
    ids = [fr.add(0, m) for m in ms]
    fr.pattern_ids = ids
    corners = [(0, 0), (7, 0), (0, 7)]
    front = [fr.add(0, dot(0, *corners[j], 0.5 + 0.1 * j, (j, -j), tag="phase")) for j in range(k)]
    fr.set_list(0, ids[:5] + front + ids[5:])                       # (in the middle of the list: members behind AND in front of them move)
    return fr.finish(upstream_pattern=up)


def _stack_terminators(q):
    """Two flat opaque splats over quadrant q: opacity G >= 0.99 on all its pixels, so the first leaves T = 1 - 0.99f and the
    second terminates every pixel of q WITHOUT being blended ((1 - 0.99f)^2 < 1e-4f); sibling quadrants see smaller alphas."""
    x, y = qxy(q, 3.5, 3.5)
    return [member(x, y, (6e-4, 0.0, 6e-4), 1.0, "term:stack"), member(x + 0.25, y, (6e-4, 0.0, 6e-4), 1.0, "term:stack")]


def _frame_a():
    fr = Frame("a", 1, 1, (0.2, 0.5, 0.9))
    rng = np.random.default_rng(1)
    fr.set_list(0, [dot(0, 0, 0, 0.5, (7, -5)), blob(0, rng), dot(0, 0, 0, 0.3, (-3, 9))])
    return fr.finish(seed=1)


def _frame_b():
    """8 x 8: quadrants 1-3 of the only tile lie outside the image.  n = 65: hits first, at 63 and at 64 (last)."""
    fr = Frame("b", 8, 8, (0.0, 0.25, 1.0))
    rng = np.random.default_rng(2)
    hits = {0: blob(0, rng), 1: dot(0, 2, 2, 0.6, (4, 4)), 30: blob(0, rng), 63: blob(0, rng), 64: dot(0, 2, 2, 0.5, (-6, 1)),
            40: blob(1, rng), 41: blob(2, rng), 42: blob(3, rng)}              # (members of the quadrants outside the image)
    fr.set_list(0, _fill(65, hits, mixed(0)))
    return fr.finish(seed=2)


def _frame_c():
    """16 x 16, one whole tile, n = 200.  q0: hits first, last and either side of every multiple of 64.  q1: per-pixel `last`
    in four different chunks.  q2: highest `last` in chunk 0 (n reaches chunk 3), 5 blended entries.  q3: the alpha
    decisions, one pixel each, and a chunk (64..127) whose only passing entries blend nowhere."""
    fr = Frame("c", 16, 16, (0.7, 0.1, 0.4))
    rng = np.random.default_rng(3)
    hits = {}
    for j, p in enumerate((0, 63, 64, 65, 127, 128, 129, 191, 192, 199)):
        hits[p] = blob(0, rng) if j % 2 == 0 else dot(0, j % 8, (3 * j) % 8, 0.5 + 0.04 * j, (j, -j))
    for j, p in enumerate((10, 70, 130, 198)):                                # q1: pixel (j, 1) ends in chunk j ...
        hits[p] = dot(1, j, 1, 0.6, (2 * j, 3))
    for j, p in enumerate((3, 5, 66, 67, 131)):                               # ... in front of it a few shared entries
        hits[p] = blob(1, rng) if p < 64 else dot(1, 3, 1, 0.3, (j, j))
    for j, p in enumerate((2, 4, 6, 8, 12)):                                  # q2: everything in chunk 0
        hits[p] = blob(2, rng) if j < 2 else dot(2, j, 2 * j - 2, 0.8, (-j, j))
    a = float(A_MIN)
    q3 = [exact(3, 0, 0, a * (1 + REL), "amin+"), exact(3, 1, 0, a * (1 - REL), "amin-"),
          exact(3, 2, 0, float(A_MAX) * (1 + REL), "amax+"), exact(3, 3, 0, float(A_MAX) * (1 - REL), "amax-"),
          exact(3, 4, 0, 0.0, "op0"), exact(3, 5, 0, a, "op_amin"), exact(3, 6, 0, 1.0, "op1"),
          # indefinite conic (its null directions have irrational slopes: no pixel sits on t = 0 but the centre): t < 0 in a
          # double wedge through all four quadrants where opacity G would pass, blended next to the wedge — a member of every quadrant
          member(*qxy(3, 3, 4), (0.5, -0.55, 0.5), 0.5, "indefinite"),
          dot(3, 2, 0, 0.5, (3, 1)), dot(3, 3, 0, 0.5, (1, 3)), dot(3, 6, 0, 0.5, (2, 2)), dot(3, 0, 0, 0.5, (2, -2))]
    for j, m in enumerate(q3):
        hits[20 + 2 * j] = m
    hits[150] = dot(3, 7, 7, 0.5, (1, 1))                                     # q3 walks chunk 1 (64..127: passing(3) below) and blends nothing there
    filler = lambda p: passing(3)(p) if 64 <= p < 128 else mixed(p % 4)(p)
    fr.set_list(0, _fill(200, hits, filler))
    return fr.finish(seed=3)


def _frame_d():
    """40 x 25: 6 tiles, 2 padding slots, partial tiles on both edges.  Tile 0: n = 0.  Tile 1: n = 1.  Tile 2: n = 2.
    Tile 3: n = 63 and the quadrant-cull members.  Tile 4: n = 64, the termination members.  Tile 5: n = 129 (partial on both
    axes), blended entries per quadrant 7 / 8 and a terminated quadrant."""
    fr = Frame("d", 40, 25, (0.9, 0.2, 0.5))
    rng = np.random.default_rng(4)
    everywhere = fr.add(0, member(20.0, 12.0, (2e-3, 0.0, 3e-3), 0.35, "multi:every_tile"))     # (tile-local to tile 0 = absolute)
    fr.set_list(0, [])
    fr.set_list(1, [blob(2, rng)])
    fr.set_list(2, [everywhere, blob(0, rng), blob(1, rng)])
    cull = cull_edge_members(0)
    assert len(cull) == 26
    hits = {2 * j + 1: m for j, m in enumerate(cull)}
    hits[0] = everywhere
    hits[60], hits[62] = blob(3, rng), blob(3, rng)
    fr.set_list(3, _fill(63, hits, mixed(0)))
    # tile 4 (row 1: 9 image rows, quadrants 2, 3 have one row): termination, one pixel each, in quadrant 0 and 1
    h = {}
    h[3], h[4] = exact(0, 1, 1, 1.0, "term:clamped"), exact(0, 1, 1, 1.0, "term:clamped")     # the second terminates unblended
    # pairs either side of 1e-4: T = 0.004 after three exact members, then alpha = 0.975 with T (1 - alpha) = 1e-4 (1 +- 1e-3)
    for j, sgn in enumerate((+1, -1)):
        px = 3 + j
        h[6 + j], h[10 + j], h[12 + j] = exact(0, px, 1, 0.9, "exact"), exact(0, px, 1, 0.8, "exact"), exact(0, px, 1, 0.8, "exact")
        T2 = float(F32(F32(1) - F32(0.9)) * (F32(1) - F32(0.8)) * (F32(1) - F32(0.8)))
        h[14 + j] = exact(0, px, 1, 1.0 - float(T_EPS) * (1 + sgn * REL) / T2, f"teps{'+' if sgn > 0 else '-'}")
        h[20 + j] = dot(0, px, 1, 0.5, (1, 1))                                  # behind it: blended only if the pixel lives on
    # a pixel that terminates on the LAST entry of a chunk (63) and one on the FIRST of the next ... tile 4 has n = 64: the
    # first-of-chunk member lives in tile 5
    h[61], h[63] = exact(1, 2, 2, 1.0, "term:clamped"), exact(1, 2, 2, 1.0, "term:chunk_last")
    h[30], h[31], h[32] = blob(0, rng), blob(1, rng), everywhere
    h[40] = member(8.0, 4.0, (0.03, 0.0, 0.05), 0.6, "multi:four_quadrants")
    fr.set_list(4, _fill(64, h, mixed(0)))
    # tile 5: 8 x 9 image pixels (quadrant 1, 3 outside; quadrant 2 one row)
    h = {1: everywhere}
    for j in range(7):
        h[5 + 9 * j] = blob(0, rng) if j % 3 == 0 else dot(0, j, j, 0.4 + 0.05 * j, (j, 2 * j))
    h[62], h[64] = exact(0, 5, 1, 1.0, "term:clamped"), exact(0, 5, 1, 1.0, "term:chunk_first")
    for j in range(8):
        h[66 + 7 * j] = dot(2, j, 0, 0.3 + 0.08 * j, (-j, j))
    fr.set_list(5, _fill(129, h, mixed(0)))
    return fr.finish(seed=4)


def _frame_e(H=17):
    """129 x 17: 9 tile columns, the last one 1 px wide, and a second tile row that is 1 px high (18 tiles, 24 slots, 6 of them
    padding; the last tile is a single pixel).  Top row: n = 127, 128, 65, 200, 2, 64, 129, 63, 1; one Gaussian covers every
    tile, one is in the lists of tiles 4 and 5 only, quadrant 0 of tile 3 is terminated as a whole by entries 2 and 3.
    H = 16 (frame "e9") is the top row alone: 9 tiles on 16 slots, 7 of them padding."""
    fr = Frame("e" if H == 17 else "e9", 129, H, (0.1, 0.8, 0.3))
    rng = np.random.default_rng(5)
    everywhere = fr.add(0, member(64.0, 8.0, (3e-4, 0.0, 2e-3), 0.3, "multi:every_tile"))
    two = fr.add(4, member(15.5, 3.0, (0.08, 0.0, 0.3), 0.5, "multi:two_tiles"))           # on the border between tiles 4 and 5
    lens = (127, 128, 65, 200, 2, 64, 129, 63, 1)
    counts = ((0, 1), (2, 3), (4, 6), None, None, (7, 8), (8, 4), (2, 6), None)            # blended entries of quadrants 0, 1 (+ 1)
    for t, n in enumerate(lens):
        if t == 8:
            fr.set_list(t, [everywhere])
            continue
        if t == 4:
            fr.set_list(t, [everywhere, two])
            continue
        h = {0: everywhere}
        if t == 3:
            h[2], h[3] = _stack_terminators(0)
            h[100] = dot(0, 3, 3, 0.5)                                                     # behind the terminators: nobody blends it
            h[190], h[199] = dot(1, 7, 7, 0.9, (1, 1)), dot(1, 7, 6, 0.9, (1, 1))
        else:
            free = list(range(1, n - 1, max(1, (n - 2) // 15)))
            for q in (0, 1):
                for j in range(counts[t][q]):
                    h[free.pop(0)] = blob(q, rng) if j % 2 == 0 else dot(q, (j * 3) % 8, (j * 5) % 8, 0.35 + 0.05 * j, (j, -2 * j))
        if t == 5:
            h[n - 1] = two
        fr.set_list(t, _fill(n, h, mixed(t % 2)))
    for t in range(9, fr.T):                                                               # one image row (tile 17: one pixel)
        fr.set_list(t, [everywhere, dot(0, (t % 8) if t < 17 else 0, 0, 0.6, (t - 9, 1)), far(t)])
    return fr.finish(seed=5)


def _frame_upstream(kind):
    """Frame (b)'s lists with dL_dcolor zero and only depth / only alpha carrying gradient."""
    fr = Frame("b-" + kind, 8, 8, (0.0, 0.25, 1.0))
    rng = np.random.default_rng(2)
    fr.set_list(0, _fill(20, {0: blob(0, rng), 5: blob(0, rng), 19: dot(0, 2, 2, 0.5, (-6, 1)), 7: dot(0, 2, 2, 0.6, (4, 4))}, mixed(0)))
    return fr.finish(upstream=kind, seed=6)


BASE_FRAMES = ("a", "b", "c", "d", "e", "e9")
EXTRA_FRAMES = ("depth_only", "alpha_only")


@functools.lru_cache(maxsize=None)
def frame(key):
    if key in BASE_FRAMES:
        return {"a": _frame_a, "b": _frame_b, "c": _frame_c, "d": _frame_d, "e": _frame_e, "e9": lambda: _frame_e(16)}[key]()
    if key in EXTRA_FRAMES:
        return _frame_upstream(key)
    if key.startswith("translation-"):
        return translation_frame(key.split("-")[1])
    if key.startswith("padding-"):
        return padding_frame(int(key.split("-")[1]))
    if key.startswith("phase-"):
        return phase_frame(int(key.split("-")[1]))
    raise KeyError(key)


ALL_FRAMES = BASE_FRAMES + EXTRA_FRAMES + ("translation-d", "translation-e") + tuple(f"padding-{k}" for k in (0,) + PAD_KS) + \
    tuple(f"phase-{k}" for k in PHASE_KS)


def single_atomic(ref):
    """Every Gaussian is blended in at most one (tile, quadrant): its record receives a single atomic, the sums have no order."""
    return bool((ref["r64"]["blended_in"].reshape(ref["frame"].P, -1).sum(1) <= 1).all())


# --------------------------------------------------------------------------------------------------------------- cull, costs

def hits_rect(splats, x0, y0):
    """splat_hits_rect of csrc/blend.hip restated at fp32 (no fused operations, a division for the reciprocal): which records
    pass the cull of the quadrant at pixel origin (x0, y0).  For counting classes, not for bits."""
    a = splats.astype(F32)
    with np.errstate(all="ignore"):
        dx0, dy0 = F32(x0) - a[:, 0], F32(y0) - a[:, 1]
        dx1, dy1 = dx0 + F32(7), dy0 + F32(7)
        med = lambda lo, v, hi: np.maximum(np.minimum(v, np.maximum(lo, hi)), np.minimum(lo, hi))
        nx, ny = med(dx0, F32(0), dx1), med(dy0, F32(0), dy1)
        cb2 = a[:, 3] + a[:, 3]
        ya = med(dy0, a[:, 7] * nx, dy1)
        qa = nx * (a[:, 2] * nx + cb2 * ya) + a[:, 4] * ya * ya
        xb = med(dx0, -a[:, 3] * ny / a[:, 2], dx1)
        qb = ny * (a[:, 4] * ny + cb2 * xb) + a[:, 2] * xb * xb
        return ~((qa > a[:, 6]) & (qb > a[:, 6]))


def expected_costs(fr, r64):
    """With cull_thr = +inf: tile_cost_out[t] = the most entries a quadrant of t walks — whole chunks of 64 until every pixel of
    the quadrant has terminated or lies outside the image, as forward_walk breaks — and bwd_cost_out[4 t + q] = the
    quadrant's highest n_contrib."""
    tile_cost, bwd = np.zeros(fr.T, np.int64), np.zeros(4 * fr.T, np.int64)
    for t, tl in enumerate(r64["tiles"]):
        for q in range(4):
            m = tl["quad"] == q
            alive_from = np.where(tl["inside"][m], np.where(tl["term"][m] >= 0, tl["term"][m], tl["n"]), -1)   # pixel lives through entry
            walked = 0
            for base in range(0, tl["n"], 64):
                if not (alive_from >= base).any():                             # every pixel terminated by an entry < base
                    break
                walked += min(64, tl["n"] - base)
            tile_cost[t] = max(tile_cost[t], walked)
            bwd[4 * t + q] = tl["last"][m & tl["inside"]].max() if (m & tl["inside"]).any() else 0
    return tile_cost, bwd


# ------------------------------------------------------------------------------------------------------------------ coverage

def coverage(fr, r64):
    """Counts of the edge classes in one frame, over in-image pixels only (so every count is of an in-image quadrant)."""
    c = {}
    bump = lambda k, v=1: c.__setitem__(k, c.get(k, 0) + int(v))
    a_min, a_max, eps = float(A_MIN), float(A_MAX), float(T_EPS)
    near = lambda v, thr, side: (v >= thr) & (v <= thr * (1 + 2 * REL)) if side > 0 else (v < thr) & (v >= thr * (1 - 2 * REL))
    for t, tl in enumerate(r64["tiles"]):
        n, ins = tl["n"], tl["inside"]
        bump(f"n={n}")
        if n == 0:
            continue
        ids = tl["ids"]
        sp = fr.splats[ids]
        contrib, quad = tl["contrib"], tl["quad"]
        maxlast = {}
        for q in range(4):
            m = (quad == q) & ins
            if not m.any():
                continue
            cq = contrib[m]
            blended = cq.any(0)
            pos = np.nonzero(blended)[0]
            bump(f"blended_entries={len(pos)}")
            last = tl["last"][m]
            maxlast[q] = int(last.max())
            if len(pos):
                bump("hit:first", pos[0] == 0)
                bump("hit:last", pos[-1] == n - 1)
                bump("hit:pos%64=63", ((pos % 64) == 63).sum())
                bump("hit:pos%64=0", (((pos % 64) == 0) & (pos > 0)).sum())
                chunks = set((pos // 64).tolist())
                bump("chunk_without_hit", any(k not in chunks for k in range(max(chunks))))
                x0, y0 = 16 * (t % fr.gx) + 8 * (q & 1), 16 * (t // fr.gx) + 8 * (q >> 1)
                passes = hits_rect(sp, x0, y0)
                walked = np.arange(n) < maxlast[q]
                bump("passes_cull_blends_nowhere", (passes & ~blended & walked).sum())
                for k in range(max(chunks)):
                    sl = slice(64 * k, 64 * k + 64)
                    bump("chunk_passes_cull_no_blend", passes[sl].any() and not blended[sl].any())
            lc = set(((last[last > 0] - 1) // 64).tolist())
            bump("last_in_3_chunks", len(lc) >= 3)
            bump("last_beyond_next_chunk", len(lc) >= 2 and max(lc) - min(lc) >= 2)          # first_j < -1 without the clamp
            bump("limit_in_chunk0_n_reaches_chunk2", 0 < maxlast[q] <= 64 and n > 128)
            term = tl["term"][m]
            whole = (term >= 0).all()
            if whole:
                bump("quadrant_terminated", 1)
                c.setdefault("_terminated", []).append((t, q, int(term.max())))
            # alpha decisions of live pixels
            oG, tge0 = tl["oG"][m], tl["tge0"][m]
            live = (np.arange(n)[None, :] <= np.where(term >= 0, term, n)[:, None])
            for side, nm in ((+1, "+"), (-1, "-")):
                bump(f"alpha_min{nm}", (near(oG, a_min, side) & tge0 & live).sum())
                bump(f"alpha_max{nm}", (near(oG, a_max, side) & tge0 & live).sum())
                tt = tl["T_before"][m] * (1 - tl["alpha"][m])
                asked = live & tge0 & (tl["alpha"][m] >= a_min)
                bump(f"t_eps{nm}", (near(tt, eps, side) & asked).sum())
            bump("t<0_where_alpha_passes", (~tge0 & (oG >= a_min) & live).sum())
            opq = sp[:, 5][None, :] * np.ones_like(oG)
            bump("opacity=0", ((opq == 0) & live & (oG == 0)).any())
            bump("opacity=1/255_blended", ((opq == A_MIN) & cq).sum())
            bump("opacity=1_blended", ((opq == 1) & cq).sum())
            tpix = term[term >= 0]
            bump("terminated_by_second_clamped", ((term >= 0) & (cq.sum(1) == 1) & (np.abs(tl["T_before"][m][np.arange(m.sum()), np.maximum(term, 0)]
                                                                                         - (1 - a_max)) < 1e-12)).sum())
            bump("terminates_on_chunk_last", ((tpix % 64) == 63).sum())
            bump("terminates_on_chunk_first", (((tpix % 64) == 0) & (tpix > 0)).sum())
            # quadrant cull: centre outside the quadrant's pixel rectangle (or on its border), blended pixels = one corner / one edge line
            lx, ly = (np.nonzero(m)[0] % 16) % 8, (np.nonzero(m)[0] // 16) % 8
            for j in pos:
                tag = fr.tags[ids[j]]
                if not str(tag).startswith("cull:"):
                    continue
                bx, by = lx[cq[:, j]], ly[cq[:, j]]
                just_above = (oG[cq[:, j], j].min() <= a_min * (1 + 2 * REL))
                _, where, kind = str(tag).split(":")
                if where.startswith("corner"):
                    ok = len(bx) == 1 and (int(bx[0]), int(by[0])) == (int(where[6]), int(where[7]))
                else:
                    line = {"edge_top": by == 0, "edge_bottom": by == 7, "edge_left": bx == 0, "edge_right": bx == 7}[where]
                    ok = len(bx) == 8 and bool(line.all())
                bump(f"{where}", ok and just_above)
                bump(f"cullkind:{kind}", ok and just_above)
        if len(set(maxlast.values())) > 1:
            bump("siblings_with_different_limits")
        for (tt_, q, at) in [x for x in c.get("_terminated", []) if x[0] == t]:
            bump("terminated_quadrant_with_sibling_walking_on", any(v > at + 1 for k, v in maxlast.items() if k != q))
    c.pop("_terminated", None)
    b = r64["blended_in"]
    bump("id_in_four_quadrants_of_a_tile", (b.sum(2) == 4).any(1).sum())
    bump("id_in_every_tile", (b.any(2).all(1)).sum() if fr.T > 1 else 0)
    in_lists = np.zeros((fr.P, fr.T), bool)
    for t in range(fr.T):
        in_lists[fr.tile_ids(t), t] = True
    bump("id_in_lists_of_two_tiles", (in_lists.sum(1) == 2).sum())
    bump("bg_nonzero", (fr.bg != 0).any())
    bump("upstream_both_signs", (fr.dL_dcolor > 0).any() and (fr.dL_dcolor < 0).any())
    bump("color_upstream_zero_depth_only", not fr.dL_dcolor.any() and not fr.dL_dalpha.any() and fr.dL_ddepth.any())
    bump("color_upstream_zero_alpha_only", not fr.dL_dcolor.any() and not fr.dL_ddepth.any() and fr.dL_dalpha.any())
    return c


REQUIRED = tuple(f"n={n}" for n in (0, 1, 2, 63, 64, 65, 127, 128, 129, 200)) + \
    tuple(f"blended_entries={k}" for k in (1, 2, 3, 4, 5, 7, 8, 9)) + \
    ("hit:first", "hit:last", "hit:pos%64=63", "hit:pos%64=0", "chunk_without_hit", "passes_cull_blends_nowhere",
     "chunk_passes_cull_no_blend", "last_in_3_chunks", "last_beyond_next_chunk", "limit_in_chunk0_n_reaches_chunk2",
     "siblings_with_different_limits", "quadrant_terminated", "terminated_quadrant_with_sibling_walking_on",
     "alpha_min+", "alpha_min-", "alpha_max+", "alpha_max-", "t<0_where_alpha_passes", "opacity=0", "opacity=1/255_blended",
     "opacity=1_blended", "terminated_by_second_clamped", "t_eps+", "t_eps-", "terminates_on_chunk_last", "terminates_on_chunk_first",
     "corner00", "corner70", "corner07", "corner77", "edge_top", "edge_bottom", "edge_left", "edge_right",
     "cullkind:iso", "cullkind:aniso", "cullkind:neardeg+", "cullkind:neardeg-", "cullkind:tiny_ca", "cullkind:onborder", "cullkind:half",
     "id_in_four_quadrants_of_a_tile", "id_in_every_tile", "id_in_lists_of_two_tiles", "bg_nonzero", "upstream_both_signs",
     "color_upstream_zero_depth_only", "color_upstream_zero_alpha_only")


# ------------------------------------------------------------------------------------------------------- the two staged calls

def run_staged(fr, cull=True, order="identity", depth=True, alpha=True, clear="memset", prefill=None, costs=False, order_seed=0,
               start=None):
    """lib.scg_blend_forward and lib.scg_blend_backward on the frame's buffers, pointers passed the way the binding passes them.
    Every output starts as NaN (n_contrib: -1), so an element the kernels leave unwritten shows.
      depth / alpha   True: the frame's upstream; None: a NULL pointer; "zero": a zero tensor
      clear           "memset": prezeroed = 0 on a NaN-filled record buffer; "forward": the buffer is handed to the forward as
                      dsplats_zero, then prezeroed = 1; "prefill": prezeroed = 1 on a buffer holding `prefill` (P, 16)
      costs           hand tile_cost_out (zeroed: the forward takes a maximum) and bwd_cost_out (all ones) to the frame
      start           None, or a fill of tests/guarded_alloc.py: every buffer the two calls write or add into (the five images,
                      the gradient records unless prefilled, bwd_cost_out) starts from that fill's bytes instead of NaN / -1 —
                      what torch.empty hands the binding.  tile_cost_out stays zeroed: that is its contract
    Returns numpy arrays.  (Imports torch and the package here: the references above need neither.)"""
    import torch
    from scgaussian_amd import _lib
    from scgaussian_amd import rasterizer as R
    check_frame(fr)
    lib = _lib.load()
    dev = torch.device("cuda", torch.cuda.current_device())
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    H, W, P = fr.H, fr.W, fr.P
    words = fr.ranges_words(order, order_seed)
    assert len(words) == lib.scg_ranges_words(W, H)
    splats, plist, ranges = up(fr.splats_for(cull)), up(fr.point_list.view(np.int32)), up(words.view(np.int32))
    st = R.GaussianRasterizationSettings(H, W, 1.0, 1.0, up(fr.bg), 1.0, torch.eye(4, device=dev), torch.eye(4, device=dev), 0,
                                         torch.zeros(3, device=dev), False, False)
    frame_ = R._frame_for(st, P, 0, dev)
    nan = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float32, device=dev)
    color, dimg, aimg, final_T = nan(3, H, W), nan(1, H, W), nan(1, H, W), nan(H, W)
    n_contrib = torch.full((H, W), -1, dtype=torch.int32, device=dev)
    dsplats = nan(P, 16) if prefill is None else up(prefill.astype(F32))
    assert (clear == "prefill") == (prefill is not None)
    tile_cost = torch.zeros(fr.T, dtype=torch.int32, device=dev) if costs else None
    bwd_cost = torch.full((4 * fr.T,), -1, dtype=torch.int32, device=dev) if costs else None
    if start is not None:
        import guarded_alloc
        for t in (color, dimg, aimg, final_T, n_contrib, bwd_cost) + (() if prefill is not None else (dsplats,)):
            if t is not None:
                guarded_alloc.poison_(t, start)
    pick = lambda sel, a: None if sel is None else (torch.zeros(H, W, dtype=torch.float32, device=dev) if sel == "zero" else up(a))
    dC, dD, dA = up(fr.dL_dcolor), pick(depth, fr.dL_ddepth), pick(alpha, fr.dL_dalpha)
    c = frame_.c
    saved = (c.tile_cost_in, c.tile_cost_out, c.bwd_cost_in, c.bwd_cost_out, c.long_lists_out, c.num_rendered_out)
    try:
        c.tile_cost_in = c.bwd_cost_in = c.long_lists_out = c.num_rendered_out = None
        c.tile_cost_out, c.bwd_cost_out = R.ptr(tile_cost), R.ptr(bwd_cost)
        stream = R._stream(dev)
        R.check(lib.scg_blend_forward(frame_.ref, R.ptr(ranges), R.ptr(plist), R.ptr(splats), R.ptr(color), R.ptr(dimg), R.ptr(aimg),
                                      R.ptr(final_T), R.ptr(n_contrib), R.ptr(dsplats) if clear == "forward" else None, stream),
                "scg_blend_forward")
        R.check(lib.scg_blend_backward(frame_.ref, R.ptr(ranges), R.ptr(plist), R.ptr(splats), R.ptr(final_T), R.ptr(n_contrib),
                                       R.ptr(dC), R.ptr(dD), R.ptr(dA), R.ptr(dsplats), 0 if clear == "memset" else 1, stream),
                "scg_blend_backward")
        try:
            torch.cuda.synchronize()
        except RuntimeError as e:                     # a GPU fault: nothing more is started on the card by this session
            import pytest
            pytest.exit(f"GPU fault in the staged blend calls on frame {fr.name}: {e}", returncode=3)
    finally:
        (c.tile_cost_in, c.tile_cost_out, c.bwd_cost_in, c.bwd_cost_out, c.long_lists_out, c.num_rendered_out) = saved
    out = dict(color=color, depth=dimg[0], alpha=aimg[0], final_T=final_T, n_contrib=n_contrib, dsplats=dsplats)
    if costs:
        out.update(tile_cost=tile_cost, bwd_cost=bwd_cost)
    return {k: v.cpu().numpy() for k, v in out.items()}


FORWARD_OUTPUTS = ("color", "depth", "alpha", "final_T", "n_contrib")
# what tests/test_gpu_parity.py runs under the compiler-written twin of the blend kernels as well; the records of the second
# group are compared bit for bit (tests/test_blend_refs_cpu.py asserts that they are single-atomic frames)
TWIN_FRAMES = ("b", "d", "e", "e9", "translation-d", "phase-1", "phase-2")
TWIN_SINGLE_ATOMIC = ("b", "translation-d", "phase-1", "phase-2")

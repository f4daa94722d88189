"""TEST INFRASTRUCTURE ONLY — the rule of csrc/geocheck.hip restated in numpy float64 (include/scg_geocheck.h states it), the scenes
its tests share, and the oracle's view of the same scenes: votes and the pixels that sit on a threshold.

Two references, two jobs.  oracle/geo_check_oracle.py walks lift -> move -> project step by step, as the reference does; the kernel
multiplies matrices composed once per pair.  The two agree to rounding, so a pixel whose round trip lands ON a threshold may vote
differently: `near_ties` marks those pixels from the oracle's own numbers and the scene tests leave them out.  `geocheck_ref` below
repeats the kernel's arithmetic operation by operation (explicit adjugate inverses, products summed in the kernel's order, no fused
multiply-add anywhere: scalar Python floats for the matrices, elementwise numpy for the pixels), so planted pixels and odd shapes are
held to it exactly.  One difference to the oracle is the header's, not an accident: the oracle forms `rel` in fp32 (numpy keeps
float32 - float32 in float32) and the kernel in fp64 on the same fp32 values; 1e-9 apart, far inside the near-tie window of 1e-5."""
import math
import os

import numpy as np

from oracle import geo_check_oracle as orc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_model.npz")
SELF_DIST = 1e3
NEAR_DIST, NEAR_DEPTH = 1e-3, 1e-5          # the near-tie windows around dist_thresh (px) and depth_thresh


# ---- the matrices of a pair, in the kernel's operation order ---------------------------------------------------------------------
def inv3(a):
    with np.errstate(all="ignore"):
        a = [np.float64(x) for x in np.asarray(a, dtype=np.float64).reshape(-1)]
        c00, c01, c02 = a[4] * a[8] - a[5] * a[7], a[5] * a[6] - a[3] * a[8], a[3] * a[7] - a[4] * a[6]
        det = a[0] * c00 + a[1] * c01 + a[2] * c02
        r = np.float64(1.0) / det
        b = [c00 * r, (a[2] * a[7] - a[1] * a[8]) * r, (a[1] * a[5] - a[2] * a[4]) * r,
             c01 * r, (a[0] * a[8] - a[2] * a[6]) * r, (a[2] * a[3] - a[0] * a[5]) * r,
             c02 * r, (a[1] * a[6] - a[0] * a[7]) * r, (a[0] * a[4] - a[1] * a[3]) * r]
    return np.array(b, dtype=np.float64).reshape(3, 3)


def inv4(a):
    with np.errstate(all="ignore"):
        a = [np.float64(x) for x in np.asarray(a, dtype=np.float64).reshape(-1)]
        s0, s1, s2 = a[0] * a[5] - a[4] * a[1], a[0] * a[6] - a[4] * a[2], a[0] * a[7] - a[4] * a[3]
        s3, s4, s5 = a[1] * a[6] - a[5] * a[2], a[1] * a[7] - a[5] * a[3], a[2] * a[7] - a[6] * a[3]
        c5, c4, c3 = a[10] * a[15] - a[14] * a[11], a[9] * a[15] - a[13] * a[11], a[9] * a[14] - a[13] * a[10]
        c2, c1, c0 = a[8] * a[15] - a[12] * a[11], a[8] * a[14] - a[12] * a[10], a[8] * a[13] - a[12] * a[9]
        det = s0 * c5 - s1 * c4 + s2 * c3 + s3 * c2 - s4 * c1 + s5 * c0
        r = np.float64(1.0) / det
        b = [(a[5] * c5 - a[6] * c4 + a[7] * c3) * r, (a[2] * c4 - a[1] * c5 - a[3] * c3) * r,
             (a[13] * s5 - a[14] * s4 + a[15] * s3) * r, (a[10] * s4 - a[9] * s5 - a[11] * s3) * r,
             (a[6] * c2 - a[4] * c5 - a[7] * c1) * r, (a[0] * c5 - a[2] * c2 + a[3] * c1) * r,
             (a[14] * s2 - a[12] * s5 - a[15] * s1) * r, (a[8] * s5 - a[10] * s2 + a[11] * s1) * r,
             (a[4] * c4 - a[5] * c2 + a[7] * c0) * r, (a[1] * c2 - a[0] * c4 - a[3] * c0) * r,
             (a[12] * s4 - a[13] * s2 + a[15] * s0) * r, (a[9] * s2 - a[8] * s4 - a[11] * s0) * r,
             (a[5] * c1 - a[4] * c3 - a[6] * c0) * r, (a[0] * c3 - a[1] * c1 + a[2] * c0) * r,
             (a[13] * s1 - a[12] * s3 - a[14] * s0) * r, (a[8] * s3 - a[9] * s1 + a[10] * s0) * r]
    return np.array(b, dtype=np.float64).reshape(4, 4)


def matmul(a, b):
    """c = a b, every element summed over k in rising order, one rounding per operation (numpy's `@` may fuse)."""
    n = a.shape[0]
    c = np.zeros((n, n), dtype=np.float64)
    with np.errstate(all="ignore"):
        for r in range(n):
            for q in range(n):
                s = a[r, 0] * b[0, q]
                for k in range(1, n):
                    s = s + a[r, k] * b[k, q]
                c[r, q] = s
    return c


def pair_table(exts, num_src):
    """(N, J) int32, J = min(num_src, N): distance, NaN last, equal distances by index; the self-distance is 1e3."""
    exts = np.asarray(exts, dtype=np.float64)
    n = exts.shape[0]
    J = min(num_src, n)
    out = np.zeros((n, J), dtype=np.int32)
    for i in range(n):
        keys = []
        for c in range(n):
            dx, dy, dz = (exts[i, 0, 3] - exts[c, 0, 3], exts[i, 1, 3] - exts[c, 1, 3], exts[i, 2, 3] - exts[c, 2, 3])
            with np.errstate(all="ignore"):
                d = SELF_DIST if c == i else float(np.sqrt(dx * dx + dy * dy + dz * dz))
            keys.append((math.isnan(d), 0.0 if math.isnan(d) else d, c))
        out[i] = [k[2] for k in sorted(keys)[:J]]
    return out


def compose(intrs, exts, num_src):
    """The workspace of scg_geocheck_setup: pairs (N,J), and per (view, slot) M1 (3,3), t1 (3), M2 (3,3), t2 (3)."""
    intrs, exts = np.asarray(intrs, dtype=np.float64), np.asarray(exts, dtype=np.float64)
    pairs = pair_table(exts, num_src)
    n, J = pairs.shape
    Kinv, Einv = [inv3(k) for k in intrs], [inv4(e) for e in exts]
    M1, t1, M2, t2 = np.zeros((n, J, 3, 3)), np.zeros((n, J, 3)), np.zeros((n, J, 3, 3)), np.zeros((n, J, 3))
    with np.errstate(all="ignore"):
        for i in range(n):
            for s in range(J):
                j = int(pairs[i, s])
                A, B = matmul(exts[j], Einv[i]), matmul(exts[i], Einv[j])
                M1[i, s] = matmul(matmul(intrs[j], A[:3, :3].copy()), Kinv[i])
                for r in range(3):
                    t1[i, s, r] = intrs[j, r, 0] * A[0, 3] + intrs[j, r, 1] * A[1, 3] + intrs[j, r, 2] * A[2, 3]
                M2[i, s] = matmul(B[:3, :3].copy(), Kinv[j])
                t2[i, s] = B[:3, 3]
    return pairs, M1, t1, M2, t2


def sample_zero_border(img, xs32, ys32):
    """oracle.bilinear_zero_border with the kernel's guard: a floor that does not fit an int32 is outside (never cast)."""
    H, W = img.shape
    xs, ys = xs32.astype(np.float64), ys32.astype(np.float64)
    with np.errstate(all="ignore"):
        good = np.isfinite(xs) & np.isfinite(ys) & (np.abs(np.floor(xs)) < 2.0 ** 31) & (np.abs(np.floor(ys)) < 2.0 ** 31)
    xs, ys = np.where(good, xs, -5.0), np.where(good, ys, -5.0)
    x0, y0 = np.floor(xs).astype(np.int64), np.floor(ys).astype(np.int64)
    wx1, wy1 = xs - x0, ys - y0
    acc = np.zeros(xs.shape, dtype=np.float64)
    with np.errstate(all="ignore"):
        for oy, wy in ((0, 1.0 - wy1), (1, wy1)):
            for ox, wx in ((0, 1.0 - wx1), (1, wx1)):
                xi, yi = x0 + ox, y0 + oy
                ok = (xi >= 0) & (xi < W) & (yi >= 0) & (yi < H)
                acc = acc + np.where(ok, img[np.clip(yi, 0, H - 1), np.clip(xi, 0, W - 1)].astype(np.float64), 0.0) * wx * wy
        return acc.astype(np.float32)


def geocheck_ref(intrs, exts, depths, dist_thresh=1.0, depth_thresh=0.01, view_thresh=5, num_src=15):
    """What scg_geocheck_setup + scg_geocheck compute: (votes uint8, masks fp32, filtered fp32, pairs int32)."""
    intrs = np.asarray(intrs, dtype=np.float64)
    depths = np.asarray(depths, dtype=np.float32)
    n, H, W = depths.shape
    pairs, M1, t1, M2, t2 = compose(intrs, exts, num_src)
    v, u = np.divmod(np.arange(H * W), W)
    u, v = u.astype(np.float64), v.astype(np.float64)
    votes_all = np.zeros((n, H, W), dtype=np.uint8)
    masks = np.zeros((n, H, W), dtype=np.float32)
    filtered = np.zeros((n, H, W), dtype=np.float32)
    with np.errstate(all="ignore"):
        for i in range(n):
            d = depths[i].reshape(-1).astype(np.float64)
            ud, vd = u * d, v * d
            K = intrs[i]
            votes, total = np.zeros(H * W, dtype=np.int32), np.zeros(H * W, dtype=np.float64)
            for s in range(pairs.shape[1]):
                m, t = M1[i, s], t1[i, s]
                k0 = m[0, 0] * ud + m[0, 1] * vd + m[0, 2] * d + t[0]
                k1 = m[1, 0] * ud + m[1, 1] * vd + m[1, 2] * d + t[1]
                k2 = m[2, 0] * ud + m[2, 1] * vd + m[2, 2] * d + t[2]
                xs, ys = k0 / k2, k1 / k2
                smp = sample_zero_border(depths[pairs[i, s]], xs.astype(np.float32), ys.astype(np.float32)).astype(np.float64)
                a, b = xs * smp, ys * smp
                m, t = M2[i, s], t2[i, s]
                X0 = m[0, 0] * a + m[0, 1] * b + m[0, 2] * smp + t[0]
                X1 = m[1, 0] * a + m[1, 1] * b + m[1, 2] * smp + t[1]
                X2 = m[2, 0] * a + m[2, 1] * b + m[2, 2] * smp + t[2]
                d_back = X2.astype(np.float32).astype(np.float64)
                h0 = K[0, 0] * X0 + K[0, 1] * X1 + K[0, 2] * X2
                h1 = K[1, 0] * X0 + K[1, 1] * X1 + K[1, 2] * X2
                h2 = K[2, 0] * X0 + K[2, 1] * X1 + K[2, 2] * X2
                ub, vb = (h0 / h2).astype(np.float32).astype(np.float64), (h1 / h2).astype(np.float32).astype(np.float64)
                moved = np.hypot(ub - u, vb - v)
                rel = np.abs(d_back - d) / d
                agree = (moved < dist_thresh) & (rel < depth_thresh)
                votes += agree
                total = total + np.where(agree, d_back, 0.0)
            mask = (votes > view_thresh).astype(np.float32)
            mean = ((total + d) / (votes + 1).astype(np.float64)).astype(np.float32)
            votes_all[i], masks[i], filtered[i] = votes.reshape(H, W), mask.reshape(H, W), (mean * mask).reshape(H, W)
    return votes_all, masks, filtered, pairs


# ---- the oracle's view: votes, depth, and the pixels on a threshold -------------------------------------------------------------
def oracle_votes(intrs, exts, depths, dist_thresh=1.0, depth_thresh=0.01, view_thresh=5, num_src=15):
    """oracle.geocheck's loop, statement by statement, with what it does not return: (votes int32, kept depth fp64, mask fp32,
    near) — near marks a pixel when, for any of its sources, `moved` lies within NEAR_DIST of dist_thresh or `rel` within
    NEAR_DEPTH of depth_thresh."""
    n, H, W = depths.shape
    neighbours = orc.get_pairs(exts, num_src)
    gu, gv = np.meshgrid(np.arange(W), np.arange(H))
    votes_all = np.zeros((n, H, W), dtype=np.int32)
    kept_depth = np.zeros((n, H, W), dtype=np.float64)
    kept_mask = np.zeros((n, H, W), dtype=np.float32)
    near = np.zeros((n, H, W), dtype=bool)
    for i in range(n):
        votes = np.zeros((H, W), dtype=np.int32)
        depth_sum = np.zeros((H, W), dtype=np.float64)
        for j in neighbours[i]:
            d_back, u_back, v_back, _, _ = orc.reproject_with_depth(depths[i], intrs[i], exts[i], depths[j], intrs[j], exts[j])
            with np.errstate(divide="ignore", invalid="ignore"):
                moved = np.hypot(u_back - gu, v_back - gv)
                rel = np.abs(d_back - depths[i]) / depths[i]
                near[i] |= (np.abs(moved - dist_thresh) <= NEAR_DIST) | (np.abs(rel.astype(np.float64) - depth_thresh) <= NEAR_DEPTH)
            agree = (moved < dist_thresh) & (rel < depth_thresh)
            votes += agree
            depth_sum += np.where(agree, d_back, 0.0)
        keep = votes > view_thresh
        votes_all[i], kept_mask[i] = votes, keep
        with np.errstate(all="ignore"):
            kept_depth[i] = (depth_sum + depths[i]) / (votes + 1) * keep
    return votes_all, kept_depth, kept_mask, near


def near_ties(intrs, exts, depths, dist_thresh=1.0, depth_thresh=0.01, num_src=15):
    return oracle_votes(intrs, exts, depths, dist_thresh, depth_thresh, 0, num_src)[3]


def ulps32(got, want):
    """|got - want| in units of the fp32 spacing at `want` (fp64); pixels where both are NaN or both the same infinity count 0."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    with np.errstate(all="ignore"):
        same = (np.isnan(got) & np.isnan(want)) | (got == want)
        unit = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
        return np.where(same, 0.0, np.abs(got - want) / unit)


# ---- the scenes of the CPU and the GPU tests -------------------------------------------------------------------------------------
def scene(name):
    """(intrs, exts, depths, kwargs of the check).  `fixture`: recorded from the reference's own geocheck (ref_model.npz geo_*);
    the others come from the generator of tests/test_geo_check.py; `wide` asks for more sources than it has views, so every view
    is one of its own sources."""
    if name == "fixture":
        ref = np.load(GOLDEN)
        return ref["geo_intrs"], ref["geo_exts"], ref["geo_depths"], dict(view_thresh=3, num_src=15)
    from test_geo_check import _scene
    n, H, W, seed, num_src = {"arc": (8, 20, 28, 0, 5), "small": (6, 24, 32, 1, 4), "wide": (4, 9, 70, 2, 15)}[name]
    intrs, exts, depths, _ = _scene(n=n, H=H, W=W, seed=seed)
    return intrs, exts, depths, dict(view_thresh=2, num_src=num_src)


SCENES = ("fixture", "arc", "small", "wide")
_CACHE = {}


def scene_refs(name):
    """Everything the tests need of a scene, computed once per process: inputs, the restatement's outputs, the oracle's."""
    if name not in _CACHE:
        intrs, exts, depths, kw = scene(name)
        r_votes, r_masks, r_filtered, r_pairs = geocheck_ref(intrs, exts, depths, **kw)
        o_votes, o_depth, o_mask, near = oracle_votes(intrs, exts, depths, **kw)
        _CACHE[name] = dict(intrs=intrs, exts=exts, depths=depths, kw=kw, r_votes=r_votes, r_masks=r_masks, r_filtered=r_filtered,
                            r_pairs=r_pairs, o_votes=o_votes, o_depth=o_depth, o_mask=o_mask, near=near)
    return _CACHE[name]


def planted_cameras(which):
    """The cameras of the pair-table tests: (N,4,4) fp64 with identity rotations."""
    if which == "tie":            # three cameras at x = -1, 0, +1: the middle one has two sources at distance exactly 1
        xs = [(-1.0, 0, 0), (0.0, 0, 0), (1.0, 0, 0)]
    elif which == "beyond":       # camera 3 is farther than 1e3 from everybody: it sorts behind the view itself
        xs = [(0.0, 0, 0), (0.5, 0.25, 0), (1.5, 0, 0.125), (0.0, 2000.0, 0)]
    else:
        raise KeyError(which)
    exts = np.repeat(np.eye(4)[None], len(xs), 0)
    exts[:, :3, 3] = np.array(xs)
    return exts

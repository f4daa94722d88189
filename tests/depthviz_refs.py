"""numpy restatement of the depth colour map's rule (include/scg_viz.h, rules 1-7 of the feature's description): what
np.percentile (numpy >= 2, float32 input, method 'linear'), matplotlib's Normalize, Colormap.__call__ and the truncating byte casts
compute, written as separately rounded fp32 operations.  tests/test_depthviz_cpu.py holds it against those libraries; the GPU tests
hold the kernels against it bit for bit."""
import os

import numpy as np

f32 = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_depthviz.npz")


def ranks(n, p=98.0):
    """(lo, hi, g) of n values at percentile p: they depend on n and p alone."""
    assert 1 <= n <= 1 << 24
    q = f32(p) / f32(100)
    pos = f32(n - 1) * q
    lo = int(np.floor(pos))
    return lo, min(lo + 1, n - 1), f32(pos - f32(lo))


def normalised(depth):
    """render.py:143: two subtractions and one division, each rounded in fp32; max == min gives NaN."""
    d = np.asarray(depth, dtype=f32)
    with np.errstate(all="ignore"):
        return ((d - d.min()) / (d.max() - d.min())).astype(f32)


def stats(x, p=98.0):
    """(vmin, vmax, a, b) as fp32 scalars.  np.sort puts NaNs last and -0.0 beside +0.0 in either order: zeros compare by value."""
    s = np.sort(np.asarray(x, dtype=f32).reshape(-1))
    lo, hi, g = ranks(s.size, p)
    a, b = s[lo], s[hi]
    with np.errstate(all="ignore"):
        d = f32(b - a)
        vmax = f32(a + f32(d * g)) if g < 0.5 else f32(b - f32(d * f32(f32(1) - g)))
    vmin = s[0]
    if np.isnan(s[-1]):
        vmin = vmax = f32(np.nan)
    return f32(vmin), f32(vmax), f32(a), f32(b)


def index(x, vmin, vmax):
    """(index 0..255, bad) per pixel: rules 4 and 5.  Normalize keeps vmin and vmax as Python floats, so numpy forms vmax - vmin
    in fp64 and divides the fp32 difference x - vmin by it in fp64, rounding the quotient to fp32 once.  Where vmax - vmin is exact
    in fp32 (vmin = 0: every normalised depth) that is the fp32 division."""
    x = np.asarray(x, dtype=f32)
    vmin, vmax = f32(vmin), f32(vmax)
    if vmin == vmax:
        return np.zeros(x.shape, np.int64), np.zeros(x.shape, bool)
    with np.errstate(all="ignore"):
        t = ((x - vmin).astype(f32).astype(np.float64) / (np.float64(vmax) - np.float64(vmin))).astype(f32)
        s = (t * f32(256)).astype(f32)
    bad = np.isnan(t)
    idx = np.where(s < 0, 0, np.where(s >= 256, 255, np.trunc(np.where(bad, 0, np.clip(s, 0, 255))))).astype(np.int64)
    return idx, bad


def colorize(x, lut, p=98.0, st=None):
    """visualization(x) with the 256x3 uint8 table `lut`: (H,W,3) uint8, R, G, B."""
    vmin, vmax = (stats(x, p) if st is None else st)[:2]
    idx, bad = index(x, vmin, vmax)
    out = np.asarray(lut, dtype=np.uint8)[idx]
    out[bad] = 0
    return out


def video_frame(render):
    """render_video.py:132,148: (clamp(render, 0, 1) * 255.).astype(uint8)[..., ::-1] of a (3,H,W) fp32 image, NaN -> 0."""
    r = np.asarray(render, dtype=f32)
    with np.errstate(all="ignore"):
        v = (np.clip(r, f32(0), f32(1)) * f32(255)).astype(f32)        # np.clip keeps a NaN, as torch.clamp does
    v = np.where(np.isnan(v), f32(0), v)
    return np.ascontiguousarray(np.trunc(v).astype(np.uint8).transpose(1, 2, 0)[..., ::-1])


def quantise(x):
    """torchvision.utils.save_image's quantiser (include/scg_eval.h); q(NaN) = 0."""
    x = np.asarray(x, dtype=f32)
    with np.errstate(all="ignore"):
        v = ((x * f32(255)).astype(f32) + f32(0.5)).astype(f32)
    v = np.where(np.isnan(v), f32(0), np.clip(v, 0, 255))
    return np.trunc(v).astype(np.uint8)


def render_u8(render):
    r = np.asarray(render, dtype=f32)
    return np.ascontiguousarray(quantise(np.clip(r, f32(0), f32(1))).transpose(1, 2, 0))


def same_stats(got, want):
    """bit for bit, except that a zero is compared by value and a NaN equals a NaN"""
    got, want = np.asarray(got, dtype=f32), np.asarray(want, dtype=f32)
    for g, w in zip(got.reshape(-1), want.reshape(-1)):
        if np.isnan(w) or w == 0:
            ok = (np.isnan(g) and np.isnan(w)) or (g == w and not np.isnan(w))
        else:
            ok = g.view(np.uint32) == w.view(np.uint32)
        if not ok:
            return False
    return True


def key_of(x):
    """the kernel's order-preserving 32-bit key of fp32 values (NaN-free input)"""
    b = np.asarray(x, dtype=f32).view(np.uint32)
    return np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def value_of(k):
    k = np.asarray(k, dtype=np.uint32)
    return np.where(k & np.uint32(0x80000000), k & np.uint32(0x7FFFFFFF), ~k).astype(np.uint32).view(f32)

"""numpy restatement of the image resize (include/img/scg_resample.h, scgaussian_amd/images.py): Pillow's Image.resize(size) with
its default filter, bicubic, for 8-bit modes `L` and `RGB`, and PILtoTorch's float image.

Written from the rule, one output index at a time in plain Python floats (IEEE double, one rounding per operation, no fused
multiply-add), independently of images.axis_table, which is vectorised.  tests/test_resize_cpu.py holds it to Pillow itself; the
GPU tests compare with it bit for bit.

Each axis is resampled on its own, the horizontal one first and only if the width changes, its result rounded to bytes; the vertical
one reads those bytes and runs only if the height changes.
"""
import functools
import math

import numpy as np

PRECISION_BITS = 22
A = -0.5


def bicubic(t):
    t = abs(t)
    if t < 1.0:
        return ((A + 2.0) * t - (A + 3.0)) * t * t + 1
    if t < 2.0:
        return (((t - 5) * t + 8) * t - 4) * A
    return 0.0


def ksize_of(in_size, out_size):
    return int(math.ceil(2.0 * max(in_size / out_size, 1.0))) * 2 + 1


@functools.lru_cache(maxsize=None)
def coefficients(in_size, out_size):
    """(bounds int32 (out, 2): xmin and count; k int32 (out, ksize)), read-only."""
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = 2.0 * fs
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / fs
    bounds = np.zeros((out_size, 2), dtype=np.int32)
    k = np.zeros((out_size, ksize), dtype=np.int32)
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)                       # int(): truncation toward zero
        xmax = min(int(center + support + 0.5), in_size) - xmin
        w = [bicubic((x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        for x, v in enumerate(w):
            k[xx, x] = int(v * (1 << PRECISION_BITS) - 0.5) if v < 0 else int(v * (1 << PRECISION_BITS) + 0.5)
        bounds[xx] = (xmin, xmax)
    bounds.setflags(write=False)
    k.setflags(write=False)
    return bounds, k


def resample_axis(src, out_size, axis):
    """One pass over `axis` (0 or 1) of a uint8 (H, W, C) array: int32 accumulators, arithmetic shift, clamp."""
    src = np.moveaxis(np.asarray(src), axis, 0)
    bounds, k = coefficients(src.shape[0], out_size)
    out = np.empty((out_size,) + src.shape[1:], dtype=np.uint8)
    wide = src.astype(np.int32)
    for i in range(out_size):
        first, count = bounds[i]
        acc = np.full(src.shape[1:], 1 << (PRECISION_BITS - 1), dtype=np.int32)
        for t in range(count):
            acc = acc + wide[first + t] * k[i, t]
        out[i] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return np.moveaxis(out, 0, axis)


def horizontal(src, wout):
    """The intermediate (H, wout, C) of an (H, W, C) image: what the vertical pass reads."""
    return resample_axis(src, wout, 1)


def resize(src, size):
    """uint8 (H, W), (H, W, 1) or (H, W, 3) -> the same number of dimensions at size = (width, height)."""
    src = np.asarray(src)
    assert src.dtype == np.uint8
    img = src.reshape(src.shape[0], src.shape[1], -1)
    wout, hout = int(size[0]), int(size[1])
    if wout != img.shape[1]:
        img = horizontal(img, wout)
    if hout != img.shape[0]:
        img = resample_axis(img, hout, 0)
    return np.array(img).reshape((hout, wout) + src.shape[2:])


def float_image(u8):
    """PILtoTorch's tensor of a resized image: float32 (C, H, W), float32(byte) / 255.0f correctly rounded."""
    u8 = np.asarray(u8)
    img = u8.reshape(u8.shape[0], u8.shape[1], -1)
    return (img.astype(np.float32) / np.float32(255.0)).transpose(2, 0, 1).copy()


def resize_float_intermediate(src, size):
    """NOT the rule: both passes with the horizontal result kept in double, rounded once at the end.  The CPU test plants an image
    on which this differs from Pillow, which shows that the comparison sees the intermediate's rounding."""
    src = np.asarray(src)
    img = src.reshape(src.shape[0], src.shape[1], -1).astype(np.float64)
    wout, hout = int(size[0]), int(size[1])
    one = float(1 << PRECISION_BITS)
    for axis, out_size in ((1, wout), (0, hout)):
        img = np.moveaxis(img, axis, 0)
        if out_size != img.shape[0]:
            bounds, k = coefficients(img.shape[0], out_size)
            out = np.zeros((out_size,) + img.shape[1:])
            for i in range(out_size):
                first, count = bounds[i]
                for t in range(count):
                    out[i] += img[first + t] * (k[i, t] / one)
            img = out
        img = np.moveaxis(img, 0, axis)
    return np.clip(np.floor(img + 0.5), 0, 255).astype(np.uint8).reshape((hout, wout) + src.shape[2:])


# ---- test images ---------------------------------------------------------------------------------------------------------------
def random_image(h, w, c, seed=0):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (h, w, c) if c else (h, w), dtype=np.uint8)


def step_image(h, w, c):
    """One vertical and one horizontal 0 / 255 edge, shifted per channel: next to an edge the filter's negative lobes drive the
    accumulator below 0 on the dark side and above 255 on the bright one, at any reduction."""
    y, x = np.mgrid[0:h, 0:w]
    planes = [(((x >= w // 2 - 3 + 3 * i) ^ (y >= h // 2 + 2 * i)) * 255).astype(np.uint8) for i in range(max(c, 1))]
    return np.stack(planes, axis=2) if c else planes[0]


def checker_image(h, w, c, cell=None):
    """Cells of a third of the longer side (so they survive an 8x reduction and overshoot as the step does)."""
    cell = cell or max(2, max(h, w) // 3)
    y, x = np.mgrid[0:h, 0:w]
    planes = [((((y + i) // cell) + (x // cell)) % 2 * 255).astype(np.uint8) for i in range(max(c, 1))]
    return np.stack(planes, axis=2) if c else planes[0]

#!/usr/bin/env python3
"""What the LPIPS metric costs (profiles/r22_lpips_timing.json).  Prints ONE JSON object and writes it to --out.

One process, warm, every call synchronised on both sides, median of --calls calls per leg (the protocol of
tools/virtualwarp_timing.py), at 504 x 378 and 1600 x 1200, with the tests' weights (tests/lpips_refs.make_weights) and images.
Per size:
  torch_first_ms    the plain-torch twin on the device (lpips.lpips_torch, fp32, whatever convolution torch picks): its FIRST call
                    at this shape, which holds the library's algorithm search — part of what a user waits for
  torch_ms          the twin's median after that
  hip_ms            Lpips.__call__: 13 convolution launches, the head, the fold
  launches_ms       the same between two events
  conv_ms           the 13 convolution launches alone between two events (scg_lp_conv3x3 on preallocated channels-last buffers)
  layer_ms, layer_tflops   each of the 13 launches alone between two events, and its rate (a single short launch between two events
                    carries the events' own cost: the sum exceeds conv_ms)
  head_ms           the head and the fold alone between two events (scg_lp_head on the taps the call left)
  conv_tflops       2 * H * W * 611 712 FLOP (305 856 multiply-adds per pixel and image) / conv_ms, and its share of the 157.3 TF peak
  dev_hip, dev_torch  |value - fp64 value| of both legs; fp64 is the twin in float64 on the device
What one process of one visit shows: the medians of these calls on this machine in this state; no run-to-run spread.

    python tools/lpips_timing.py [--calls 25] [--out profiles/r22_lpips_timing.json]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import lpips_refs as LR                                                                      # noqa: E402
from scgaussian_amd import _lib, _lib_lp, lpips                                              # noqa: E402

SIZES = {"504x378": (378, 504), "1600x1200": (1200, 1600)}
DEV = "cuda"
PEAK_TF = 157.3
FLOP_PER_PIXEL_AND_IMAGE = 2 * 305856


def wall(fn, calls):
    """median wall ms of fn(), synchronised on both sides; one warm-up call first"""
    fn()
    out = []
    for _ in range(calls):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return round(statistics.median(out), 4)


def events(fn, calls):
    """median ms between two events around fn()"""
    fn()
    out = []
    for _ in range(calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return round(statistics.median(out), 4)


def conv_chain(lp, x, y):
    """The 13 layers through scg_lp_conv3x3 on buffers allocated once: a function that launches them."""
    lib = _lib_lp.load()
    _, H, W = x.shape
    pair = torch.stack([x, y]).permute(0, 2, 3, 1).contiguous()
    offs, off = [], 0
    for cin, cout in lpips.CHANNELS:
        offs.append(off)
        off += 9 * cin * cout
    boffs = []
    for _, cout in lpips.CHANNELS:
        boffs.append(off)
        off += cout
    bufs, src, h, w = [], pair, H, W
    for i, (cin, cout) in enumerate(lpips.CHANNELS):
        pool = i in lpips.POOL_BEFORE
        hi, wi = h, w
        if pool:
            h, w = h // 2, w // 2
        dst = torch.empty((2, h, w, cout), dtype=torch.float32, device=x.device)
        flags = _lib_lp.LP_RELU | (_lib_lp.LP_POOL if pool else 0) | (_lib_lp.LP_ZSCORE if i == 0 else 0)
        bufs.append((cin, cout, hi, wi, src, dst, flags))
        src = dst
    base = lp.params.data_ptr()
    stream = _lib.stream_of(x, "lpips_timing")

    def run(only=None):
        for i, (cin, cout, hi, wi, s, d, flags) in enumerate(bufs):
            if only is None or i == only:
                _lib_lp.check(lib.scg_lp_conv3x3(2, cin, cout, hi, wi, s.data_ptr(), base + 4 * offs[i], base + 4 * boffs[i],
                                                 d.data_ptr(), flags, stream), "scg_lp_conv3x3")
    return run


def one_size(H, W, calls, weights):
    x, y = (torch.from_numpy(a).to(DEV) for a in LR.make_images(H, W, seed=1))
    lp = lpips.Lpips(*weights, device=DEV)
    res = {"H": H, "W": W, "launches": 15, "scratch_bytes": int(_lib_lp.load().scg_lp_scratch_bytes(H, W))}
    twin = lambda: lpips.lpips_torch(x, y, lp.convs, lp.lins)[0]                              # noqa: E731
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    v_torch = twin()
    torch.cuda.synchronize()
    res["torch_first_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
    res["torch_ms"] = wall(twin, calls)
    res["hip_ms"] = wall(lambda: lp(x, y), calls)
    res["launches_ms"] = events(lambda: lp(x, y), calls)
    chain = conv_chain(lp, x, y)
    res["conv_ms"] = events(chain, calls)
    res["layer_ms"] = [events(lambda i=i: chain(i), calls) for i in range(len(lpips.CHANNELS))]
    res["layer_tflops"] = [round(2 * 9 * cin * cout * 2 * (H >> lv) * (W >> lv) / (ms * 1e-3) / 1e12, 1)
                           for (cin, cout), lv, ms in zip(lpips.CHANNELS, (0, 0, 1, 1, 2, 2, 2, 3, 3, 3, 4, 4, 4), res["layer_ms"])]
    lp(x, y)
    res["head_ms"] = events(lambda: lp.head(H, W), calls)
    flop = 2 * H * W * FLOP_PER_PIXEL_AND_IMAGE
    res["conv_tflops"] = round(flop / (res["conv_ms"] * 1e-3) / 1e12, 2)
    res["conv_share_of_peak"] = round(res["conv_tflops"] / PEAK_TF, 3)
    v_hip = lp(x, y)
    res["value_hip"], res["value_torch"] = float(v_hip), float(v_torch)
    try:
        v64 = float(lpips.lpips_torch(x.double(), y.double(), lp.convs, lp.lins)[0])
        res["value_fp64"] = v64
        res["dev_hip"], res["dev_torch"] = abs(float(v_hip) - v64), abs(float(v_torch) - v64)
    except Exception as e:                                                                   # no fp64 convolution at this size
        res["value_fp64"] = None
        res["fp64_error"] = f"{type(e).__name__}: {e}"[:200]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=25)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r22_lpips_timing.json"))
    ap.add_argument("--sizes", default=",".join(SIZES))
    args = ap.parse_args()
    weights = LR.make_weights()
    res = {"tool": "tools/lpips_timing.py", "device": torch.cuda.get_device_name(0), "calls": args.calls,
           "weights": f"tests/lpips_refs.make_weights(seed={LR.WEIGHT_SEED})", "sizes": {}}
    for name in args.sizes.split(","):
        res["sizes"][name] = one_size(*SIZES[name], args.calls, weights)
        torch.cuda.empty_cache()
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()

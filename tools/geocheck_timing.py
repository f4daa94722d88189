#!/usr/bin/env python3
"""What the cross-view depth consistency check costs (profiles/r14_geocheck_timing.json).  Prints ONE JSON object and writes it to
--out.

One process, warm, every call synchronised on both sides, median of --calls calls per leg (the protocol of tools/eval_timing.py), on
cameras along an arc in front of a slanted plane with 4 % outliers, at two sizes:
  3x1600x1200    the reference's 3-view DTU case at DTU's native size; num_src = 15 > 3, so every view is also its own source
  49x400x300     a full DTU scan at a quarter of the size, 15 sources per view
Per size:
  twin           geo_check.geocheck on the device with fp64 matrices (what the tests pass): torch tensor code, a few dozen
                 operators per view
  hip_setup      GeoCheck.setup: the pair table and the composed matrices, one launch
  hip_run        GeoCheck.run: every pixel of every view, one launch
  hip_one_shot   geo_check.geocheck_hip: allocation, setup and run
  hip_run_device the run alone between two events around `calls` back-to-back launches: the kernel without the host's share
and what the two paths computed: the share of masks that differ and the largest depth deviation where they agree.

    python tools/geocheck_timing.py [--calls 25] [--out profiles/r14_geocheck_timing.json]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from scgaussian_amd import geo_check as gc                                                   # noqa: E402

SIZES = {"3x1600x1200": (3, 1200, 1600), "49x400x300": (49, 300, 400)}
NUM_SRC = 15
DEV = "cuda"


def scene(n, H, W, seed=0):
    """Cameras on an arc looking at a slanted plane, about a pixel of disparity between neighbours; depth maps rendered
    analytically, 4 % of the pixels corrupted (the generator of tests/test_geo_check.py at any size)."""
    rng = np.random.default_rng(seed)
    f = 1.1 * W
    K = np.array([[f, 0, W / 2], [0, f, H / 2], [0, 0, 1.0]])
    exts = np.zeros((n, 4, 4))
    depths = np.zeros((n, H, W), dtype=np.float32)
    nrm, d0 = np.array([0.1, -0.05, 1.0]), 6.0
    ys, xs = np.mgrid[0:H, 0:W]
    rays = np.linalg.inv(K) @ np.stack([xs.ravel(), ys.ravel(), np.ones(H * W)])
    for i in range(n):
        ang = 0.0004 * (i - n / 2)
        R = np.array([[np.cos(ang), 0, np.sin(ang)], [0, 1, 0], [-np.sin(ang), 0, np.cos(ang)]])
        t = np.array([(6.0 / f) * (i - n / 2) + 1e-4 * i * i, 0.3 * (6.0 / f) * i, 0.0])
        exts[i] = np.eye(4)
        exts[i, :3, :3], exts[i, :3, 3] = R, t
        depths[i] = ((d0 + nrm @ (R.T @ t)) / (nrm @ (R.T @ rays))).reshape(H, W)
    bad = rng.random(depths.shape) < 0.04
    depths[bad] *= rng.uniform(1.05, 1.6, size=int(bad.sum())).astype(np.float32)
    return np.repeat(K[None], n, 0), exts, depths


def median_ms(fn, calls, warm=3):
    times = []
    for it in range(warm + calls):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if it >= warm:
            times.append((time.perf_counter() - t0) * 1e3)
    return round(statistics.median(times), 4), round(min(times), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=25)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r14_geocheck_timing.json"))
    a = ap.parse_args()
    assert a.calls >= 20
    res = {"device": torch.cuda.get_device_name(0), "calls": a.calls, "num_src": NUM_SRC,
           "what": "median ms per call, one process, warm, synchronised around each call; hip_run_device: events around the calls"}
    for tag, (n, H, W) in SIZES.items():
        intrs, exts, depths = (torch.from_numpy(x).to(DEV) for x in scene(n, H, W))
        kw = dict(view_thresh=min(5, n - 1), num_src=NUM_SRC)
        chk = gc.GeoCheck(n, H, W, num_src=NUM_SRC, device=DEV).setup(intrs, exts)
        run_kw = dict(view_thresh=kw["view_thresh"])
        for leg, fn in (("twin", lambda: gc.geocheck(intrs, exts, depths, **kw)),
                        ("hip_setup", lambda: chk.setup(intrs, exts)),
                        ("hip_run", lambda: chk.run(depths, **run_kw)),
                        ("hip_one_shot", lambda: gc.geocheck_hip(intrs, exts, depths, **kw))):
            res[f"{tag}_{leg}_ms"], res[f"{tag}_{leg}_min_ms"] = median_ms(fn, a.calls)
        begin, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        begin.record()
        for _ in range(a.calls):
            chk.run(depths, **run_kw)
        end.record()
        torch.cuda.synchronize()
        dev_ms = begin.elapsed_time(end) / a.calls
        res[f"{tag}_hip_run_device_ms"] = round(dev_ms, 4)
        res[f"{tag}_pixel_source_pairs_per_us"] = round(n * H * W * chk.J / (dev_ms * 1e3), 1)
        res[f"{tag}_speedup_run"] = round(res[f"{tag}_twin_ms"] / res[f"{tag}_hip_run_ms"], 2)
        res[f"{tag}_speedup_setup_and_run"] = round(res[f"{tag}_twin_ms"] / (res[f"{tag}_hip_setup_ms"] + res[f"{tag}_hip_run_ms"]), 2)
        # what the two paths computed
        td, tm = gc.geocheck(intrs, exts, depths, **kw)
        hd, hm = chk.run(depths, **run_kw)
        same = tm == hm
        res[f"{tag}_masks_kept_share"] = round(hm.mean().item(), 4)
        res[f"{tag}_masks_differ_share"] = round(1.0 - same.float().mean().item(), 6)
        keep = same & (hm > 0)
        res[f"{tag}_depth_max_rel_diff"] = float(((hd - td).abs() / td.abs())[keep].max().item()) if keep.any() else None
    text = json.dumps(res)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text + "\n")


if __name__ == "__main__":
    main()

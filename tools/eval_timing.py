#!/usr/bin/env python3
"""What the evaluation of a test view costs (profiles/r13_eval_timing.json).  Prints ONE JSON object and writes it to --out.

One process, warm, every call synchronised on both sides, median of --calls calls per leg (the protocol of tools/dtu_timing.py), at
1600 x 1200 (DTU's native size) and 400 x 300.  Per size, one view under a DTU mask:
  torch_restatement   the arithmetic of render.py:143-156 + metrics.py:36-44, :87-89 in plain torch on the GPU (tests/eval_refs.py
                      view_torch): normalised depth, get_pixel_loss, five quantised images copied to the host one by one, the
                      pixels uploaded again, masked images, 11x11 SSIM and PSNR read as python numbers
  hip_view            evaluate.evaluate_view: at most six launches, no host read (the synchronisation around the call is the
                      protocol's)
and a set of ten such views:
  hip_set_of_10       evaluate.EvalSet: ten add() calls and the set's single read in results()
PNG encoding and the file system are in neither leg.

    python tools/eval_timing.py [--calls 25] [--out profiles/r13_eval_timing.json]"""
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
import eval_refs as ER                                                                       # noqa: E402
from scgaussian_amd import evaluate                                                          # noqa: E402

SIZES = {"1600x1200": (1200, 1600), "400x300": (300, 400)}
DEV = "cuda"
SET_VIEWS = 10


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r13_eval_timing.json"))
    a = ap.parse_args()
    assert a.calls >= 20
    res = {"device": torch.cuda.get_device_name(0), "calls": a.calls,
           "what": "median ms per call, one process, warm, synchronised around each call; one view under a mask, and a set of 10"}
    for tag, (H, W) in SIZES.items():
        render, gt, depth = (t.to(DEV) for t in ER.images(H, W, seed=0, spread=0.05))
        y, x = torch.meshgrid(torch.linspace(-1, 1, H), torch.linspace(-1, 1, W), indexing="ij")
        dtumask = (((x / 0.6) ** 2 + (y / 0.75) ** 2) < 1).float().to(DEV)[None]

        def hip_set():
            es = evaluate.EvalSet(SET_VIEWS)
            for i in range(SET_VIEWS):
                es.add(f"{i:05d}.png", render, gt, depth, dtumask)
            return es.results()
        for leg, fn in (("torch_restatement", lambda: ER.view_torch(render, gt, depth, dtumask)),
                        ("hip_view", lambda: evaluate.evaluate_view(render, gt, depth, dtumask)),
                        ("hip_set_of_10", hip_set)):
            res[f"{tag}_{leg}_ms"], res[f"{tag}_{leg}_min_ms"] = median_ms(fn, a.calls)
        res[f"{tag}_view_speedup"] = round(res[f"{tag}_torch_restatement_ms"] / res[f"{tag}_hip_view_ms"], 2)
        res[f"{tag}_set_per_view_ms"] = round(res[f"{tag}_hip_set_of_10_ms"] / SET_VIEWS, 4)
        # what the two legs computed
        ssim, psnr = ER.view_torch(render, gt, depth, dtumask)
        full, _ = hip_set()
        res[f"{tag}_psnr"], res[f"{tag}_ssim"] = round(full["PSNR"], 4), round(full["SSIM"], 6)
        res[f"{tag}_psnr_torch"], res[f"{tag}_ssim_torch"] = round(psnr, 4), round(ssim, 6)
    text = json.dumps(res)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text + "\n")


if __name__ == "__main__":
    main()

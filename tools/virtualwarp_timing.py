#!/usr/bin/env python3
"""What the virtual-view warp loss and the depth smoothness cost (profiles/r21_virtualwarp_timing.json).  Prints ONE JSON object and
writes it to --out.

One process, warm, every call synchronised on both sides, median of --calls calls per leg (the protocol of tools/ply_timing.py), at
504 x 378 and 1008 x 756 with 3 views.  Each leg is forward plus backward of  warp_loss + smooth_loss(depth, guide=image)  on
leaves that require gradients.  Per size:
  torch_ms         the plain-torch restatement on the device (virtual.warp_loss_torch, virtual.smooth_loss_torch), fp32
  hip_ms           VirtualWarp.loss + virtual.smooth_loss: 3 + 2 launches forward, 1 + 1 backward, plus autograd's own
  launches_ms      the same between two events
  warp_*/smooth_*  each loss alone
What one process of one visit shows: the medians of these calls on this machine in this state; no run-to-run spread.

    python tools/virtualwarp_timing.py [--calls 25] [--out profiles/r21_virtualwarp_timing.json]"""
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
import virtualwarp_refs as VR                                                                # noqa: E402
from scgaussian_amd import virtual                                                           # noqa: E402

SIZES = {"504x378": (378, 504), "1008x756": (756, 1008)}
NV = 3
DEV = "cuda"


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


def one_size(H, W, calls):
    sc = VR.make_scene(H, W, NV, seed=1)
    t = VR.tensors(sc, device=DEV)
    warp = virtual.VirtualWarp(t["intrs"], t["w2cs"], t["img_colors"])
    warp.set_pose(sc["vir_c2w"])
    img, depth, mask = t["virtual_img"].requires_grad_(True), t["virtual_depth"].requires_grad_(True), t["vir_mask"]

    def leg(warp_fn, smooth_fn):
        def run():
            img.grad = depth.grad = None
            loss = 0
            if warp_fn is not None:
                loss = loss + warp_fn()
            if smooth_fn is not None:
                loss = loss + smooth_fn()
            loss.backward()
            return loss
        return run
    hip_w = lambda: warp.loss(img, depth, mask)                                              # noqa: E731
    hip_s = lambda: virtual.smooth_loss(depth, img.detach())                                 # noqa: E731
    tor_w = lambda: virtual.warp_loss_torch(img, depth, mask, warp.colors, warp.records)[0]  # noqa: E731
    tor_s = lambda: virtual.smooth_loss_torch(depth, img.detach())                           # noqa: E731
    res = {"H": H, "W": W, "views": NV, "launches_forward": 5, "launches_backward": 2}
    res["torch_ms"] = wall(leg(tor_w, tor_s), calls)
    res["hip_ms"] = wall(leg(hip_w, hip_s), calls)
    res["torch_launches_ms"] = events(leg(tor_w, tor_s), calls)
    res["launches_ms"] = events(leg(hip_w, hip_s), calls)
    res["warp_torch_ms"], res["warp_hip_ms"] = wall(leg(tor_w, None), calls), wall(leg(hip_w, None), calls)
    res["warp_launches_ms"] = events(leg(hip_w, None), calls)
    res["smooth_torch_ms"], res["smooth_hip_ms"] = wall(leg(None, tor_s), calls), wall(leg(None, hip_s), calls)
    res["smooth_launches_ms"] = events(leg(None, hip_s), calls)
    a, b = leg(hip_w, hip_s)(), leg(tor_w, tor_s)()
    res["loss_hip"], res["loss_torch"] = float(a), float(b)
    res["scratch_bytes"] = int(warp.scratch.numel() * 4)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=25)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r21_virtualwarp_timing.json"))
    ap.add_argument("--sizes", default=",".join(SIZES))
    args = ap.parse_args()
    res = {"tool": "tools/virtualwarp_timing.py", "device": torch.cuda.get_device_name(0), "calls": args.calls, "sizes": {}}
    for name in args.sizes.split(","):
        res["sizes"][name] = one_size(*SIZES[name], args.calls)
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()

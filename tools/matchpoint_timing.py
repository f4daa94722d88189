#!/usr/bin/env python3
"""What the init stage's snapshot costs (profiles/r20_matchpoint_timing.json).  Prints ONE JSON object and writes it to --out.

One process, warm, every call synchronised on both sides, median of --calls calls per leg (the protocol of tools/ply_timing.py), at
3 views and at 7 views of 504 x 378 with 2 000 matches per ordered pair.  No file is encoded in either leg.  Per size:
  torch_loop_ms    the plain-torch restatement of the reference's loop on the device: per pair the position, the depth and the
                   index_put; per view the copy np.save needs, min / max / normalise and the copy save_image needs with its
                   mul(255).add(0.5).clamp(0, 255).to(uint8); at the end the two concatenations, their copies and the host cast of
                   colour * 255
  hip_ms           matchpoint.pack + to_host: four launches and the ONE device-to-host copy
  ... split:       launches_ms   the four launches between two events
                   copy_ms       MatchpointSnapshot.to_host alone, with the bytes it moves
What one process of one visit shows: the medians of these calls on this machine in this state; no run-to-run spread.

    python tools/matchpoint_timing.py [--calls 25] [--out profiles/r20_matchpoint_timing.json]"""
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
import matchpoint_refs as MR                                                                 # noqa: E402
from scgaussian_amd import matchpoint                                                        # noqa: E402

H, W, M = 378, 504, 2000
SIZES = {"3_views": 3, "7_views": 7}
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


def torch_loop(view_gs):
    """scene/gaussian_model.py:611-642 restated: the same operations on the device, the same copies, no file."""
    xyzs, colors, planes, images = [], [], [], []
    for _key, vgs in view_gs.items():
        sparse = torch.zeros(vgs["height"], vgs["width"], device=DEV)
        for _b, v in vgs["match_infos"].items():
            xyzs.append(v["rays_o"] + v["rays_d"] * v["z_val"])
            colors.append(v["color"])
            uv = v["uv"]
            depth = v["z_val"].squeeze(-1) * v["cam_rays_d"][:, 2]
            sparse[(uv[:, 1].clamp(0, vgs["height"] - 1).to(torch.int64), uv[:, 0].clamp(0, vgs["width"] - 1).to(torch.int64))] = depth
        planes.append(sparse.cpu().numpy())                                                   # np.save's copy
        n = (sparse - sparse.min()) / (sparse.max() - sparse.min())
        images.append(n.mul(255).add_(0.5).clamp_(0, 255).to("cpu", torch.uint8).numpy())     # save_image's
    xyz, rgb = torch.cat(xyzs).cpu().numpy(), torch.cat(colors).cpu().numpy() * 255
    return xyz, rgb.astype(np.uint8), planes, images


def one_size(V, calls):
    segs = V * (V - 1)
    arena = MR.random_arena([M] * segs, [s // (V - 1) for s in range(segs)], [(H, W)] * V, seed=V)
    view_gs = MR.view_gs_of(arena, DEV)
    inputs = matchpoint.MatchpointInputs.from_view_gs(view_gs)
    res = {"views": V, "pairs": segs, "matches": inputs.N, "H": H, "W": W}
    res["torch_loop_ms"] = wall(lambda: torch_loop(view_gs), calls)
    res["hip_ms"] = wall(lambda: matchpoint.pack(inputs).to_host(), calls)
    res["launches_ms"] = events(lambda: matchpoint.pack(inputs), calls)

    def copy():
        snap = matchpoint.pack(inputs)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        snap.to_host()
        return (time.perf_counter() - t0) * 1e3, snap
    copy()
    res["copy_ms"] = round(statistics.median(copy()[0] for _ in range(calls)), 4)
    snap = copy()[1]
    res["copy_bytes"] = int(snap.layout.total)
    res["copy_GBs"] = round(snap.layout.total / (res["copy_ms"] * 1e-3) / 1e9, 2)
    res["bytes_per_pixel"] = round(snap.layout.total / (V * H * W), 3)
    # the two legs hold the same planes (the byte planes too wherever no pixel is hit twice within a pair's index_put)
    _xyz, _rgb, planes, _images = torch_loop(view_gs)
    got = snap.host_views()[1]
    res["planes_equal_pixels"] = float(np.mean([np.mean(a == b) for a, b in zip(planes, got)]))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=25)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r20_matchpoint_timing.json"))
    ap.add_argument("--sizes", default=",".join(SIZES))
    args = ap.parse_args()
    res = {"tool": "tools/matchpoint_timing.py", "device": torch.cuda.get_device_name(0), "calls": args.calls, "sizes": {}}
    for name in args.sizes.split(","):
        res["sizes"][name] = one_size(SIZES[name], args.calls)
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()

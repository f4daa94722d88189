#!/usr/bin/env python3
"""What writing the result images costs, on the host with Pillow and on the GPU (profiles/r23_png_timing.json).  Prints ONE JSON
object and writes it to --out.

One process, warm, every call synchronised on both sides, median of --calls calls per leg (the protocol of tools/lpips_timing.py);
files go to a memory-backed directory (/dev/shm when it exists), so no disk is in any leg.  Sizes 1600 x 1200 and 400 x 300; image
kinds, all uint8 device tensors as render_set and render_video hold them:
  render       a rendered synthetic scene, (H,W,3)
  depth_gray   its normalised depth, (H,W), written as three equal channels
  mask         the dark-run mask of dtu.background_mask on that render, 0 / 255, (H,W), written as three equal channels
  turbo        the turbo colour map of the depth, (H,W,3)
Per size and kind:
  pillow_ms        the parent's route: .cpu(), then evaluate._save_png (Pillow, compress level 6)
  device_ms        png.save_png: the three launches, the two reads, CRC-32 and the write
  launches_ms      the three launches between two events
  reads_ms         PackedPngs.to_host(): the table, then `total` bytes into pinned memory
  crc_write_ms     PackedPngs.write(): zlib.crc32 over the copied bytes and the file
  pillow_bytes, device_bytes   the two files' sizes; both decode to the same pixels (checked here)
Per size, video: render_video over --frames views of one size without files, with Pillow's files and with the device's (one timed
call each after a warm one; the files of the two routes are compared pixel for pixel on the first frame).
What one process of one visit shows: the medians of these calls on this machine in this state; no run-to-run spread.

    python tools/png_timing.py [--calls 25] [--frames 60] [--out profiles/r23_png_timing.json]"""
import argparse
import json
import os
import shutil
import statistics
import sys
import tempfile
import time
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from scgaussian_amd import dtu, evaluate, png, video                                         # noqa: E402
from scgaussian_amd import render as rmod                                                    # noqa: E402
from scgaussian_amd import synthetic as syn                                                  # noqa: E402

SIZES = {"1600x1200": (1200, 1600), "400x300": (300, 400)}
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


def scene(H, W, frames):
    sc = syn.make_scene(20000, W, H, seed=5)
    model = syn.make_raw_model(sc).to(DEV)
    model.active_sh_degree = 3
    bg = torch.zeros(3, device=DEV)
    views = [types.SimpleNamespace(**syn.orbit_camera(W, H, -12.0 + 24.0 * i / max(frames - 1, 1), -2.0, 7.0).to(DEV)._asdict())
             for i in range(frames)]
    return views, model, rmod.PipelineParams(), bg


def decode(path):
    from PIL import Image
    return np.asarray(Image.open(path))


def kinds_of(views, model, pipe, bg):
    """The four device tensors of one frame."""
    with torch.no_grad():
        pkg = rmod.render(views[0], model, pipe, bg)
        out = video.render_video(views[:1], model, pipe, bg, render=lambda *_a: pkg)
        mask, _gt, _count = dtu.background_mask(pkg["render"].contiguous())
    return {"render": torch.from_numpy(out["renders"][0]).to(DEV), "depth_gray": torch.from_numpy(out["depth"][0]).to(DEV),
            "mask": (mask[0].to(torch.uint8) * 255).contiguous(), "turbo": torch.from_numpy(out["depth_color"][0]).to(DEV)}


def image_legs(t, folder, calls):
    a, b = os.path.join(folder, "pillow.png"), os.path.join(folder, "device.png")
    res = {"pillow_ms": wall(lambda: evaluate._save_png(a, t.cpu().numpy()), calls),
           "device_ms": wall(lambda: png.save_png(b, t), calls)}
    plan = png.PngPlan([t.shape], t.device, own_inputs=False)
    res["launches_ms"] = events(lambda: plan.encode([t]), calls)
    res["reads_ms"] = wall(lambda: plan.encode([t]).to_host(), calls)                      # (holds the launches: subtract them)
    res["reads_ms"] = round(res["reads_ms"] - wall(lambda: plan.encode([t]), calls), 4)
    packed = plan.encode([t]).to_host()
    res["crc_write_ms"] = wall(lambda: packed.write([b]), calls)
    res["pillow_bytes"], res["device_bytes"] = os.path.getsize(a), os.path.getsize(b)
    res["kinds"] = {("dynamic", "stored")[k]: int((plan.chunk_info()[:, 1] == k).sum()) for k in (0, 1)}
    if not np.array_equal(decode(a), decode(b)):
        raise SystemExit("the two routes' files decode to different pixels")
    return res


def video_legs(views, model, pipe, bg, folder):
    def run(route):
        kw = {} if route is None else {"out_dir": os.path.join(folder, route), "png": route}
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        video.render_video(views, model, pipe, bg, **kw)
        torch.cuda.synchronize()
        return round((time.perf_counter() - t0) * 1e3, 2)
    video.render_video(views[:2], model, pipe, bg, out_dir=os.path.join(folder, "warm"), png="device")       # warm both routes
    video.render_video(views[:2], model, pipe, bg, out_dir=os.path.join(folder, "warm"))
    res = {"frames": len(views), "no_files_ms": run(None), "device_ms": run("device"), "pillow_ms": run("pillow")}
    for sub, name in (("renders", "00000.png"), ("depth", "00000.png"), ("depth", "color_00000.png")):
        pa, pb = (os.path.join(folder, r, "video", "ours_0", sub, name) for r in ("pillow", "device"))
        if not np.array_equal(decode(pa), decode(pb)):
            raise SystemExit(f"{sub}/{name}: the two routes' files decode to different pixels")
    for r in ("pillow", "device"):
        base = os.path.join(folder, r, "video", "ours_0")
        res[r + "_bytes"] = sum(os.path.getsize(os.path.join(d, n)) for d, _s, names in os.walk(base) for n in names)
    res["device_over_no_files"] = round(res["device_ms"] / res["no_files_ms"], 2)
    res["pillow_over_no_files"] = round(res["pillow_ms"] / res["no_files_ms"], 2)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=25)
    ap.add_argument("--frames", type=int, default=60)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r23_png_timing.json"))
    args = ap.parse_args()
    folder = tempfile.mkdtemp(prefix="scg_png_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    res = {"device": torch.cuda.get_device_name(0), "calls": args.calls, "memory_backed": folder.startswith("/dev/shm"), "sizes": {}}
    try:
        for name, (H, W) in SIZES.items():
            views, model, pipe, bg = scene(H, W, args.frames)
            row = {k: image_legs(t, folder, args.calls) for k, t in kinds_of(views, model, pipe, bg).items()}
            row["video"] = video_legs(views, model, pipe, bg, folder)
            res["sizes"][name] = row
            print(name, json.dumps(row), file=sys.stderr, flush=True)
    finally:
        shutil.rmtree(folder, ignore_errors=True)
    text = json.dumps(res, indent=1)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()

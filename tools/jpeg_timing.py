#!/usr/bin/env python3
"""What writing JPEG files and the two Motion-JPEG videos costs, on the host with Pillow and on the GPU
(profiles/r24_jpeg_timing.json).  Prints ONE JSON object and writes it to --out.

One process, warm, every call synchronised on both sides, median of --calls calls per leg (the protocol of tools/png_timing.py);
files go to a memory-backed directory (/dev/shm when it exists), so no disk is in any leg.  Sizes 1600 x 1200 and 400 x 300; image
kinds, both uint8 B, G, R device tensors as render_video holds them:
  frame        a rendered synthetic scene, frames_bgr[0]
  turbo        the turbo colour map of its depth, depth_frames_bgr[0]
Per size and kind, quality 90 at 4:2:0:
  pillow_ms        the parent's only route: .cpu(), then Pillow save(format="JPEG", quality=90, subsampling=2, restart_marker_rows=1)
  device_ms        jpeg.save_jpeg: the three launches, the two reads and the write
  launches_ms      the three launches between two events
  reads_ms         PackedJpegs.to_host(): the table, then `total` bytes into pinned memory
  write_ms         PackedJpegs.write()
  bytes, same_bytes   the file's size; whether the two routes' files are the same bytes
Per size, video: render_video over --frames views without files, with its PNG tree alone (png="device"), with the tree and
video="mjpeg", and with the tree and the Pillow route (the returned host frames through Pillow into jpeg.write_avi); one timed call
each after a warm one; videos_*_ms is a leg minus the tree's; same_bytes compares the two routes' .avi files.
What one process of one visit shows: the medians of these calls on this machine in this state; no run-to-run spread.

    python tools/jpeg_timing.py [--calls 25] [--frames 60] [--out profiles/r24_jpeg_timing.json]"""
import argparse
import io
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
from scgaussian_amd import jpeg, video                                                       # noqa: E402
from scgaussian_amd import render as rmod                                                    # noqa: E402
from scgaussian_amd import synthetic as syn                                                  # noqa: E402

SIZES = {"1600x1200": (1200, 1600), "400x300": (300, 400)}
DEV = "cuda"
QUALITY, SUB = 90, "4:2:0"


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


def pillow_file(bgr: np.ndarray) -> bytes:
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(bgr[:, :, ::-1])).save(b, format="JPEG", quality=QUALITY, subsampling=2, optimize=False,
                                                                restart_marker_rows=1)
    return b.getvalue()


def image_legs(t, folder, calls):
    a, b = os.path.join(folder, "pillow.jpg"), os.path.join(folder, "device.jpg")

    def pillow():
        with open(a, "wb") as fh:
            fh.write(pillow_file(t.cpu().numpy()))
    res = {"pillow_ms": wall(pillow, calls), "device_ms": wall(lambda: jpeg.save_jpeg(b, t, QUALITY, SUB, bgr=True), calls)}
    plan = jpeg.JpegPlan([t.shape], t.device, QUALITY, SUB, bgr=True, own_inputs=False)
    res["launches_ms"] = events(lambda: plan.encode([t]), calls)
    res["reads_ms"] = wall(lambda: plan.encode([t]).to_host(), calls)                      # (holds the launches: subtract them)
    res["reads_ms"] = round(res["reads_ms"] - wall(lambda: plan.encode([t]), calls), 4)
    packed = plan.encode([t]).to_host()
    res["write_ms"] = wall(lambda: packed.write([b]), calls)
    res["bytes"] = os.path.getsize(b)
    res["same_bytes"] = open(a, "rb").read() == open(b, "rb").read()
    return res


def video_legs(views, model, pipe, bg, folder):
    H, W = int(views[0].image_height), int(views[0].image_width)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return round((time.perf_counter() - t0) * 1e3, 2)

    def pillow_route(vs, out_dir):
        out = video.render_video(vs, model, pipe, bg, out_dir=out_dir, png="device")
        base = os.path.join(out_dir, "video", "ours_0")
        os.makedirs(base, exist_ok=True)
        jpeg.write_avi(os.path.join(base, "render_video.avi"), [pillow_file(f) for f in out["frames_bgr"]], 30, W, H)
        jpeg.write_avi(os.path.join(base, "depth_video.avi"), [pillow_file(f) for f in out["depth_frames_bgr"]], 30, W, H)

    warm = os.path.join(folder, "warm")
    video.render_video(views[:2], model, pipe, bg, out_dir=warm, video="mjpeg", png="device")
    pillow_route(views[:2], warm)
    shutil.rmtree(warm, ignore_errors=True)
    # render_video writes its PNG tree whenever it has an out_dir: every file leg writes it by the device route (png="device"), so
    # that the legs differ by the two videos alone
    res = {"frames": len(views),
           "no_files_ms": timed(lambda: video.render_video(views, model, pipe, bg)),
           "png_tree_ms": timed(lambda: video.render_video(views, model, pipe, bg, out_dir=os.path.join(folder, "tree"), png="device")),
           "mjpeg_ms": timed(lambda: video.render_video(views, model, pipe, bg, out_dir=os.path.join(folder, "device"), png="device",
                                                        video="mjpeg", jpeg_quality=QUALITY, jpeg_subsampling=SUB)),
           "pillow_ms": timed(lambda: pillow_route(views, os.path.join(folder, "pillow")))}
    same = True
    for name in ("render_video.avi", "depth_video.avi"):
        pa, pb = (os.path.join(folder, r, "video", "ours_0", name) for r in ("pillow", "device"))
        same = same and open(pa, "rb").read() == open(pb, "rb").read()
        res[name + "_bytes"] = os.path.getsize(pb)
    res["same_bytes"] = same
    res["videos_mjpeg_ms"] = round(res["mjpeg_ms"] - res["png_tree_ms"], 2)
    res["videos_pillow_ms"] = round(res["pillow_ms"] - res["png_tree_ms"], 2)
    res["mjpeg_over_no_files"] = round(res["mjpeg_ms"] / res["no_files_ms"], 2)
    res["pillow_over_no_files"] = round(res["pillow_ms"] / res["no_files_ms"], 2)
    for r in ("tree", "device", "pillow"):
        shutil.rmtree(os.path.join(folder, r), ignore_errors=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=25)
    ap.add_argument("--frames", type=int, default=60)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r24_jpeg_timing.json"))
    args = ap.parse_args()
    folder = tempfile.mkdtemp(prefix="scg_jpg_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    res = {"device": torch.cuda.get_device_name(0), "calls": args.calls, "quality": QUALITY, "subsampling": SUB,
           "memory_backed": folder.startswith("/dev/shm"), "sizes": {}}
    try:
        for name, (H, W) in SIZES.items():
            views, model, pipe, bg = scene(H, W, args.frames)
            with torch.no_grad():
                out = video.render_video(views[:1], model, pipe, bg)
            kinds = {"frame": torch.from_numpy(out["frames_bgr"][0].copy()).to(DEV),
                     "turbo": torch.from_numpy(out["depth_frames_bgr"][0].copy()).to(DEV)}
            row = {k: image_legs(t, folder, args.calls) for k, t in kinds.items()}
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

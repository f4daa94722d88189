#!/usr/bin/env python3
"""What downsizing a camera image costs (profiles/r19_resize_timing.json).  Prints ONE JSON object and writes it to --out.

One process, warm, every call synchronised on both sides, median of --calls calls per leg (the protocol of tools/ply_timing.py), one
random RGB image per size: 4032 x 3024 -> 504 x 378 (LLFF, -r 8), -> 1008 x 756 (-r 4), 1600 x 1200 -> 400 x 300 (DTU).  Per size:
  baseline_ms               the reference's route on this machine's host: PILtoTorch(img, res) (utils/general_utils.py:22-28, stated
                            below) followed by .to("cuda"); pillow_resize_ms is its resize alone
  hip_call_ms               images.pil_to_torch(img, res) as a whole; pil_to_array_ms is the np.asarray(img) inside it (Pillow packs its
                            4-byte pixels into 3-byte ones on the host) and hip_from_array_ms the call from that array on
  ... split:                staging_ms      the copy of the image bytes and the tables into the pinned buffer
                            upload_ms       the one host-to-device copy of that buffer
                            launches_ms     both launches between two events, from a device source
                            vertical_ms     the vertical launch alone between two events, on a tight (hin, wout) intermediate (the
                                            real one differs only in its padded pitch); horizontal_ms_derived = launches - vertical
                            source_read     the source bytes over launches_ms against the project's measured copy ceiling (6.29 TB/s)
  batch20_ms                images.resize_batch of 20 such images (chunks of at most 256 MB staged)
  decode_ms                 Pillow's decode of a JPEG of the same size from a memory-backed directory: NOT part of the resize, and
                            reported so that nobody takes the resize for the whole load
  same_bytes                the kernels' bytes equal Pillow's, for the single call and for the batch
What one process of one visit shows: the medians of these calls on this machine in this state; no run-to-run spread.

    python tools/resize_timing.py [--calls 25] [--out profiles/r19_resize_timing.json]"""
import argparse
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

import numpy as np
import torch
import PIL
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from scgaussian_amd import images                                                            # noqa: E402

SIZES = {"llff_r8": ((4032, 3024), (504, 378)), "llff_r4": ((4032, 3024), (1008, 756)), "dtu_r4": ((1600, 1200), (400, 300))}
DEV = "cuda"
COPY_CEILING_GBS = 6290.0
BATCH = 20


def pil_to_torch_host(pil_image, resolution):
    """PILtoTorch as the reference computes it."""
    resized = torch.from_numpy(np.array(pil_image.resize(resolution))) / 255.0
    return resized.permute(2, 0, 1) if len(resized.shape) == 3 else resized.unsqueeze(dim=-1).permute(2, 0, 1)


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
    print(f"  leg done: {statistics.median(out):.3f} ms", file=sys.stderr, flush=True)
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


def one_size(in_size, out_size, folder, calls):
    (W, H), (w, h) = in_size, out_size
    rng = np.random.default_rng(W + h)
    arr = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    img = Image.fromarray(arr)
    plan = images.plan_of(in_size, out_size, 3)
    res = {"in": list(in_size), "out": list(out_size), "hksize": plan.hksize, "vksize": plan.vksize,
           "source_bytes": plan.image_bytes, "tables_bytes": int(plan.tables.size)}
    fl0 = torch.empty((3, h, w), dtype=torch.float32, device=DEV)
    res["baseline_ms"] = wall(lambda: pil_to_torch_host(img, out_size).to(DEV), calls)
    res["pillow_resize_ms"] = wall(lambda: img.resize(out_size), calls)
    res["hip_call_ms"] = wall(lambda: images.pil_to_torch(img, out_size), calls)
    res["pil_to_array_ms"] = wall(lambda: np.asarray(img), calls)
    res["hip_from_array_ms"] = wall(lambda: images.resize_u8(arr, out_size, out_float=fl0), calls)

    staged = torch.empty(plan.staged_bytes(1), dtype=torch.uint8, pin_memory=True)
    view = staged.numpy()

    def stage():
        view[:plan.image_bytes] = arr.reshape(-1)
        view[plan.tables_offset(1):] = plan.tables
    res["staging_ms"] = wall(stage, calls)
    res["upload_ms"] = wall(lambda: staged.to(DEV, non_blocking=True), calls)
    res["upload_GBs"] = round(staged.numel() / (res["upload_ms"] * 1e-3) / 1e9, 2)

    dev_src = torch.from_numpy(arr).to(DEV)
    out = torch.empty((h, w, 3), dtype=torch.uint8, device=DEV)
    fl = torch.empty((3, h, w), dtype=torch.float32, device=DEV)
    res["launches_ms"] = events(lambda: images.resize_u8(dev_src, out_size, out=out, out_float=fl), calls)
    mid = images.resize_u8(dev_src, (w, H))
    res["vertical_ms"] = events(lambda: images.resize_u8(mid, out_size, out=out, out_float=fl), calls)
    res["horizontal_ms_derived"] = round(res["launches_ms"] - res["vertical_ms"], 4)
    gbs = plan.image_bytes / (res["launches_ms"] * 1e-3) / 1e9
    res["source_read"] = {"GBs": round(gbs, 1), "of_copy_ceiling": round(gbs / COPY_CEILING_GBS, 4)}

    want = np.asarray(img.resize(out_size))
    batch = [arr] * BATCH
    res["batch20_ms"] = wall(lambda: images.resize_batch(batch, out_size, want_float=True), max(3, calls // 5))
    got_batch = images.resize_batch(batch, out_size).cpu().numpy()
    res["same_bytes"] = {"single": bool(np.array_equal(out.cpu().numpy(), want)),
                         "batch": bool(all(np.array_equal(g, want) for g in got_batch)),
                         "float": bool(torch.equal(images.pil_to_torch(img, out_size).cpu(), pil_to_torch_host(img, out_size).contiguous()))}

    path = os.path.join(folder, f"{W}x{H}.jpg")
    smooth = Image.fromarray(arr[::16, ::16]).resize(in_size)                             # a photograph-like image: noise does not compress
    smooth.save(path, quality=92)
    res["jpeg_bytes"] = os.path.getsize(path)

    def decode():
        with Image.open(path) as im:
            im.load()
    res["decode_ms"] = wall(decode, calls)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=25)
    ap.add_argument("--dir", default="/dev/shm" if os.path.isdir("/dev/shm") else None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r19_resize_timing.json"))
    ap.add_argument("--sizes", default=",".join(SIZES))
    args = ap.parse_args()
    folder = tempfile.mkdtemp(prefix="scg_resize_timing_", dir=args.dir)
    try:
        res = {"tool": "tools/resize_timing.py", "device": torch.cuda.get_device_name(0), "calls": args.calls, "pillow": PIL.__version__,
               "host_cpus_used": torch.get_num_threads(),
               "directory": "memory-backed" if (args.dir or "").startswith("/dev/shm") else "default temporary directory",
               "copy_ceiling_GBs": COPY_CEILING_GBS, "sizes": {}}
        for name in args.sizes.split(","):
            print(name, file=sys.stderr, flush=True)
            res["sizes"][name] = one_size(*SIZES[name], folder, args.calls)
    finally:
        shutil.rmtree(folder, ignore_errors=True)
    text = json.dumps(res, indent=1)
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()

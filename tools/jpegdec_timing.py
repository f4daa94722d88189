"""What decoding camera images on the GPU costs against the host route (no gate: a measurement).

    python tools/jpegdec_timing.py [--out profiles/r25_jpegdec_timing.json] [--calls 25] [--scene 20]
    tools/kstats.sh jpegdec python tools/jpegdec_timing.py --decodes-only 10      the kernel trace of profiles/r25_jpegdec_kernel_trace.txt:
                                                                                  ten decodes of the small image, then ten of the large one
    python tools/jpegdec_timing.py --batch [--out profiles/r26_jpegdec_batch_timing.json]      a scene's images in ONE decode_batch:
                                                                                  20 and 3 files at both sizes against the loop of load_image
    tools/kstats.sh jpegdec_batch python tools/jpegdec_timing.py --batch-only 10  the kernel trace of a 20-image batch (1600 x 1200), ten times

One process, warm, every figure the MEDIAN of `--calls` calls synchronised on both sides, the files in a memory-backed directory.
Inputs: a 4032 x 3024 and a 1600 x 1200 4:2:0 file at quality 90, SYNTHETIC (a ramp with noise: no photograph is at hand) — a
photograph's bit rate, and with it the number of subsequences and the sync behaviour, may differ.  Baseline: the reference's route
PILtoTorch(Image.open(path), res).to("cuda") (utils/general_utils.py:22-28, stated below), its decode alone as
np.asarray(Image.open(path)).  Against it: jpeg_decode.decode, images.load_image, the launches alone between two events, the
upload, the sync launches the file took, the cost of a sync launch, a scene of `--scene` images by both routes.  Both routes must
give the same bytes (`same_bytes`)."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from scgaussian_amd import images, jpeg_decode  # noqa: E402


def piltotorch(pil_image, resolution):
    t = torch.from_numpy(np.array(pil_image.resize(resolution))) / 255.0
    return t.permute(2, 0, 1) if t.dim() == 3 else t.unsqueeze(dim=-1).permute(2, 0, 1)


def median_ms(fn, calls):
    fn()
    times = []
    for _ in range(calls):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(times)


def synthetic(h, w, seed):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    base = np.stack([x * 255 // (w - 1), y * 255 // (h - 1), (x + y) * 255 // (w + h - 2)], axis=2).astype(np.int64)
    return np.clip(base + rng.integers(-12, 13, size=(h, w, 3)), 0, 255).astype(np.uint8)


def measure(path, res, calls, scene, folder):
    dev = torch.device("cuda", torch.cuda.current_device())
    with open(path, "rb") as fh:
        data = fh.read()
    info = jpeg_decode.parse(data)
    out = {"file_bytes": len(data), "segment_bytes": info.segment_end - info.segment_start, "size": [info.W, info.H], "resolution": list(res)}
    out["subsequences"] = -(-out["segment_bytes"] // jpeg_decode.SUBSEQ)
    want = piltotorch(Image.open(path), res).to(dev)
    got = images.load_image(path, res, dev)
    u8 = jpeg_decode.decode(path, dev)
    out["route"], out["sync_launches_taken"], out["status"] = jpeg_decode.LAST["route"], jpeg_decode.LAST["rounds"], jpeg_decode.LAST["status"]
    out["same_bytes"] = bool(torch.equal(got.view(torch.int32), want.contiguous().view(torch.int32))
                             and np.array_equal(u8.cpu().numpy(), np.asarray(Image.open(path))))
    out["baseline_piltotorch_to_cuda_ms"] = median_ms(lambda: piltotorch(Image.open(path), res).to(dev), calls)
    out["baseline_decode_alone_ms"] = median_ms(lambda: np.asarray(Image.open(path)), calls)
    out["parent_pil_to_torch_ms"] = median_ms(lambda: images.pil_to_torch(Image.open(path), res, dev), calls)
    out["jpeg_decode_decode_ms"] = median_ms(lambda: jpeg_decode.decode(path, dev), calls)
    out["images_load_image_ms"] = median_ms(lambda: images.load_image(path, res, dev), calls)
    out["parse_ms"] = median_ms(lambda: jpeg_decode.parse(data), calls)
    staged = jpeg_decode.stage(info, data)
    out["upload_ms"] = median_ms(lambda: staged.to(dev, non_blocking=True), calls)
    upload = staged.to(dev)
    plan = jpeg_decode.plan_of(info.frame, dev)
    pixels = torch.empty(plan.shape, dtype=torch.uint8, device=dev)
    seg = upload.data_ptr() + jpeg_decode.HEADER_BYTES + info.segment_start
    max_rounds = jpeg_decode.sizes(info.frame, out["segment_bytes"])[2]

    def launches(rounds):
        times = []
        for _ in range(calls + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            plan.launch(upload.data_ptr(), seg, out["segment_bytes"], pixels, 0, rounds)
            e1.record()
            torch.cuda.synchronize()
            times.append(e0.elapsed_time(e1))
        return statistics.median(times[1:])

    first = min(jpeg_decode.FIRST_ROUNDS, max_rounds)
    out["launches_alone_ms"] = launches(first)
    if max_rounds >= first + 2:
        out["ms_per_sync_launch_beyond_convergence"] = (launches(first + 2) - out["launches_alone_ms"]) / 2
        out["launches_with_one_sync_launch_ms"] = launches(1)          # (states not settled: only the cost)
    paths = []
    for i in range(scene):
        p = os.path.join(folder, f"scene_{info.W}_{i}.jpg")
        with open(p, "wb") as fh:
            fh.write(data)
        paths.append(p)
    out["scene_images"] = scene
    out["scene_baseline_ms"] = median_ms(lambda: [piltotorch(Image.open(p), res).to(dev) for p in paths], 3)
    out["scene_device_ms"] = median_ms(lambda: [images.load_image(p, res, dev) for p in paths], 3)
    for p in paths:
        os.remove(p)
    return out


def scene_files(folder, w, h, count):
    """`count` synthetic files of one size (different noise each, so that no two share a bit stream)."""
    paths = []
    for i in range(count):
        p = os.path.join(folder, f"batch_{w}_{i}.jpg")
        if not os.path.exists(p):
            Image.fromarray(synthetic(h, w, w + i)).save(p, quality=90, subsampling="4:2:0")
        paths.append(p)
    return paths


def measure_batch(paths, res, calls):
    """A scene of len(paths) images: the loop of load_image (what the parent commit offers) against load_images, decode_batch alone
    and the batch's launches between two events."""
    dev = torch.device("cuda", torch.cuda.current_device())
    out = {"images": len(paths), "resolution": list(res)}
    loop = [images.load_image(p, res, dev) for p in paths]
    got = images.load_images(paths, res, dev)
    out["same_bytes"] = all(torch.equal(a.view(torch.int32), b.contiguous().view(torch.int32)) for a, b in zip(got, loop))
    last = dict(jpeg_decode.LAST)
    out.update(uploads=last["uploads"], host_reads=last["host_reads"], headers=last["headers"], chunks=last["chunks"],
               sync_launches_taken=max(last["rounds"]), routes=sorted(set(last["route"])))
    out["loop_of_load_image_ms"] = median_ms(lambda: [images.load_image(p, res, dev) for p in paths], calls)
    out["load_images_ms"] = median_ms(lambda: images.load_images(paths, res, dev), calls)
    out["decode_batch_ms"] = median_ms(lambda: jpeg_decode.decode_batch(paths, dev), calls)
    files = [open(p, "rb").read() for p in paths]
    stage = jpeg_decode.BatchStage([jpeg_decode.parse(f) for f in files], files).plan()
    out.update(staged_bytes=stage.nbytes, file_bytes=sum(len(f) for f in files), workspace_bytes=stage.workspace_bytes,
               max_rounds=stage.max_rounds)
    staged = torch.empty(stage.nbytes, dtype=torch.uint8, pin_memory=True)
    out["stage_ms"] = median_ms(lambda: jpeg_decode.BatchStage([jpeg_decode.parse(f) for f in files], files).plan().fill(staged.numpy()), calls)
    out["upload_ms"] = median_ms(lambda: staged.to(dev, non_blocking=True), calls)
    upload = staged.to(dev)
    pixels = torch.empty(stage.out_bytes, dtype=torch.uint8, device=dev)
    ws = torch.empty(stage.workspace_bytes, dtype=torch.uint8, device=dev)
    rounds = min(jpeg_decode.FIRST_ROUNDS, stage.max_rounds)
    times = []
    for _ in range(calls + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        jpeg_decode.launch_batch(stage, upload, pixels, ws, rounds)
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    out["launches_alone_ms"] = statistics.median(times[1:])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "r25_jpegdec_timing.json"))
    ap.add_argument("--calls", type=int, default=25)
    ap.add_argument("--scene", type=int, default=20)
    ap.add_argument("--decodes-only", type=int, default=0, help="decode each image this many times and measure nothing (for a kernel trace)")
    ap.add_argument("--batch", action="store_true", help="the batch leg: 20 and 3 files at both sizes (default --out: r26_jpegdec_batch_timing.json)")
    ap.add_argument("--batch-only", type=int, default=0, help="decode a 20-image batch this many times and measure nothing (for a kernel trace)")
    args = ap.parse_args()
    memory = "/dev/shm" if os.path.isdir("/dev/shm") and os.access("/dev/shm", os.W_OK) else None
    if args.batch_only:
        with tempfile.TemporaryDirectory(dir=memory) as folder:
            paths = scene_files(folder, 1600, 1200, args.scene)
            for _ in range(args.batch_only):
                jpeg_decode.decode_batch(paths)
        torch.cuda.synchronize()
        return
    if args.batch:
        if args.out.endswith("r25_jpegdec_timing.json"):
            args.out = os.path.join(os.path.dirname(args.out), "r26_jpegdec_batch_timing.json")
        result = {"device": torch.cuda.get_device_name(0), "calls": args.calls, "files_in": memory or "the default temporary directory",
                  "inputs": "synthetic (ramp + noise, another seed per file), 4:2:0, quality 90", "scenes": {}}
        with tempfile.TemporaryDirectory(dir=memory) as folder:
            for (w, h), res in (((1600, 1200), (200, 150)), ((4032, 3024), (504, 378))):
                for count in (args.scene, 3):
                    result["scenes"][f"{count} x {w}x{h}"] = measure_batch(scene_files(folder, w, h, count), res, args.calls)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(result, fh, indent=1)
        print(json.dumps(result, indent=1))
        return
    if args.decodes_only:
        import io
        for (w, h) in ((1600, 1200), (4032, 3024)):
            buf = io.BytesIO()
            Image.fromarray(synthetic(h, w, w)).save(buf, format="JPEG", quality=90, subsampling="4:2:0")
            for _ in range(args.decodes_only):
                jpeg_decode.decode(buf.getvalue())
        torch.cuda.synchronize()
        return
    result = {"device": torch.cuda.get_device_name(0), "calls": args.calls, "files_in": memory or "the default temporary directory",
              "inputs": "synthetic (ramp + noise), 4:2:0, quality 90: a photograph's bit rate and sync behaviour may differ", "images": {}}
    with tempfile.TemporaryDirectory(dir=memory) as folder:
        for (w, h), res in (((4032, 3024), (504, 378)), ((1600, 1200), (200, 150))):
            path = os.path.join(folder, f"{w}x{h}.jpg")
            Image.fromarray(synthetic(h, w, w)).save(path, quality=90, subsampling="4:2:0")
            result["images"][f"{w}x{h}"] = measure(path, res, args.calls, args.scene, folder)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
    print(json.dumps(result, indent=1))


if __name__ == "__main__":
    main()

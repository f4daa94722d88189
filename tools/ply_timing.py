#!/usr/bin/env python3
"""What saving and loading a scene cost (profiles/r18_ply_timing.json).  Prints ONE JSON object and writes it to --out.

One process, warm, every call synchronised on both sides, median of --calls calls per leg (the protocol of tools/eval_timing.py),
at 10 000 + 2 000 and 1 000 000 + 250 000 Gaussians (ray-bound + background), files in a memory-backed directory (--dir, default
/dev/shm when it exists).  Per size, a model whose fourteen tensors are on the GPU:
  host_save / host_load     the route before this module: ply_io.save_ply / ply_io.load_ply(device="cuda")
  hip_save / hip_load       ply.save_ply / ply.load_ply as a whole
  ... split:                pack_launch / unpack_launch  the launch(es) between two events (ms) with the bytes they move (read +
                            written, from the layout) and that rate against the project's measured copy ceiling (6.29 TB/s)
                            copy          PackedScene.to_host: the one device-to-host transfer
                            write / read  the three files written from the host buffer / the bodies read into pinned memory
                            upload        load_ply's host-to-device transfers
  color_host / color_hip    render.sh_to_rgb + store_color_ply against ply.save_color_pcd (degree 3)
What one process of one visit shows: the medians of these calls on this machine in this state; no run-to-run spread.

    python tools/ply_timing.py [--calls 25] [--out profiles/r18_ply_timing.json]"""
import argparse
import ctypes as C
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from scgaussian_amd import _lib, _lib_io, ply, ply_io                                         # noqa: E402
from scgaussian_amd import render as rmod                                                    # noqa: E402

SIZES = {"10k+2k": (10_000, 2_000), "1M+250k": (1_000_000, 250_000)}
DEV = "cuda"
COPY_CEILING_GBS = 6290.0


def model(nr, nb, seed=0):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)                                              # noqa: E731
    d = r(nr, 3)
    return ply_io.RayBoundModel(
        features_dc=torch.rand(nr, 1, 3, generator=g) * 3 - 1.5, features_rest=r(nr, 15, 3) * 0.1, opacity=r(nr, 1),
        scaling=r(nr, 3) - 3, rotation=r(nr, 4), zval=torch.rand(nr, 1, generator=g) + 0.2, rayo=r(nr, 3) * 0.1,
        rayd=d / d.norm(dim=1, keepdim=True), bg_xyz=r(nb, 3), bg_features_dc=torch.rand(nb, 1, 3, generator=g) * 3 - 1.5,
        bg_features_rest=r(nb, 15, 3) * 0.1, bg_opacity=r(nb, 1), bg_scaling=r(nb, 3) - 3, bg_rotation=r(nb, 4)).to(DEV)


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


def rate(nbytes, ms):
    gbs = nbytes / (ms * 1e-3) / 1e9
    return {"bytes": int(nbytes), "GBs": round(gbs, 1), "of_copy_ceiling": round(gbs / COPY_CEILING_GBS, 4)}


def one_size(nr, nb, folder, calls):
    g = model(nr, nb)
    P = nr + nb
    old, new = os.path.join(folder, "old", "point_cloud.ply"), os.path.join(folder, "new", "point_cloud.ply")
    res = {"nr": nr, "nb": nb}
    res["host_save_ms"] = wall(lambda: ply_io.save_ply(old, g), calls)
    res["hip_save_ms"] = wall(lambda: ply.save_ply(g, new), calls)
    res["pack_launch_ms"] = events(lambda: ply.pack(g), calls)
    lay = ply.pack(g).layout
    moved = 2 * (lay.ray_bytes + lay.bg_bytes) - 24 * nr - 12 * nb + 40 * nr + 24 * nb + lay.color_bytes   # tensors read, bodies written; the colour tiles' inputs and body
    res["pack_launch"] = rate(moved, res["pack_launch_ms"])

    def copy():
        p = ply.pack(g)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        p.to_host()
        return (time.perf_counter() - t0) * 1e3, p
    copy()
    res["copy_ms"] = round(statistics.median(copy()[0] for _ in range(calls)), 4)
    res["copy_GBs"] = round(lay.total / (res["copy_ms"] * 1e-3) / 1e9, 2)
    packed = copy()[1]
    res["write_ms"] = wall(lambda: packed.write(new), calls)
    res["files_bytes"] = sum(os.path.getsize(os.path.join(folder, "new", f)) for f in os.listdir(os.path.join(folder, "new")))
    for f in os.listdir(os.path.join(folder, "new")):
        a, b = (open(os.path.join(folder, d, f), "rb").read() for d in ("old", "new"))
        assert a == b, f

    holder = ply_io.RayBoundModel(**{k: getattr(g, k)[:1].cpu() for k in ("features_dc", "features_rest", "opacity", "scaling", "rotation",
                                                                          "zval", "rayo", "rayd")})
    res["host_load_ms"] = wall(lambda: ply_io.load_ply(old, device=DEV), calls)
    res["hip_load_ms"] = wall(lambda: ply.load_ply(holder, new), calls)
    assert torch.equal(holder.features_rest, g.features_rest) and torch.equal(holder.bg_rotation, g.bg_rotation)

    # the parts of load_ply: the read into pinned memory, the upload, the launch
    parts = {"read_ms": [], "upload_ms": [], "unpack_launch_ms": []}
    for _ in range(calls + 1):
        for path, bg in ((new, False), (os.path.join(folder, "new", "point_cloud_bg.ply"), True)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            with open(path, "rb") as fh:
                head = ply.read_header(fh, path)
                table = ply.column_table([n for n, _t in head["props"]], bg)
                rows, stride = head["count"], len(head["props"])
                body = rows * stride * 4
                staged = torch.empty(body + table.nbytes, dtype=torch.uint8, pin_memory=True)
                view = staged.numpy()
                fh.readinto(memoryview(view[:body]))
                view[body:] = table.view(np.uint8)
            t1 = time.perf_counter()
            upload = staged.to(DEV, non_blocking=True)
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            out = ply._empty_set(rows, bg, torch.device(DEV, torch.cuda.current_device()))
            m = _lib.ScgModel()
            dst = m.bg if bg else m.ray
            dst.count = rows
            for n, t in out.items():
                setattr(dst, n[3:] if bg else n, t.data_ptr())
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            _lib_io.check(_lib_io.load().scg_ply_unpack(upload.data_ptr(), body, table.ctypes.data_as(C.POINTER(C.c_int32)), rows, stride,
                                                        int(bg), C.byref(m), torch.cuda.current_stream().cuda_stream), "scg_ply_unpack")
            b.record()
            torch.cuda.synchronize()
            key = "bg" if bg else "ray"
            parts["read_ms"].append((key, (t1 - t0) * 1e3))
            parts["upload_ms"].append((key, (t2 - t1) * 1e3))
            parts["unpack_launch_ms"].append((key, a.elapsed_time(b)))
    for k, v in parts.items():
        v = v[2:]                                                                            # the first round is the warm-up
        res[k] = round(statistics.median(x for n, x in v if n == "ray") + statistics.median(x for n, x in v if n == "bg"), 4)
    res["unpack_launch"] = rate(2 * (lay.ray_bytes + lay.bg_bytes) - 24 * nr - 12 * nb, res["unpack_launch_ms"])

    cam = torch.tensor([0.0, 0.0, 4.0], device=DEV)
    cold, cnew = os.path.join(folder, "cold"), os.path.join(folder, "cnew")

    def color_host():
        xyz = g.get_xyz
        rgb = rmod.sh_to_rgb(3, g.get_features, xyz, cam)
        rmod.store_color_ply(os.path.join(cold, "point_cloud_color.ply"), xyz.cpu().numpy(), rgb.cpu().numpy() * 255)
    res["color_host_ms"] = wall(color_host, calls)
    res["color_hip_ms"] = wall(lambda: ply.save_color_pcd(g, cam, cnew, sh_degree=3), calls)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=25)
    ap.add_argument("--dir", default="/dev/shm" if os.path.isdir("/dev/shm") else None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r18_ply_timing.json"))
    ap.add_argument("--sizes", default=",".join(SIZES))
    args = ap.parse_args()
    folder = tempfile.mkdtemp(prefix="scg_ply_timing_", dir=args.dir)
    try:
        res = {"tool": "tools/ply_timing.py", "device": torch.cuda.get_device_name(0), "calls": args.calls,
               "directory": "memory-backed" if (args.dir or "").startswith("/dev/shm") else "default temporary directory",
               "copy_ceiling_GBs": COPY_CEILING_GBS, "sizes": {}}
        for name in args.sizes.split(","):
            res["sizes"][name] = one_size(*SIZES[name], os.path.join(folder, name), args.calls)
    finally:
        shutil.rmtree(folder, ignore_errors=True)
    text = json.dumps(res, indent=1)
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""What the depth colour map of a frame and a whole video cost (profiles/r15_depthviz_timing.json).  Prints ONE JSON object and
writes it to --out.

One process, warm, every call synchronised on both sides, median of --calls calls per leg (the protocol of tools/eval_timing.py), at
1600 x 1200 and 400 x 300.  Per size, one frame whose normalised depth and rendering are on the GPU:
  host_frame          the reference's per-frame statements, restated (render_video.py:146-151 with :98-113): the normalised depth
                      copied to the host, np.percentile(depth, 98), depth.min(), matplotlib's Normalize + ScalarMappable('turbo')
                      .to_rgba where matplotlib is importable (else the numpy restatement of tests/depthviz_refs.py; "mapper" says
                      which), the truncating cast; the rendering copied to the host, * 255., cast, reversed
  hip_colorize        video.DepthColorizer.colorize: the select and the frame kernel, no host read (the synchronisation around the
                      call is the protocol's)
  hip_frame           DepthColorizer.frame with all five outputs (what render_video does per frame behind the rasteriser)
and a video of 60 frames of a synthetic scene (--video-runs runs, median):
  video_host_loop     render, clamp, normalise in torch, then host_frame's statements per frame
  video_hip           video.render_video: one host read after the loop
PNG encoding, the file system and the video container are in no leg.

select_*: scg_viz_select alone, 20 calls per synchronisation, on a normalised depth (most first digits in a dozen bins), on uniform
random bits (every bin) and on a constant plane (one bin), with the library as shipped and with each variant of csrc/depthviz.hip's
SCG_VIZ_HIST_MODE whose library exists: "plain" one LDS atomic per value, "merge" equal digits of a wave merged by a ballot first,
"wave" a histogram per wave in the first pass.  Build them with --build-variants (on the machine that has the object files).

    python tools/depthviz_timing.py [--calls 25] [--out profiles/r15_depthviz_timing.json]"""
import argparse
import json
import os
import statistics
import sys
import time
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import depthviz_refs as D                                                                    # noqa: E402
from scgaussian_amd import _lib, video                                                       # noqa: E402
from scgaussian_amd import render as rmod                                                    # noqa: E402
from scgaussian_amd import synthetic as syn                                                  # noqa: E402

SIZES = {"1600x1200": (1200, 1600), "400x300": (300, 400)}
DEV = "cuda"
FRAMES = 60
SELECTS_PER_SYNC = 20
HIST_MODES = ("plain", "merge", "wave")          # SCG_VIZ_HIST_MODE 0, 1, 2

try:
    import matplotlib as mpl
    import matplotlib.cm as cm
    MAPPER = "matplotlib " + mpl.__version__
except ImportError:                                                                          # pragma: no cover
    mpl = cm = None
    MAPPER = "numpy restatement"


def visualization(depth):
    """render_video.py:98-113 without the file"""
    vmax = np.percentile(depth, 98)
    vmin = depth.min()
    if mpl is None:
        return D.colorize(depth, video.TURBO, st=(vmin, vmax))
    mapper = cm.ScalarMappable(norm=mpl.colors.Normalize(vmin=vmin, vmax=vmax), cmap="turbo")
    return (mapper.to_rgba(depth)[:, :, :3] * 255).astype(np.uint8)


def host_frame(rendering, depth):
    """render_video.py:146-151: `rendering` clamped (3,H,W), `depth` normalised (1,H,W), both on the GPU"""
    color_depth = visualization(depth.detach().cpu().numpy()[0])
    video_img = (rendering.permute(1, 2, 0).detach().cpu().numpy() * 255.).astype(np.uint8)[..., ::-1]
    return video_img, color_depth[..., ::-1]


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


def smooth_depth(H, W):
    y, x = torch.meshgrid(torch.linspace(0, 1, H), torch.linspace(0, 1, W), indexing="ij")
    g = torch.Generator().manual_seed(0)
    return (3 + 2.5 * y + 0.8 * x + 0.3 * torch.sin(9 * x) * torch.cos(7 * y) + 0.01 * torch.rand(H, W, generator=g)).float()


def video_scene(H, W):
    sc = syn.make_scene(20000, W, H, seed=3)
    model = syn.make_raw_model(sc).to(DEV)
    model.active_sh_degree = 3
    views = [types.SimpleNamespace(**syn.orbit_camera(W, H, -15.0 + 0.5 * i, -2.0, 7.0).to(DEV)._asdict()) for i in range(FRAMES)]
    return views, model, rmod.PipelineParams(), torch.zeros(3, device=DEV)


def select_leg(lib, plane, rng):
    n = plane.numel()
    nbytes = lib.scg_viz_select_scratch_bytes(n)
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    stats, nan = torch.zeros(4, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream

    def fn():
        for _ in range(SELECTS_PER_SYNC):
            rc = lib.scg_viz_select(plane.data_ptr(), _lib.ptr(rng), n, 98.0, stats.data_ptr(), nan.data_ptr(), scratch.data_ptr(), nbytes, stream)
            assert rc == 0
    return fn, stats


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=25)
    ap.add_argument("--video-runs", type=int, default=3)
    ap.add_argument("--build-variants", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r15_depthviz_timing.json"))
    a = ap.parse_args()
    assert a.calls >= 20
    res = {"device": torch.cuda.get_device_name(0), "calls": a.calls, "mapper": MAPPER, "numpy": np.__version__, "frames": FRAMES,
           "what": "median ms per call, one process, warm, synchronised around each call; select_*: us per scg_viz_select"}
    libs = {"shipped": _lib.load()}
    for mode, name in enumerate(HIST_MODES):
        path = _lib.LIB_PATH.replace(".so", f"_viz{name}.so")
        if a.build_variants:
            from scgaussian_amd import build
            build.build(tag=f"viz{name}", defines=(f"SCG_VIZ_HIST_MODE={mode}",), only=("depthviz.hip",))
        if os.path.exists(path):
            libs[name] = _lib.open_library(path)
    for tag, (H, W) in SIZES.items():
        raw = smooth_depth(H, W).to(DEV)[None]
        depth = (raw - raw.min()) / (raw.max() - raw.min())
        rendering = torch.rand(3, H, W, device=DEV, generator=torch.Generator(DEV).manual_seed(1))
        viz = video.DepthColorizer(H, W)
        outs = {k: torch.empty((H, W) if k == "depth_u8" else (H, W, 3), dtype=torch.uint8, device=DEV)
                for k in ("depth_color", "depth_color_bgr", "depth_u8", "render_u8", "frame_bgr")}
        for leg, fn in (("host_frame", lambda: host_frame(rendering, depth)),
                        ("hip_colorize", lambda: viz.colorize(depth, out=outs["depth_color"])),
                        ("hip_frame", lambda: viz.frame(raw, viz.depth_range(raw), render=rendering, **outs))):
            res[f"{tag}_{leg}_ms"], res[f"{tag}_{leg}_min_ms"] = median_ms(fn, a.calls)
        res[f"{tag}_frame_speedup"] = round(res[f"{tag}_host_frame_ms"] / res[f"{tag}_hip_colorize_ms"], 1)
        # the two legs computed the same bytes
        frame_h, color_h = host_frame(rendering, depth)
        res[f"{tag}_same_bytes"] = bool(np.array_equal(color_h[..., ::-1], viz.colorize(depth).cpu().numpy())
                                        and np.array_equal(frame_h, outs["frame_bgr"].cpu().numpy()))
        # the select alone, by what the first digit looks like
        bits = torch.randint(-2 ** 31, 2 ** 31 - 1, (H * W,), dtype=torch.int64, generator=torch.Generator().manual_seed(2)).to(torch.int32)
        spread = bits.view(torch.float32).nan_to_num(0.0).to(DEV)
        planes = {"depth01": depth.reshape(-1).contiguous(), "random_bits": spread, "constant": torch.full((H * W,), 0.625, device=DEV)}
        for pname, plane in planes.items():
            got = {}
            for lname, lib in libs.items():
                fn, stats = select_leg(lib, plane, None)
                med, mn = median_ms(fn, a.calls)
                res[f"{tag}_select_{pname}_{lname}_us"] = round(med * 1e3 / SELECTS_PER_SYNC, 2)
                res[f"{tag}_select_{pname}_{lname}_min_us"] = round(mn * 1e3 / SELECTS_PER_SYNC, 2)
                got[lname] = stats.cpu().view(torch.int32).tolist()
            assert all(v == got["shipped"] for v in got.values()), (tag, pname, got)
        # a video
        views, model, pipe, bg = video_scene(H, W)

        def host_loop():
            with torch.no_grad():
                for view in views:
                    pkg = rmod.render(view, model, pipe, bg)
                    r = torch.clamp(pkg["render"], min=0., max=1.)
                    d = pkg["rendered_depth"]
                    d = (d - d.min()) / (d.max() - d.min())
                    host_frame(r, d)
        for leg, fn in (("video_host_loop", host_loop), ("video_hip", lambda: video.render_video(views, model, pipe, bg))):
            res[f"{tag}_{leg}_ms"], res[f"{tag}_{leg}_min_ms"] = median_ms(fn, a.video_runs, warm=1)
        res[f"{tag}_video_speedup"] = round(res[f"{tag}_video_host_loop_ms"] / res[f"{tag}_video_hip_ms"], 2)
        res[f"{tag}_video_per_frame_saved_ms"] = round((res[f"{tag}_video_host_loop_ms"] - res[f"{tag}_video_hip_ms"]) / FRAMES, 3)
    text = json.dumps(res)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text + "\n")


if __name__ == "__main__":
    main()

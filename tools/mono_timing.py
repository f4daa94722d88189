#!/usr/bin/env python3
"""What building the scene's view_gs and packing it for its consumers costs (profiles/r17_mono_timing.json).  Prints ONE JSON object
and writes it to --out.

Leg one, the parent commit's route: the plain-torch restatement of the reference's create_from_mono loop (tests/mono_refs.py
torch_loop: per ordered pair two grid_samples, the batched 3x3 products, three inverse() calls, the small uploads), then
InitStage.from_view_gs and SeedInputs.from_view_gs on its dictionary.  Leg two: mono.MonoSetup.build (staging, ONE upload, three
launches) + InitStage.from_mono + SeedInputs.from_mono.  Same process, same cameras and matches, warm, synchronised around each call,
median of --calls calls per leg, at 3 views x 2 000 and 7 views x 2 000 matches per ordered pair on 504 x 378 images.  Also recorded:
the three launches alone between two events (median of the same number of replays on a built setup), and the host reads of leg two
(a count that follows from the code: the pairs' counts, once).

    python tools/mono_timing.py [--calls 25] [--out profiles/r17_mono_timing.json]"""
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
import mono_refs as MR                                                                       # noqa: E402
from scgaussian_amd import mono, seed                                                        # noqa: E402
from scgaussian_amd.init_stage import InitStage                                              # noqa: E402

SIZES = {"3views": 3, "7views": 7}
PER_PAIR, W, H = 2000, 504, 378
LAUNCHES = {"scg_mono_images": 1, "scg_mono_matches": 1, "scg_mono_pairs": 1}


def scene(V, seed_=0):
    rng = np.random.default_rng(seed_)
    masks = [None if i % 3 == 0 else (rng.random((H, W)) > 0.1).astype(np.float64) for i in range(V)]
    cams = MR.cameras([(H, W)] * V, rng, masks=masks, fovs=[55.0] * V)
    return cams, MR.match_data(cams, PER_PAIR, rng, lo=0.0, hi=1.0)


def median_ms(fn, calls):
    times = []
    for it in range(3 + calls):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if it >= 3:
            times.append((time.perf_counter() - t0) * 1e3)
    return round(statistics.median(times), 4), round(min(times), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=25)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r17_mono_timing.json"))
    a = ap.parse_args()
    assert a.calls >= 20
    dev = "cuda"
    res = {"device": torch.cuda.get_device_name(0), "calls": a.calls, "what": "median ms per scene setup + packing for the init stage and the seed",
           "matches_per_pair": PER_PAIR, "image": [W, H], "launches_by_entry": LAUNCHES, "hip_host_reads": 1}
    for tag, V in SIZES.items():
        cams, md = scene(V)

        def torch_route():
            vg = MR.torch_loop(cams, md, dev)
            stage = InitStage.from_view_gs(vg)
            return vg, stage, seed.SeedInputs.from_view_gs(vg, stage)

        def hip_route():
            setup = mono.MonoSetup.build(cams, md, dev)
            stage = InitStage.from_mono(setup)
            return setup, stage, seed.SeedInputs.from_mono(setup, stage)

        torch.manual_seed(0)
        vg, stage_t, _ = torch_route()
        torch.manual_seed(0)
        setup, stage_h, _ = hip_route()
        assert stage_t.segments == stage_h.segments and torch.equal(stage_t.z, stage_h.z)       # the same depths from the same seed
        dev_err = float((torch.cat([i["color"] for v in vg.values() for i in v["match_infos"].values()]) - setup.color).abs().max())
        res[f"{tag}_matches"], res[f"{tag}_pairs"], res[f"{tag}_color_max_abs_diff"] = setup.plan.N, setup.plan.nseg, dev_err
        res[f"{tag}_torch_ms"], res[f"{tag}_torch_min_ms"] = median_ms(torch_route, a.calls)
        res[f"{tag}_hip_ms"], res[f"{tag}_hip_min_ms"] = median_ms(hip_route, a.calls)
        res[f"{tag}_hip_build_alone_ms"], _ = median_ms(lambda: mono.MonoSetup.build(cams, md, dev), a.calls)
        res[f"{tag}_hip_plan_alone_ms"], _ = median_ms(lambda: mono.MonoPlan(cams, md), a.calls)          # host only: walk, tables, staging
        begin, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        kernel = []
        for it in range(3 + a.calls):
            torch.cuda.synchronize()
            begin.record()
            setup.launch()
            end.record()
            end.synchronize()
            if it >= 3:
                kernel.append(begin.elapsed_time(end))
        res[f"{tag}_hip_three_launches_ms"] = round(statistics.median(kernel), 4)
        res[f"{tag}_speedup"] = round(res[f"{tag}_torch_ms"] / res[f"{tag}_hip_ms"], 2)
    text = json.dumps(res)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text + "\n")


if __name__ == "__main__":
    main()

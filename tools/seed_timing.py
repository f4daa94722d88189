#!/usr/bin/env python3
"""What seeding the model from the init stage costs (profiles/r11_seed_timing.json).  Prints ONE JSON object and writes it to --out.

Times the plain-torch restatement of the reference's create_from_pcd in the reference's per-pair form (tests/seed_refs.py
seed_per_pair: per ordered pair a mask, six boolean gathers and an indexed write, then the concatenations; the kNN through the
project's simple_knn) against seed.seed_arrays (csrc/seed.hip + the same kNN): same process, same inputs on the device, warm, every
call on a fresh copy of min_loss, synchronised around each call, median of --calls calls per leg, at 3 views x 2 000 matches
per ordered pair (6 pairs) and 7 views x 2 000 (42 pairs), 640 x 480 images, about half the matches kept.  Also recorded: the whole
seed.create_from_pcd on packed inputs (the four torch.stack calls and the parameter hand-over included), the kNN alone on the kept
points, and the kernel launches of one seed_arrays call (a count that follows from the code: it depends on no size).

    python tools/seed_timing.py [--calls 25] [--out profiles/r11_seed_timing.json]"""
import argparse
import contextlib
import io
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import seed_refs as S                                                                        # noqa: E402
from scgaussian_amd import seed                                                              # noqa: E402
from simple_knn._C import distCUDA2                                                          # noqa: E402

SIZES = {"3views": 3, "7views": 7}
PER_PAIR, W, H = 2000, 640, 480
# the kernel launches of one seed_arrays call, by C entry (csrc/seed.hip, csrc/knn.hip): the same at any number of pairs or views
LAUNCHES = {"scg_seed_classify": 2, "scg_seed_scatter": 1, "scg_knn3_mean_dist2_ws": 2, "scg_seed_finish": 1}


def arena(V, dev, seed_=0):
    g = torch.Generator().manual_seed(seed_)
    r = lambda *s: torch.rand(*s, generator=g)                                              # noqa: E731
    pairs = [(a, b) for a in range(V) for b in range(V) if b != a]
    N = PER_PAIR * len(pairs)
    d = torch.nn.functional.normalize(r(N, 3) - 0.5, dim=1)
    a = dict(rays_o=r(N, 3) * 2 - 1, rays_d=d, color=r(N, 3), z=r(N) * 6 + 2, cam_z=r(N) * 0.5 + 0.5,
             uv=torch.stack([r(N) * W, r(N) * H], 1), min_loss=r(N) * 0.2, counts=[PER_PAIR] * len(pairs),
             seg_view=[p[0] for p in pairs], V=V, H=H, W=W)
    return {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in a.items()}


def median_ms(fn, fresh, calls):
    times = []
    for it in range(3 + calls):
        x = fresh()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn(x)
        torch.cuda.synchronize()
        if it >= 3:
            times.append((time.perf_counter() - t0) * 1e3)
    return round(statistics.median(times), 4), round(min(times), 4)


class _Model:
    pass


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=25)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r11_seed_timing.json"))
    a = ap.parse_args()
    assert a.calls >= 20
    dev = "cuda"
    res = {"device": torch.cuda.get_device_name(0), "calls": a.calls, "what": "median ms per create_from_pcd call",
           "matches_per_pair": PER_PAIR, "image": [W, H], "launches_by_entry": LAUNCHES}
    for tag, V in SIZES.items():
        ar = arena(V, dev)
        views = {v: dict(intr=torch.eye(3, device=dev), w2c=torch.eye(4, device=dev), near_far=torch.tensor([0.5, 50.0], device=dev),
                         image_color=torch.rand(H * W, 3, device=dev)) for v in range(V)}
        vg = S.view_gs_of(ar, views)
        inputs = seed.SeedInputs.from_view_gs(vg)
        fresh = lambda: ar["min_loss"].clone()                                              # noqa: E731
        want = S.seed(ar, distCUDA2)
        got = seed.seed_arrays(inputs, ar["min_loss"])
        assert got["n"] == want["n"] and torch.equal(got["zval"], want["zval"]) and torch.equal(got["sparse_depths"], want["sparse_depths"])
        res[f"{tag}_matches"], res[f"{tag}_pairs"], res[f"{tag}_rows"] = ar["z"].numel(), len(ar["counts"]), got["n"]
        legs = {"torch_per_pair": lambda ml: S.seed_per_pair(vg, S.nested_state(vg, ml), distCUDA2),
                "hip": lambda ml: seed.seed_arrays(inputs, ml)}
        for leg, fn in legs.items():
            res[f"{tag}_{leg}_ms"], res[f"{tag}_{leg}_min_ms"] = median_ms(fn, fresh, a.calls)

        def whole(ml):
            with contextlib.redirect_stdout(io.StringIO()):
                seed.create_from_pcd(_Model(), S.nested_state(vg, ml), inputs=inputs)
        res[f"{tag}_hip_create_from_pcd_ms"], _ = median_ms(whole, fresh, a.calls)
        pts = got["points"]
        res[f"{tag}_knn_alone_ms"], res[f"{tag}_knn_alone_min_ms"] = median_ms(lambda p: distCUDA2(p), lambda: pts.clone(), a.calls)
        res[f"{tag}_speedup"] = round(res[f"{tag}_torch_per_pair_ms"] / res[f"{tag}_hip_ms"], 2)
        res[f"{tag}_hip_launches"] = sum(LAUNCHES.values())
    text = json.dumps(res)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text + "\n")


if __name__ == "__main__":
    main()

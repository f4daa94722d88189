#!/usr/bin/env python3
"""What a densification costs (profiles/r09_densify_timing.json).  Prints ONE JSON object and writes it to --out.

Times the plain-torch restatement of the reference's densify_and_prune (tests/densify_refs.py: the reference's operators, boolean-mask
indexings and concatenations, on torch.optim.Adam) against densify.densify_and_prune (csrc/densify.hip, on ArenaAdam): same process,
same inputs and noise, warm, every call on a fresh copy of the model and optimizer state, synchronised around each call, median of
--calls calls per leg, at 10 000 + 2 000 and 200 000 + 50 000 Gaussians.

    python tools/densify_timing.py [--calls 25] [--out profiles/r09_densify_timing.json]"""
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
import densify_refs as D                                                                     # noqa: E402
from scgaussian_amd import densify, optim                                                    # noqa: E402

SIZES = {"10k+2k": (10_000, 2_000), "200k+50k": (200_000, 50_000)}
MAX_GRAD, MIN_OPACITY, EXTENT = 4e-4, 0.005, 5.0


def inputs(nr, nb, seed=0):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)                                             # noqa: E731
    P = nr + nb
    d = r(nr, 3)
    t = {"_zval": torch.rand(nr, 1, generator=g) * 6 + 3, "_rayo": r(nr, 3) * 0.1, "_rayd": d / d.norm(dim=1, keepdim=True),
         "bg_xyz": r(nb, 3) * 3}
    for pre, n in (("_", nr), ("bg_", nb)):
        t.update({pre + "features_dc": r(n, 1, 3), pre + "features_rest": r(n, 15, 3) * 0.15, pre + "opacity": r(n, 1) * 2,
                  pre + "scaling": r(n, 3) * 0.6 - 3.0, pre + "rotation": r(n, 4)})
    denom = torch.randint(1, 6, (P, 1), generator=g).float()
    # about one Gaussian in six over the threshold: the share the reference's own runs densify
    t.update(xyz_gradient_accum=denom * torch.rand(P, 1, generator=g) * 1.2 * MAX_GRAD, denom=denom,
             max_radii2D=torch.rand(P, generator=g) * 50)
    states = {n: (3.0, r(*t[a].shape) * 1e-3, torch.rand(t[a].shape, generator=g) * 1e-6) for a, n, _t, _lr in D.RAY + D.BG}
    return t, states, torch.randn(2, P, 3, generator=g)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=25)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r09_densify_timing.json"))
    a = ap.parse_args()
    assert a.calls >= 20
    dev = "cuda"
    res = {"device": torch.cuda.get_device_name(0), "calls": a.calls, "what": "median ms per densify_and_prune call"}
    for tag, (nr, nb) in SIZES.items():
        t, states, noise = inputs(nr, nb)
        t = {k: v.to(dev) for k, v in t.items()}
        noise = noise.to(dev)

        def fresh(cls):
            m = D.StandIn(t, 0.01, cls, dev)
            for n, (step, m1, m2) in states.items():
                m.set_state(n, step, m1, m2)
            return m
        legs = {"torch_restatement": (torch.optim.Adam, lambda m: D.densify_and_prune(m, MAX_GRAD, MIN_OPACITY, EXTENT, 20, noise)),
                "hip": (optim.ArenaAdam, lambda m: densify.densify_and_prune(m, MAX_GRAD, MIN_OPACITY, EXTENT, 20, noise=noise))}
        for leg, (cls, fn) in legs.items():
            times = []
            for it in range(3 + a.calls):
                m = fresh(cls)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn(m)
                torch.cuda.synchronize()
                if it >= 3:
                    times.append((time.perf_counter() - t0) * 1e3)
            res[f"{tag}_{leg}_ms"] = round(statistics.median(times), 4)
            res[f"{tag}_{leg}_min_ms"] = round(min(times), 4)
            res[f"{tag}_rows_after"] = int(m.bg_xyz.shape[0])
        res[f"{tag}_speedup"] = round(res[f"{tag}_torch_restatement_ms"] / res[f"{tag}_hip_ms"], 2)
    text = json.dumps(res)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text + "\n")


if __name__ == "__main__":
    main()

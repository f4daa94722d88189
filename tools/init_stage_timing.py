#!/usr/bin/env python3
"""What the ray-depth init stage costs (profiles/r08_init_stage_timing.json).  Prints ONE JSON object and writes it to --out.

Three ways to run the reference's init stage (train.py:49-95; 2 000 Adam iterations on the per-match ray depths, the learning
rate halved before iterations 500, 1 000 and 1 500), in ONE process, alternating, on the same device:

    torch_loop     the plain torch loop (tests/init_refs.py: the reference's method and loop restated), torch.optim.Adam, and the
                   loss.item() per iteration that feeds the reference's progress bar
    loss_op_arena  the same loop with init_stage.match_loss_from_base (one launch forward, none backward) and optim.ArenaAdam
    run_schedule   InitStage.run_schedule: four launches (partial sums recorded), then losses() on the host

at the reference's size (3 views x 2 000 matches per ordered pair: 12 000 depths) and with 4 views (24 000).  Every figure is host
wall time around work that ends in a device synchronise: the median of --rounds rounds; run_schedule, being short, is repeated
--fused-reps times per round and its per-run median taken.  The three legs end at depths that agree (max |difference| reported).

    python tools/init_stage_timing.py [--iters 2000] [--rounds 3] [--fused-reps 20] [--matches 2000] [--out FILE]"""
import argparse
import json
import math
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import init_refs as ir                                                                       # noqa: E402
from scgaussian_amd import optim                                                             # noqa: E402
from scgaussian_amd.init_stage import InitStage, match_loss_from_base                        # noqa: E402

W, H = 1008, 756


def make_view_gs(n_views, M, seed, device):
    """n_views cameras on a line looking down +z at points 4-8 units away; every ordered pair holds M matches (half a pixel of
    noise on the partner's side, 20 % masked out); depths start between 0.6 and 1.5 times the true one."""
    g = torch.Generator().manual_seed(seed)
    f = 0.5 * H / math.tan(math.radians(24.0))
    K = torch.tensor([[f, 0, W / 2], [0, f, H / 2], [0, 0, 1.0]], dtype=torch.float64)
    w2c = []
    for i in range(n_views):
        m = torch.eye(4, dtype=torch.float64)
        m[0, 3], m[1, 3] = -0.5 * (i - (n_views - 1) / 2), 0.03 * i
        w2c.append(m)
    names = [f"view{i}" for i in range(n_views)]
    vg = {n: {"width": W, "height": H, "intr": K.float().to(device), "w2c": w2c[i].float().to(device), "match_infos": {}}
          for i, n in enumerate(names)}

    def side(i, uv, P):
        c2w = torch.linalg.inv(w2c[i])
        p = (torch.linalg.inv(K) @ torch.cat([uv, torch.ones(M, 1, dtype=torch.float64)], 1).t()).t()
        cr = p / p.norm(dim=-1, keepdim=True)
        o = c2w[:3, 3][None].repeat(M, 1)
        t = (P - o).norm(dim=-1) * (torch.rand(M, generator=g, dtype=torch.float64) * 0.9 + 0.6)
        d = dict(uv=uv, rays_o=o, rays_d=(c2w[:3, :3] @ cr.t()).t(), cam_rays_d=cr,
                 blender_mask=(torch.rand(M, generator=g) > 0.1).double(), z_val=t[:, None])
        return {k: v.float().contiguous().to(device) for k, v in d.items()}

    def proj(i, P):
        xyz = (K @ ((w2c[i][:3, :3] @ P.t()).t() + w2c[i][:3, 3]).t()).t()
        return xyz[:, :2] / xyz[:, 2:]
    for i in range(n_views):
        for j in range(i + 1, n_views):
            P = torch.stack([torch.rand(M, generator=g, dtype=torch.float64) * 3 - 1.5,
                             torch.rand(M, generator=g, dtype=torch.float64) * 2 - 1,
                             torch.rand(M, generator=g, dtype=torch.float64) * 4 + 4], 1)
            vg[names[i]]["match_infos"][names[j]] = side(i, proj(i, P), P)
            vg[names[j]]["match_infos"][names[i]] = side(j, proj(j, P) + torch.randn(M, 2, generator=g, dtype=torch.float64) * 0.5, P)
    for v in vg.values():
        for mi in v["match_infos"].values():
            mi["z_val"].requires_grad_(True)
    return vg


def fresh(base):
    """A view_gs that shares the constant tensors of `base` and has its own z_val leaves."""
    return {a: {**v, "match_infos": {b: {**mi, "z_val": mi["z_val"].detach().clone().requires_grad_(True)}
                                     for b, mi in v["match_infos"].items()}} for a, v in base.items()}


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def leg_torch(base, iters, halve_at):
    vg = fresh(base)
    dt, out = timed(lambda: ir.torch_init_loop(vg, iters, halve_at, item_each_iteration=True))
    return dt, ir.flat(vg, out["best"])


def leg_loss_op(base, iters, halve_at):
    vg = fresh(base)
    stage = InitStage.from_view_gs(vg, record_losses=False)
    stage.install(vg)
    dt, out = timed(lambda: ir.torch_init_loop(vg, iters, halve_at, loss_fn=lambda v: match_loss_from_base(v, stage),
                                               optimizer_cls=optim.ArenaAdam, item_each_iteration=True))
    return dt, ir.flat(vg, out["best"])


def leg_fused(base, iters, halve_at, reps):
    times, best = [], None
    for _ in range(reps):
        stage = InitStage.from_view_gs(fresh(base))

        def go():
            stage.run_schedule(iters, halve_at)
            return stage.losses()
        dt, _losses = timed(go)
        times.append(dt)
        best = stage.best_z
    return statistics.median(times), best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=2000)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--fused-reps", type=int, default=20)
    ap.add_argument("--matches", type=int, default=2000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("init_stage_timing needs the GPU: there is nothing to time without one")
    dev = torch.device("cuda")
    halve_at = tuple(a.iters * k // 4 for k in (1, 2, 3))
    res = {"device": torch.cuda.get_device_name(0), "iters": a.iters, "halve_at": halve_at, "rounds": a.rounds,
           "fused_reps_per_round": a.fused_reps, "matches_per_ordered_pair": a.matches, "image": [W, H]}
    for n_views in (3, 4):
        base = make_view_gs(n_views, a.matches, seed=n_views, device=dev)
        warm = max(20, a.iters // 50)                             # every shape and code object once
        leg_torch(base, warm, ())
        leg_loss_op(base, warm, ())
        leg_fused(base, a.iters, halve_at, 2)
        t = {"torch_loop": [], "loss_op_arena": [], "run_schedule": []}
        ends = {}
        for _ in range(a.rounds):
            for name, fn in (("torch_loop", lambda: leg_torch(base, a.iters, halve_at)),
                             ("loss_op_arena", lambda: leg_loss_op(base, a.iters, halve_at)),
                             ("run_schedule", lambda: leg_fused(base, a.iters, halve_at, a.fused_reps))):
                dt, best = fn()
                t[name].append(dt)
                ends[name] = best
        tag = f"views{n_views}"
        res[tag] = {"depths": int(ends["run_schedule"].numel())}
        for name, v in t.items():
            res[tag][name + "_s"] = round(statistics.median(v), 6)
            res[tag][name + "_s_all"] = [round(x, 6) for x in v]
        res[tag]["torch_loop_over_run_schedule"] = round(res[tag]["torch_loop_s"] / res[tag]["run_schedule_s"], 1)
        res[tag]["loss_op_arena_over_run_schedule"] = round(res[tag]["loss_op_arena_s"] / res[tag]["run_schedule_s"], 1)
        # the legs do the same work: how many best depths agree to 1e-3 (Adam's rounding differs: the few matches that sit on a
        # kink of their L1 term at some iteration may part ways)
        for name in ("torch_loop", "loss_op_arena"):
            d = (ends[name].reshape(-1) - ends["run_schedule"].reshape(-1)).abs()
            res[tag][f"best_z_share_within_1e-3_of_{name}"] = round(float((d <= 1e-3).float().mean()), 4)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()

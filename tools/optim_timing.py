#!/usr/bin/env python3
"""What the optimizer step and the densification statistics cost (profiles/r07_optim_*).  Prints ONE JSON object.

(a) the optimizer step alone: the reference's two Adam optimizers (twelve groups, scene/gaussian_model.py:496-512) over
    syn.make_raw_model parameters at S1 (10 k Gaussians) and S2 (200 k), SH degree 0 / 1 / 3 (features_rest gradients zero beyond
    the active degree's columns): host + GPU wall time per iteration of torch's default Adam, torch fused=True and ArenaAdam.
(b) a whole S1 iteration (render() + fused image loss + backward + Adam + densification statistics) in four forms: eager with
    torch's fused Adam; captured step + eager ArenaAdam; everything captured with ArenaAdam; everything captured with torch's
    capturable fused Adam.

    python tools/optim_timing.py [--part a|b|ab] [--iters 200] [--only arena|fused|default] [--sizes S1,S2] [--degrees 0,1,3]

--only runs one implementation of (a) (for a `rocprofv3 --kernel-trace --stats` run of its kernels)."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import scgaussian_amd                                                                       # noqa: E402
from scgaussian_amd import losses, optim, synthetic as syn                                  # noqa: E402

RAY = [("zval", 1.6e-4), ("features_dc", 2.5e-3), ("features_rest", 1.25e-4), ("opacity", 5e-2), ("scaling", 5e-3),
       ("rotation", 1e-3)]
BG = [("bg_xyz", 1.6e-4), ("bg_features_dc", 2.5e-3), ("bg_features_rest", 1.25e-4), ("bg_opacity", 5e-2),
      ("bg_scaling", 5e-3), ("bg_rotation", 1e-3)]
SIZES = {"S1": 10_000, "S2": 200_000}


def make_opts(model, kind):
    def groups(spec):
        return [{"params": [getattr(model, a)], "lr": lr, "name": a} for a, lr in spec]
    if kind == "arena":
        return [optim.ArenaAdam(groups(s), lr=0.0, eps=1e-15) for s in (RAY, BG)]
    kw = {"fused": True} if kind == "fused" else ({"fused": True, "capturable": True} if kind == "fused_capturable" else {})
    return [torch.optim.Adam(groups(s), lr=0.0, eps=1e-15, **kw) for s in (RAY, BG)]


def part_a(sizes, degrees, iters, only):
    out = {}
    for sz in sizes:
        P = SIZES[sz]
        sc = syn.make_scene(P, 64, 64, seed=0)
        for deg in degrees:
            cols = 3 * ((deg + 1) ** 2 - 1)
            for kind in ([only] if only else ["default", "fused", "arena"]):
                model = syn.make_raw_model(sc).to("cuda").requires_grad_()
                for p in model.parameters():
                    p.grad = torch.randn_like(p) * 1e-3
                    if p.dim() == 3 and p.shape[1] > 1:
                        p.grad.view(p.shape[0], -1)[:, cols:] = 0
                opts = make_opts(model, kind)
                for _ in range(10):
                    for o in opts:
                        o.step()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(iters):
                    for o in opts:
                        o.step()
                torch.cuda.synchronize()
                ms = (time.perf_counter() - t0) / iters * 1e3
                out[f"{sz}_deg{deg}_{kind}_ms"] = round(ms, 4)
                del opts, model
    return out


def part_b(iters):
    from scgaussian_amd.graph_step import CapturedStep
    from scgaussian_amd.render import PipelineParams, render
    scgaussian_amd.single_gpu_host_setup()
    dev = torch.device("cuda")
    P, W, H = 10_000, 256, 256
    gt = syn.make_scene(P, W, H, seed=0, log_scale_mean=-3.3)
    cams = [c.to(dev) for c in (syn.default_camera(W, H), syn.orbit_camera(W, H, 8.0, 0.0, 7.0),
                                syn.orbit_camera(W, H, -8.0, 3.0, 7.0))]
    pipe, bg = PipelineParams(), torch.zeros(3, device=dev)
    truth = syn.make_raw_model(gt).to(dev)
    with torch.no_grad():
        targets = [render(c, truth, pipe, bg)["render"].clone() for c in cams]
    out = {}
    for form in ("eager_torch_fused", "captured_step_eager_arena", "all_captured_arena", "all_captured_torch_fused"):
        model = syn.make_raw_model(gt).to(dev).requires_grad_()
        model.active_sh_degree = 3
        params = model.parameters()
        kind = {"eager_torch_fused": "fused", "captured_step_eager_arena": "arena", "all_captured_arena": "arena",
                "all_captured_torch_fused": "fused_capturable"}[form]
        opts = make_opts(model, kind)
        max_r = torch.zeros(P, device=dev)
        acc = torch.zeros(P, 1, device=dev)
        den = torch.zeros(P, 1, device=dev)
        in_graph = form.startswith("all_captured")

        def stats(pkg):
            g2d, radii = pkg["viewspace_points"].grad, pkg["radii"]
            if kind == "arena":
                optim.densification_stats(max_r, acc, den, g2d, radii)
            elif in_graph:                                        # capturable torch form (no boolean indexing)
                vis = radii > 0
                acc.add_(torch.where(vis[:, None], torch.norm(g2d[:, :2], dim=-1, keepdim=True), 0.0))
                den.add_(vis[:, None].float())
                torch.maximum(max_r, torch.where(vis, radii.float(), 0.0), out=max_r)
            else:                                                 # the reference's form (train.py:191-192)
                vis = radii > 0
                max_r[vis] = torch.max(max_r[vis], radii[vis].float())
                acc[vis] += torch.norm(g2d[vis, :2], dim=-1, keepdim=True)
                den[vis] += 1

        def fn_of(v, with_opt):
            def fn():
                pkg = render(cams[v], model, pipe, bg)
                loss = losses.image_loss(pkg["render"], targets[v], 0.2)
                loss.backward()
                if with_opt:
                    stats(pkg)
                    for o in opts:
                        o.step()
                    return loss
                return loss, pkg
            return fn
        if in_graph:
            for p in params:                                      # state before the capture (a step on zero gradients)
                p.grad = torch.zeros_like(p)
            for o in opts:
                o.step()
                for st in o.state.values():
                    st["step"].zero_()
                if kind == "arena":
                    o.sync_hyperparameters()
            for v in range(3):
                for _ in range(3):
                    for p in params:
                        p.grad = None
                    fn_of(v, False)()
            steps = [CapturedStep(fn_of(v, True), params=params, warmup=0) for v in range(3)]
        elif form == "captured_step_eager_arena":
            steps = [CapturedStep(fn_of(v, False), params=params) for v in range(3)]
        else:
            steps = None

        def one(it):
            v = it % 3
            if in_graph:
                steps[v].replay()
            elif steps is not None:
                _loss, pkg = steps[v].replay()
                stats(pkg)
                for o in opts:
                    o.step()
            else:
                for o in opts:
                    o.zero_grad(set_to_none=True)
                _loss, pkg = fn_of(v, False)()
                stats(pkg)
                for o in opts:
                    o.step()
        for it in range(30):
            one(it)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for it in range(iters):
            one(it)
        torch.cuda.synchronize()
        out[f"S1_iter_{form}_ms"] = round((time.perf_counter() - t0) / iters * 1e3, 4)
        if steps is not None:
            out[f"S1_iter_{form}_overflows"] = sum(s.overflows for s in steps)
            for s in steps:
                s.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="ab")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--only", default=None)
    ap.add_argument("--sizes", default="S1,S2")
    ap.add_argument("--degrees", default="0,1,3")
    a = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0)}
    if "a" in a.part:
        res.update(part_a(a.sizes.split(","), [int(d) for d in a.degrees.split(",")], a.iters, a.only))
    if "b" in a.part:
        res.update(part_b(a.iters))
    print(json.dumps(res))


if __name__ == "__main__":
    main()

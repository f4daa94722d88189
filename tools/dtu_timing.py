#!/usr/bin/env python3
"""What the DTU-only part of a training iteration costs (profiles/r10_dtu_timing.json).  Prints ONE JSON object and writes it to --out.

One process, warm, every call synchronised on both sides, median of --calls calls per leg (the protocol of tools/densify_timing.py),
at 1600 x 1200 (DTU's native size) and 400 x 300.  Per size, forward AND backward of
  torch_restatement   train.py:149-158 + :167-168 in plain torch (tests/dtu_refs.py): the mask loop, the boolean-index write, the
                      boolean-index mean and its backward
  hip_mask_per_iter   dtu.background_mask(inplace) + dtu.alpha_term, the mask rebuilt every iteration as the reference does
  hip_view_once       dtu.alpha_term on a dtu.DtuView built once per camera
and the evaluation metrics of train.py:252-265: plain torch (clamp, two boolean gathers, l1, psnr) against dtu.eval_metrics.
Last, a captured training step (graph_step.CapturedStep, 10 000 Gaussians at 256 x 256) with losses.image_loss alone and with
dtu.training_loss: what the DTU terms add to a replay.

    python tools/dtu_timing.py [--calls 25] [--out profiles/r10_dtu_timing.json]"""
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
import dtu_refs as DR                                                                        # noqa: E402
from scgaussian_amd import dtu, graph_step, losses, rasterizer as R, synthetic as syn        # noqa: E402

SIZES = {"1600x1200": (1200, 1600), "400x300": (300, 400)}
DEV = "cuda"


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


def scene_image(H, W, seed=0):
    """An object on a dark background: bright inside an ellipse, dark (under the threshold) outside."""
    g = torch.Generator().manual_seed(seed)
    y, x = torch.meshgrid(torch.linspace(-1, 1, H), torch.linspace(-1, 1, W), indexing="ij")
    inside = (x / 0.6) ** 2 + (y / 0.75) ** 2 < 1
    img = torch.where(inside[None], torch.rand(3, H, W, generator=g) * 0.7 + 0.2, torch.rand(3, H, W, generator=g) * 0.04)
    return img.to(DEV)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=25)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r10_dtu_timing.json"))
    a = ap.parse_args()
    assert a.calls >= 20
    res = {"device": torch.cuda.get_device_name(0), "calls": a.calls,
           "what": "median ms per call (forward + backward), one process, warm, synchronised around each call"}
    for tag, (H, W) in SIZES.items():
        gt0 = scene_image(H, W)
        alpha = torch.rand(1, H, W, device=DEV, requires_grad=True)
        view = dtu.DtuView(gt0)
        res[f"{tag}_masked_share"] = round(float(view.count) / (H * W), 4)

        def torch_leg():
            alpha.grad = None
            bg_mask, _gt, _n = DR.bg_mask_loop(gt0)
            alpha[bg_mask].mean().backward()

        def hip_per_iter():
            alpha.grad = None
            v = dtu.DtuView(gt0.clone(), inplace=True)        # (the image is cloned in both legs: the restatement clones it too)
            dtu.alpha_term(alpha, v).backward()

        def hip_once():
            alpha.grad = None
            dtu.alpha_term(alpha, view).backward()
        for leg, fn in (("torch_restatement", torch_leg), ("hip_mask_per_iter", hip_per_iter), ("hip_view_once", hip_once)):
            res[f"{tag}_{leg}_ms"], res[f"{tag}_{leg}_min_ms"] = median_ms(fn, a.calls)
        res[f"{tag}_per_iter_speedup"] = round(res[f"{tag}_torch_restatement_ms"] / res[f"{tag}_hip_mask_per_iter_ms"], 2)
        res[f"{tag}_view_once_speedup"] = round(res[f"{tag}_torch_restatement_ms"] / res[f"{tag}_hip_view_once_ms"], 2)
        # evaluation metrics under a mask
        img = (gt0 + 0.1 * torch.randn_like(gt0))
        dtumask = (gt0.max(0).values > 0.1).float() * 255.0

        def torch_metrics():
            image, gt_image = torch.clamp(img, 0.0, 1.0), torch.clamp(gt0, 0.0, 1.0)
            mask = dtumask > 0
            p, q = image[:, mask], gt_image[:, mask]
            l1 = torch.abs(p - q).mean().mean().double()
            mse = ((p - q) ** 2).view(p.shape[0], -1).mean(1, keepdim=True)
            return l1, (20 * torch.log10(1.0 / torch.sqrt(mse))).mean().double()
        res[f"{tag}_metrics_torch_ms"], _ = median_ms(torch_metrics, a.calls)
        res[f"{tag}_metrics_hip_ms"], _ = median_ms(lambda: dtu.eval_metrics(img, gt0, dtumask), a.calls)
        res[f"{tag}_metrics_speedup"] = round(res[f"{tag}_metrics_torch_ms"] / res[f"{tag}_metrics_hip_ms"], 2)
    # a captured step with and without the DTU terms
    import math
    P, W, H = 10_000, 256, 256
    sc = syn.make_scene(P, W, H, seed=1)
    cam = syn.orbit_camera(W, H, 3.0, -2.0, 7.0).to(DEV)
    st = R.GaussianRasterizationSettings(H, W, math.tan(cam.FoVx / 2), math.tan(cam.FoVy / 2), torch.zeros(3, device=DEV), 1.0,
                                         cam.world_view_transform, cam.full_proj_transform, 3, cam.camera_center, False, False)
    rast = R.GaussianRasterizer(st)
    leaves = [t.detach().clone().to(DEV).requires_grad_(True) for t in (sc.means3D, sc.shs, sc.opacities, sc.scales, sc.rotations)]

    def render():
        m, f, o, s, r = leaves
        c, _radii, _d, al = rast(means3D=m, means2D=torch.zeros_like(m, requires_grad=True), opacities=o, shs=f, scales=s, rotations=r)
        return c, al
    with torch.no_grad():
        c0, _ = render()
    gt = (c0 * 0.7 + 0.2).clamp(0, 1)
    gt[:, :100, 32:224] = 0.02
    view = dtu.DtuView(gt)

    def plain():
        c, _al = render()
        loss = losses.image_loss(c, view.gt, 0.2)
        loss.backward()
        return loss

    def with_dtu():
        c, al = render()
        loss = dtu.training_loss(c, al, view)
        loss.backward()
        return loss
    for leg, fn in (("captured_step_image_loss", plain), ("captured_step_dtu_loss", with_dtu)):
        step = graph_step.CapturedStep(fn, params=leaves)
        res[f"{leg}_ms"], res[f"{leg}_min_ms"] = median_ms(step.replay, max(a.calls, 100), warm=10)
        step.close()
    res["captured_step_workload"] = f"{P} Gaussians at {W}x{H}, masked share {round(float(view.count) / (H * W), 4)}"
    text = json.dumps(res)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Recover a perturbed camera pose with the rasterizer's camera gradients: the Gaussians of synthetic.py's scene stay fixed, a
`CameraPose` wraps the perturbed camera and `torch.optim.Adam` moves its 6-vector `delta` until the render matches the image of the
true camera.

    python examples/fit_pose.py [--iters 60] [--gaussians 80]

`delta` requires grad, so GaussianRasterizer routes the call through camera_grad.py's node: viewmatrix.grad, projmatrix.grad and
campos.grad come out of two extra launches per backward, and torch carries them through the pose algebra to `delta.grad`.
tests/test_gpu_camgrad.py drives this very loop twice, with the CPU oracle and with the kernels (`rasterize`)."""
import argparse
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from scgaussian_amd import synthetic as syn                                                    # noqa: E402
from scgaussian_amd.pose import CameraPose                                                     # noqa: E402

PERTURBATION = (0.02, -0.03, 0.015, 0.05, -0.04, 0.06)       # (omega, upsilon): 2.3 degrees and 0.09 scene units


def rasterize_hip(cam, sc, bg, deg=3):
    """The colour image of scene `sc` from `cam` (anything with a camera's attributes) through the HIP rasterizer."""
    from diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer
    st = GaussianRasterizationSettings(cam.image_height, cam.image_width, math.tan(cam.FoVx / 2), math.tan(cam.FoVy / 2), bg, 1.0,
                                       cam.world_view_transform, cam.full_proj_transform, deg, cam.camera_center, False, False)
    return GaussianRasterizer(st)(means3D=sc.means3D, means2D=torch.zeros_like(sc.means3D), opacities=sc.opacities, shs=sc.shs,
                                  scales=sc.scales, rotations=sc.rotations)[0]


def pose_error(pose_cam: CameraPose, true_cam) -> float:
    """sqrt(angle^2 + |t' - t|^2) between the wrapper's pose and the true camera's, in fp64 on the host."""
    R, t = (x.detach().double().cpu() for x in pose_cam.pose())
    wv = true_cam.world_view_transform.detach().double().cpu()
    dR = R @ wv[:3, :3]                                      # R' R_true^T (the upper 3x3 of world_view_transform is R_true^T)
    angle = math.acos(max(-1.0, min(1.0, (float(dR.trace()) - 1.0) / 2.0)))
    return math.sqrt(angle ** 2 + float(((t - wv[3, :3]) ** 2).sum()))


def fit(iters=60, P=80, W=40, H=24, seed=2, lr=1e-2, rasterize=rasterize_hip, dev="cuda", verbose=True):
    """Returns (initial pose error, [(iteration, loss, pose error)], final pose error)."""
    dev = torch.device(dev)
    sc = syn.make_scene(P, W, H, seed=seed, log_scale_mean=-1.5).to(dev)
    true_cam = syn.orbit_camera(W, H, 6.0, -4.0, 7.0).to(dev)
    bg = torch.tensor([0.1, 0.2, 0.3], device=dev)
    with torch.no_grad():
        target = rasterize(true_cam, sc, bg)
    cam = CameraPose(true_cam)
    with torch.no_grad():
        cam.delta.copy_(torch.tensor(PERTURBATION, device=dev))
    cam.retract()                                            # the perturbed pose is the base; delta starts at zero
    e0 = pose_error(cam, true_cam)
    opt = torch.optim.Adam([cam.delta], lr=lr)
    history = []
    for it in range(iters):
        opt.zero_grad(set_to_none=True)
        loss = ((rasterize(cam, sc, bg) - target) ** 2).mean()
        loss.backward()
        opt.step()
        if it % 10 == 0 or it == iters - 1:
            history.append((it, float(loss.detach()), pose_error(cam, true_cam)))
            if verbose:
                print(f"iter {it:3d}  loss {history[-1][1]:.3e}  pose error {history[-1][2]:.5f}  (initial {e0:.5f})")
    return e0, history, pose_error(cam, true_cam)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=60)
    ap.add_argument("--gaussians", type=int, default=80)
    a = ap.parse_args()
    fit(a.iters, a.gaussians)

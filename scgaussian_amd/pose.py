"""A camera whose pose can be refined: `CameraPose(camera)` wraps a reference `Camera` (scene/cameras.py; or a
synthetic.CameraRecord) and puts a 6-vector `delta = (omega, upsilon)` in front of its world-to-camera pose (R0, t0):

    R' = Exp(omega) . R0        t' = t0 + upsilon

`world_view_transform`, `full_proj_transform = world_view_transform @ projection_matrix` and `camera_center = -R'^T t'` are
recomputed from `delta` on its device at every read, in torch, without `inverse()` and without a host read; every other attribute
is the wrapped camera's, so `render(pose_cam, gaussians, pipe, bg)` works as it stands and — `delta` being a parameter that requires
grad — goes through the rasterizer's camera-gradient nodes (camera_grad.py): `delta.grad` after `loss.backward()`.
`retract()` folds `delta` into (R0, t0) and zeroes it: the three matrices do not change.

The matrices are new tensors at every read; the wrapper names them with `tag_camera`, so the rasterizer keys its per-camera
history by that name and never reads a matrix back to identify the camera.  The dozen small launches each way stay in torch.

Exp is Rodrigues' formula, R = I + A K + B K^2 with K = [omega]x, A = sin(th) / th, B = (1 - cos(th)) / th^2 = (sin(th/2) / (th/2))^2 / 2
(the half-angle form has no cancellation: its fp32 error is a few ulp at every angle).  Below th = SERIES_BELOW both factors come
from their series in th^2 (four terms), which needs no square root and so has a finite gradient at omega = 0.  The switch-over sits
where the two branches' fp32 errors meet: the series' truncation error, th^8 / 362880 for A and th^8 / 1814400 for B, reaches the
direct form's rounding error (about 1e-7) at th = 0.66 and 0.81; at 0.5 it is 1e-8, below one ulp, so both branches are at rounding
level on either side (tests/test_camgrad_cpu.py measures both against fp64 there).
"""
from __future__ import annotations

import torch
import torch.nn as nn

from ._cameras import tag_camera

SERIES_BELOW = 0.5                       # radians


def _hat(w):
    """[w]x as (3,3), differentiable."""
    z = torch.zeros((), dtype=w.dtype, device=w.device)
    return torch.stack([z, -w[2], w[1], w[2], z, -w[0], -w[1], w[0], z]).reshape(3, 3)


def so3_exp(omega: torch.Tensor) -> torch.Tensor:
    """Exp(omega) (3,3) of a rotation vector (3,): see the module docstring.  No data-dependent branch: no host read."""
    s = (omega * omega).sum()                                                # th^2
    small = s < SERIES_BELOW * SERIES_BELOW
    a_series = 1.0 - s / 6.0 * (1.0 - s / 20.0 * (1.0 - s / 42.0))          # 1 - s/6 + s^2/120 - s^3/5040
    b_series = 0.5 - s / 24.0 * (1.0 - s / 30.0 * (1.0 - s / 56.0))         # 1/2 - s/24 + s^2/720 - s^3/40320
    th = torch.sqrt(torch.where(small, torch.ones_like(s), s))               # (the branch not taken sees th = 1: finite everywhere)
    half = 0.5 * th
    sh = torch.sin(half) / half
    a = torch.where(small, a_series, torch.sin(th) / th)
    b = torch.where(small, b_series, 0.5 * sh * sh)
    K = _hat(omega)
    return torch.eye(3, dtype=omega.dtype, device=omega.device) + a * K + b * (K @ K)


class CameraPose(nn.Module):
    def __init__(self, camera):
        super().__init__()
        object.__setattr__(self, "_camera", camera)                          # (not a submodule: its tensors are not this module's)
        wv = camera.world_view_transform.detach().to(torch.float32)
        dev = wv.device
        # world_view_transform is the transposed world-to-camera matrix: its upper 3x3 is R0^T, its last row t0
        self.register_buffer("R0", wv[:3, :3].t().contiguous().clone())
        self.register_buffer("t0", wv[3, :3].contiguous().clone())
        proj = getattr(camera, "projection_matrix", None)
        if proj is None:
            from .synthetic import projection_matrix
            proj = projection_matrix(camera.znear, camera.zfar, camera.FoVx, camera.FoVy).transpose(0, 1)
        self.register_buffer("projection", proj.detach().to(dev, torch.float32).contiguous().clone())
        self.delta = nn.Parameter(torch.zeros(6, dtype=torch.float32, device=dev))
        self._name = ("pose", getattr(camera, "uid", None), id(self))

    def __getattr__(self, name):
        try:
            return super().__getattr__(name)                                 # parameters, buffers
        except AttributeError:
            return getattr(self.__dict__["_camera"], name)                   # everything else passes through

    def pose(self):
        """(R' (3,3), t' (3,)) world-to-camera, differentiable by delta."""
        R = so3_exp(self.delta[:3]) @ self.R0
        return R, self.t0 + self.delta[3:]

    @property
    def world_view_transform(self):
        R, t = self.pose()
        top = torch.cat([R.t(), torch.zeros(3, 1, dtype=R.dtype, device=R.device)], 1)
        row = torch.cat([t, torch.ones(1, dtype=R.dtype, device=R.device)])[None]
        return tag_camera(torch.cat([top, row], 0), self._name)

    @property
    def projection_matrix(self):
        return self.projection

    @property
    def full_proj_transform(self):
        return self.world_view_transform @ self.projection

    @property
    def camera_center(self):
        R, t = self.pose()
        return -(R.t() @ t)

    @torch.no_grad()
    def retract(self):
        """Fold delta into the base pose and zero it."""
        R, t = self.pose()
        self.R0.copy_(R)
        self.t0.copy_(t)
        self.delta.zero_()
        return self

    def to_record(self):
        """The current pose as a synthetic.CameraRecord of detached tensors (tests, tools)."""
        from .synthetic import CameraRecord
        with torch.no_grad():
            return CameraRecord(int(self.image_height), int(self.image_width), float(self.FoVx), float(self.FoVy),
                                self.world_view_transform.clone(), self.full_proj_transform.clone(), self.camera_center.clone(),
                                float(getattr(self, "znear", 0.01)), float(getattr(self, "zfar", 100.0)))

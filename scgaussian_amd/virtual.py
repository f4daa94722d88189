"""The two sparse-view regularisers of utils/loss_utils.py on the GPU, forward and backward (csrc/virtualwarp.hip, libscg_vw.so,
include/vw/scg_virtualwarp.h), and the host arithmetic that goes with them:

    VirtualWarp(intrs, w2cs, img_colors)       owns the planar colours (nv,3,H,W), the matrix records and the scratch
      .from_view_gs(view_gs) / .from_mono(setup)   the same from the reference's dictionary (image_color (h,w,3) permuted once)
      .set_pose(vir_c2w, intr=None)            composes M_v = K_v R_v R_vir K_0^-1 and t_v = K_v (R_v t_vir + t_v) in fp64 on the host,
                                               rounds once and writes the records through one pinned copy, in place
      .loss(virtual_img, virtual_depth, vir_mask)   get_virtual_warp_loss (:208-246): 3 launches forward, 1 backward
      .loss_map, .winner, .in_bounds           by-products of the last call
    virtual_warp_loss(...)                     the reference's signature
    smooth_loss(depth, guide=None)             get_smooth_loss (:19-38): 2 launches forward, 1 backward
    near_virtual_pose(c2ws, near_far, rng)     utils/virtual_poses.py:151-179 on the host
    virtual_camera(c2w, like=cam)              a camera record render.render accepts
    install(loss_utils)                        rebinds get_virtual_warp_loss and get_smooth_loss

The scratch holds what the forward leaves for the backward (the warped images, the sampler's depth derivative, the winning view's
coefficient maps): a loss's backward must run before the same VirtualWarp's next forward, as in a training step; anything else
raises.  CPU tensors go through the plain-torch twins below (warp_loss_torch, smooth_loss_torch), which also serve as the
restatement the tests and tools/virtualwarp_timing.py run on the device.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

from . import _lib, _lib_vw, synthetic
from ._lib import ScgError

MAX_VIEWS = _lib_vw.VW_MAX_VIEWS
_WHAT = "the virtual-view losses"


def _err(msg: str) -> ScgError:
    return ScgError(f"virtual: {msg}")


# ---- host arithmetic ------------------------------------------------------------------------------------------------------------
def compose_records(intrs, w2cs, vir_c2w, intr=None, dtype=np.float32) -> np.ndarray:
    """(nv,12) fp32: per view M_v (row major) and t_v, composed in fp64 from the fp32 inputs and rounded once (dtype=np.float64:
    not rounded, for the tests)."""
    K = np.asarray(intrs, dtype=np.float64)[:, :3, :3]
    E = np.asarray(w2cs, dtype=np.float64)
    c2w = np.asarray(vir_c2w, dtype=np.float64)
    if K.ndim != 3 or E.shape != (K.shape[0], 4, 4) or c2w.shape[-1] != 4 or c2w.shape[0] < 3:
        raise _err("intrs must be (nv,3,3), w2cs (nv,4,4) and vir_c2w (3,4)")
    K0 = K[0] if intr is None else np.asarray(intr, dtype=np.float64)[:3, :3]
    K0i = np.linalg.inv(K0)
    R, t = E[:, :3, :3], E[:, :3, 3]
    M = K @ R @ c2w[:3, :3] @ K0i
    tv = np.einsum("vij,vj->vi", K, np.einsum("vij,j->vi", R, c2w[:3, 3]) + t)
    return np.concatenate([M.reshape(-1, 9), tv], axis=1).astype(dtype)


def _unit(v):
    return v / np.linalg.norm(v)


def _look(lookdir, up, position):
    z = _unit(lookdir)
    x = _unit(np.cross(up, z))
    y = _unit(np.cross(z, x))
    return np.stack([x, y, z, position], axis=1)


def near_virtual_pose(c2ws, near_far, rng=np.random) -> np.ndarray:
    """A random pose near the training cameras, (3,4) camera-to-world: the average camera displaced by up to the cameras' largest
    coordinate per axis, looking at the focus point of the depth range (utils/virtual_poses.py:151-179).  rng: anything with
    rand(n) (numpy.random, a RandomState): three numbers are drawn."""
    poses = np.asarray(c2ws)
    nf = np.array(near_far)
    close, far = nf.min() * .9, nf.max() * 2.
    dt = .75
    focal = 1 / ((1 - dt) / close + dt / far)
    radii = np.concatenate([np.abs(poses[:, :3, 3]).max(0), [1.]])
    up = poses[:, :3, 1].mean(0)
    avg = _look(poses[:, :3, 2].mean(0), up, poses[:, :3, 3].mean(0))
    t = radii * np.concatenate([2 * rng.rand(3) - 1., [1, ]])
    position = avg @ t
    lookat = avg @ [0, 0, -focal, 1.]
    return _look(position - lookat, up, position)


def virtual_camera(c2w, like):
    """The camera record of the pose `c2w` ((3,4) or (4,4), camera to world) with the size and field of view of `like`: matrices as
    scene/cameras.py:60-63 builds them (synthetic.make_camera), on the device of like's."""
    m = np.eye(4)
    m[:3, :4] = np.asarray(c2w, dtype=np.float64)[:3, :4]
    w2c = np.linalg.inv(m)
    cam = synthetic.make_camera(w2c[:3, :3].T, w2c[:3, 3], float(like.FoVx), float(like.FoVy), int(like.image_width),
                                int(like.image_height), float(getattr(like, "znear", 0.01)), float(getattr(like, "zfar", 100.0)))
    return cam.to(like.world_view_transform.device)


# ---- the plain-torch twins ------------------------------------------------------------------------------------------------------
def _box_ssim_term(x, y):
    """clamp((1 - SSIM_n / SSIM_d) / 2, 0, 1) with 5x5 means behind a reflection pad of 2: x (1,3,H,W), y (nv,3,H,W)."""
    pool = lambda t: F.avg_pool2d(F.pad(t, (2, 2, 2, 2), mode="reflect"), 5, 1)      # noqa: E731
    mx, my = pool(x), pool(y)
    sx, sy, sxy = pool(x * x) - mx * mx, pool(y * y) - my * my, pool(x * y) - mx * my
    n = (2 * mx * my + 0.01 ** 2) * (2 * sxy + 0.03 ** 2)
    d = (mx * mx + my * my + 0.01 ** 2) * (sx + sy + 0.03 ** 2)
    return torch.clamp((1 - n / d) / 2, 0, 1)


def warp_loss_torch(virtual_img, virtual_depth, vir_mask, img_colors, records):
    """The rule of include/vw/scg_virtualwarp.h in torch operators, differentiable by autograd, in the dtype and on the device of
    virtual_img.  Returns (loss, loss_map (H,W), winner (H,W) int8, in_bounds (nv,H,W) bool)."""
    dt, dev = virtual_img.dtype, virtual_img.device
    H, W = virtual_img.shape[-2:]
    nv = img_colors.shape[0]
    rec = records.to(dev, dt).reshape(nv, 12)
    py, px = torch.meshgrid(torch.arange(H, device=dev, dtype=dt), torch.arange(W, device=dev, dtype=dt), indexing="ij")
    pix = torch.stack([px.reshape(-1), py.reshape(-1), torch.ones(H * W, device=dev, dtype=dt)])
    a = rec[:, :9].reshape(nv, 3, 3) @ pix
    xyz = virtual_depth.reshape(1, 1, -1) * a + rec[:, 9:].reshape(nv, 3, 1)
    xy = xyz[:, :2] / (xyz[:, 2:] + 1e-8)
    grid = torch.stack([2 * xy[:, 0] / (W - 1) - 1, 2 * xy[:, 1] / (H - 1) - 1], dim=-1).unsqueeze(1)
    inb = (grid.abs() <= 1).all(dim=-1).reshape(nv, H, W)
    # a NaN coordinate, or one whose tap does not fit an int32, samples zero: the kernels' rule where torch's samplers differ
    fits = (((grid + 1) * torch.tensor([W, H], device=dev, dtype=dt) - 1) / 2).abs() < 2.0 ** 31
    grid = torch.where(fits, grid, torch.full_like(grid, -1e6))
    warp = F.grid_sample(img_colors.to(dt), grid, mode="bilinear", padding_mode="zeros", align_corners=False).reshape(nv, 3, H, W)
    s = _box_ssim_term(virtual_img.reshape(1, 3, H, W), warp).mean(dim=1)
    s = torch.where(inb, s, torch.full_like(s, 1000.0))
    low = s.detach().amin(dim=0)
    idx = torch.arange(nv, device=dev).reshape(nv, 1, 1)
    hit = (s.detach() == low) | (s.detach().isnan() & low.isnan())
    w = torch.where(hit, idx, nv).amin(dim=0).clamp_max(nv - 1)      # the lowest index attaining the minimum; the first NaN (torch.min)
    best = s.gather(0, w.unsqueeze(0))[0]
    none = (best.detach() >= 1000) | ~vir_mask.reshape(H, W).to(torch.bool)
    loss_map = torch.where(none, torch.zeros_like(best), best)
    return loss_map.mean(), loss_map.detach(), torch.where(none, -1, w).to(torch.int8), inb


def smooth_loss_torch(depth, guide=None):
    """get_smooth_loss in torch operators (the CPU twin)."""
    dx = (depth[:, :-1] - depth[:, 1:]).abs()
    dy = (depth[:-1, :] - depth[1:, :]).abs()
    if guide is not None:
        g = guide.detach()
        if g.dim() == 3:
            gx, gy = (g[:, :, :-1] - g[:, :, 1:]).abs().mean(dim=0), (g[:, :-1, :] - g[:, 1:, :]).abs().mean(dim=0)
        else:
            gx, gy = (g[:, :-1] - g[:, 1:]).abs(), (g[:-1, :] - g[1:, :]).abs()
        dx, dy = dx * torch.exp(-gx), dy * torch.exp(-gy)
    return dx.mean() + dy.mean()


# ---- the kernels ----------------------------------------------------------------------------------------------------------------
class _WarpLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, virtual_img, virtual_depth, warp, mask):
        H, W, nv, dev = warp.H, warp.W, warp.nv, warp.device
        img = virtual_img.detach().to(torch.float32).contiguous()
        depth = virtual_depth.detach().to(torch.float32).reshape(H, W).contiguous()
        stream = _lib.stream_of(img, _WHAT)
        with torch.cuda.device(dev):
            loss = torch.empty((), dtype=torch.float32, device=dev)
            warp.loss_map = torch.empty((H, W), dtype=torch.float32, device=dev)
            warp.winner = torch.empty((H, W), dtype=torch.int8, device=dev)
            warp.in_bounds = torch.empty((nv, H, W), dtype=torch.uint8, device=dev)
            _lib_vw.check(_lib_vw.load().scg_vw_warp_forward(
                nv, H, W, img.data_ptr(), depth.data_ptr(), mask.data_ptr(), warp.colors.data_ptr(), warp.records.data_ptr(),
                loss.data_ptr(), warp.loss_map.data_ptr(), warp.winner.data_ptr(), warp.in_bounds.data_ptr(),
                warp.scratch.data_ptr(), warp.scratch.numel() * 4, stream), "scg_vw_warp_forward")
        warp._generation += 1
        ctx.warp, ctx.generation, ctx.winner, ctx.depth_shape = warp, warp._generation, warp.winner, tuple(virtual_depth.shape)
        ctx.save_for_backward(img)
        return loss

    @staticmethod
    def backward(ctx, grad):
        warp = ctx.warp
        if ctx.generation != warp._generation:
            raise _err("this VirtualWarp ran another forward since: its scratch no longer holds this loss's warp")
        img, = ctx.saved_tensors
        H, W, dev = warp.H, warp.W, warp.device
        up = grad.detach().to(torch.float32).reshape(1).contiguous()
        with torch.cuda.device(dev):
            d_img = torch.empty((3, H, W), dtype=torch.float32, device=dev)
            d_depth = torch.empty((H, W), dtype=torch.float32, device=dev)
            _lib_vw.check(_lib_vw.load().scg_vw_warp_backward(
                warp.nv, H, W, img.data_ptr(), up.data_ptr(), ctx.winner.data_ptr(), warp.scratch.data_ptr(),
                warp.scratch.numel() * 4, d_img.data_ptr(), d_depth.data_ptr(), _lib.stream_of(img, _WHAT)), "scg_vw_warp_backward")
        return d_img, d_depth.reshape(ctx.depth_shape), None, None


class VirtualWarp:
    def __init__(self, intrs, w2cs, img_colors):
        if img_colors.dim() != 4 or img_colors.shape[1] != 3:
            raise _err("img_colors must be (nv,3,H,W)")
        nv, _, H, W = img_colors.shape
        if not 1 <= nv <= MAX_VIEWS:
            raise _err(f"{nv} views are outside what the kernels take (1..{MAX_VIEWS})")
        if min(H, W) < _lib_vw.VW_MIN_DIM or max(H, W) > _lib_vw.VW_MAX_DIM:
            raise _err(f"{H} x {W} pixels: height and width must be {_lib_vw.VW_MIN_DIM}..{_lib_vw.VW_MAX_DIM}")
        if tuple(intrs.shape) != (nv, 3, 3) or tuple(w2cs.shape) != (nv, 4, 4):
            raise _err(f"intrs must be ({nv},3,3) and w2cs ({nv},4,4)")
        self.nv, self.H, self.W, self.device = int(nv), int(H), int(W), img_colors.device
        self.colors = img_colors.detach().to(torch.float32).contiguous()
        self._intrs = intrs.detach().to("cpu", torch.float32).numpy()          # read once: set_pose composes on the host
        self._w2cs = w2cs.detach().to("cpu", torch.float32).numpy()
        self.records = torch.zeros((nv, 12), dtype=torch.float32, device=self.device)
        self.on_gpu = self.device.type == "cuda"
        self._staging = torch.zeros((nv, 12), dtype=torch.float32)
        self._copied = None
        self.scratch = None
        if self.on_gpu:
            self._staging = self._staging.pin_memory()
            nbytes = _lib_vw.load().scg_vw_warp_scratch_bytes(nv, H, W)
            if nbytes == 0:
                raise _err("the sizes are outside what the kernels take")
            self.scratch = torch.empty((nbytes + 3) // 4, dtype=torch.float32, device=self.device)
        self._generation = 0
        self.loss_map = self.winner = self.in_bounds = None

    @classmethod
    def from_view_gs(cls, view_gs):
        views = list(view_gs.values())
        if not views:
            raise _err("no view")
        if len({(int(v["height"]), int(v["width"])) for v in views}) != 1:
            raise _err("the views must have equal sizes")
        colors = torch.stack([v["image_color"].permute(2, 0, 1) for v in views])
        return cls(torch.stack([v["intr"].reshape(3, 3) for v in views]), torch.stack([v["w2c"].reshape(4, 4) for v in views]), colors)

    @classmethod
    def from_mono(cls, setup):
        return cls.from_view_gs(setup.view_gs)

    def set_pose(self, vir_c2w, intr=None) -> None:
        """Write the nv records for this virtual pose, in place: one pinned host-to-device copy on the current stream, no read."""
        if isinstance(vir_c2w, torch.Tensor):
            vir_c2w = vir_c2w.detach().cpu().numpy()
        if isinstance(intr, torch.Tensor):
            intr = intr.detach().cpu().numpy()
        rec = compose_records(self._intrs, self._w2cs, vir_c2w, intr)
        if self._copied is not None:
            self._copied.synchronize()             # the staging buffer's last copy has left it (a host wait; nothing is read)
        self._staging.copy_(torch.from_numpy(rec))
        self.records.copy_(self._staging, non_blocking=True)
        if self.on_gpu:
            self._copied = torch.cuda.Event()
            self._copied.record(torch.cuda.current_stream(self.device))

    def _check(self, virtual_img, virtual_depth, vir_mask):
        H, W = self.H, self.W
        if tuple(virtual_img.shape) != (3, H, W):
            raise _err(f"virtual_img must be (3,{H},{W})")
        if tuple(virtual_depth.shape) not in ((1, H, W), (H, W)):
            raise _err(f"virtual_depth must be (1,{H},{W}) or ({H},{W})")
        if vir_mask.numel() != H * W or vir_mask.dtype not in (torch.bool, torch.uint8):
            raise _err(f"vir_mask must hold {H * W} bool or uint8 elements")
        if virtual_img.device != self.device or virtual_depth.device != self.device or vir_mask.device != self.device:
            raise _err(f"the inputs must be on {self.device}, with the colours")

    def loss(self, virtual_img, virtual_depth, vir_mask):
        self._check(virtual_img, virtual_depth, vir_mask)
        if not self.on_gpu:
            loss, self.loss_map, self.winner, inb = warp_loss_torch(virtual_img, virtual_depth, vir_mask, self.colors, self.records)
            self.in_bounds = inb.to(torch.uint8)
            return loss
        mask = vir_mask.detach().reshape(-1).contiguous()
        mask = mask.view(torch.uint8) if mask.dtype == torch.bool else mask
        return _WarpLoss.apply(virtual_img, virtual_depth, self, mask)


def virtual_warp_loss(virtual_img, virtual_depth, vir_c2w, intrs, w2cs, img_colors, vir_mask):
    """get_virtual_warp_loss's signature.  Builds a VirtualWarp per call: a loop keeps one and calls set_pose / loss."""
    warp = VirtualWarp(intrs, w2cs, img_colors)
    warp.set_pose(vir_c2w)
    return warp.loss(virtual_img, virtual_depth, vir_mask)


class _SmoothLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, depth, guide):
        H, W = depth.shape
        d = depth.detach().to(torch.float32).contiguous()
        g = None if guide is None else guide.detach().to(torch.float32).contiguous()
        C_ = 0 if g is None else (1 if g.dim() == 2 else g.shape[0])
        lib = _lib_vw.load()
        nbytes = lib.scg_vw_smooth_scratch_bytes(H, W)
        if nbytes == 0:
            raise _err(f"{H} x {W} pixels are outside what the kernels take (1..{_lib_vw.VW_MAX_DIM})")
        with torch.cuda.device(d.device):
            loss = torch.empty((), dtype=torch.float32, device=d.device)
            scratch = torch.empty(nbytes // 4, dtype=torch.float32, device=d.device)
            _lib_vw.check(lib.scg_vw_smooth_forward(H, W, C_, d.data_ptr(), None if g is None else g.data_ptr(), loss.data_ptr(),
                                                    scratch.data_ptr(), nbytes, _lib.stream_of(d, _WHAT)), "scg_vw_smooth_forward")
        ctx.save_for_backward(d, g)
        ctx.C = C_
        return loss

    @staticmethod
    def backward(ctx, grad):
        d, g = ctx.saved_tensors
        H, W = d.shape
        up = grad.detach().to(torch.float32).reshape(1).contiguous()
        with torch.cuda.device(d.device):
            out = torch.empty_like(d)
            _lib_vw.check(_lib_vw.load().scg_vw_smooth_backward(H, W, ctx.C, d.data_ptr(), None if g is None else g.data_ptr(),
                                                                up.data_ptr(), out.data_ptr(), _lib.stream_of(d, _WHAT)),
                          "scg_vw_smooth_backward")
        return out, None


def smooth_loss(depth, guide=None):
    """get_smooth_loss(depth, guide): depth (H,W) only — the reference's slicing gives NaN for (1,H,W); guide None, (H,W) or (C,H,W)."""
    if depth.dim() != 2:
        raise _err(f"depth must be (H,W), not {tuple(depth.shape)}: the reference's slicing gives NaN for anything else")
    H, W = depth.shape
    if guide is not None:
        if tuple(guide.shape[-2:]) != (H, W) or guide.dim() not in (2, 3) or guide.device != depth.device:
            raise _err(f"guide must be ({H},{W}) or (C,{H},{W}) on the depth's device")
        if guide.dim() == 3 and not 1 <= guide.shape[0] <= _lib_vw.VW_MAX_GUIDE_CHANNELS:
            raise _err(f"a guide of {guide.shape[0]} channels is outside 1..{_lib_vw.VW_MAX_GUIDE_CHANNELS}")
    if not depth.is_cuda:
        return smooth_loss_torch(depth, guide)
    return _SmoothLoss.apply(depth, guide)


def install(loss_utils) -> None:
    """Rebind the two names of the reference's utils/loss_utils.py (any object with attributes) to this module's."""
    loss_utils.get_virtual_warp_loss = virtual_warp_loss
    loss_utils.get_smooth_loss = smooth_loss

"""Plain CPU references for the training-side kernels, parametrised by dtype.

Called with torch.float64 they ARE the reference of the edge-parity tests; called with torch.float32 they give the error of a
plain fp32 evaluation of the same expression (`e32`), from which those tests derive their bar:

    err_kernel <= max(4 * e32, floor)

The factor 4 covers a different but legitimate fp32 summation order (the image-loss kernel adds 11 + 11 separable taps where
conv2d adds 121; the match loss reduces its terms over waves); the floors are the bars the suite held before these tests.
tests/test_loss_refs_cpu.py pins image_loss_ref(float64) to the goldens the reference project itself produced
(tests/golden/ref_pieces.npz, iloss_a_* / iloss_b_*) and knn_ref64 to the fp32 brute force, so nothing here is anchored to the
kernels."""
from __future__ import annotations

import math

import numpy as np
import torch
import torch.nn.functional as F

from oracle import knn_oracle as ko
from oracle import match_loss_oracle as mlo

FACTOR = 4.0                     # err_kernel <= max(FACTOR * e32, floor)
GRAD_FLOOR = 1e-6                # normalised image-loss gradient (test_combined_image_loss_...: err < 1e-6)
VALUE_FLOOR = 2e-6               # image-loss values, absolute (the golden tests' bar)
MARGIN_PX = 1e-3                 # no match of the fp64 reference may lie this close (pixels) to a step of the match loss


# ---------------------------------------------------------------------------------------------------------------- image loss

def window_1d(dtype=torch.float32) -> torch.Tensor:
    """gaussian(11, 1.5) of utils/loss_utils.py:46-48: built and normalised in fp32 (as the kernel's host side does), then cast."""
    g = torch.tensor([math.exp(-(x - 5) ** 2 / (2.0 * 1.5 ** 2)) for x in range(11)], dtype=torch.float32)
    return (g / g.sum()).to(dtype)


def image_loss_ref(x, y, lam, dtype, upstream=(1.0, 0.0)):
    """The reference's (1 - lam) * l1_loss + lam * (1 - ssim) on the CPU in `dtype` (utils/loss_utils.py:40, :56-94; train.py:160).
    x, y: (C,H,W) or (B,C,H,W).  The gradient is that of a * loss + b w.r.t. x, upstream = (a, b).
    Returns dict(l1, ssim, loss: python floats; grad: tensor of x's shape in `dtype`)."""
    x = x.detach().cpu().to(dtype).clone().requires_grad_(True)
    y = y.detach().cpu().to(dtype)
    x4, y4 = (x, y) if x.dim() == 4 else (x[None], y[None])
    C = x4.shape[1]
    g = window_1d(dtype)
    win = (g[:, None] @ g[None, :])[None, None].expand(C, 1, 11, 11).contiguous()
    conv = lambda t: F.conv2d(t, win, padding=5, groups=C)          # noqa: E731
    mu1, mu2 = conv(x4), conv(y4)
    mu1_sq, mu2_sq, mu1_mu2 = mu1 * mu1, mu2 * mu2, mu1 * mu2
    s1, s2, s12 = conv(x4 * x4) - mu1_sq, conv(y4 * y4) - mu2_sq, conv(x4 * y4) - mu1_mu2
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    smap = ((2 * mu1_mu2 + C1) * (2 * s12 + C2)) / ((mu1_sq + mu2_sq + C1) * (s1 + s2 + C2))
    ssim = smap.mean()
    l1 = (x - y).abs().mean()
    loss = (1.0 - lam) * l1 + lam * (1.0 - ssim)
    (upstream[0] * loss + upstream[1]).backward()
    return dict(l1=float(l1.detach()), ssim=float(ssim.detach()), loss=float(loss.detach()), grad=x.grad.detach())


def grad_scale(g64: torch.Tensor, upstream: float = 1.0) -> float:
    """s = max(max|g64|, |upstream| / numel): the second term is the L1 term's gradient scale (keeps gt == img, whose fp64
    gradient is exactly 0, well defined)."""
    return max(float(g64.abs().max()), abs(upstream) / g64.numel())


def image_loss_bars(x, y, lam, upstream=(1.0, 0.0)):
    """fp64 reference, and e32 = |fp32 evaluation - fp64 evaluation| for l1, ssim, loss and the normalised gradient."""
    r64 = image_loss_ref(x, y, lam, torch.float64, upstream)
    r32 = image_loss_ref(x, y, lam, torch.float32, upstream)
    s = grad_scale(r64["grad"], upstream[0])
    e32 = {k: abs(r32[k] - r64[k]) for k in ("l1", "ssim", "loss")}
    e32["grad"] = float((r32["grad"].double() - r64["grad"]).abs().max()) / s
    return r64, e32, s


# ---------------------------------------------------------------------------------------------------------------- match loss

_PAIR_KEYS = ("uv0", "rays_o", "rays_d", "cam_rays_d", "mask0", "mask1", "intr1", "w2c1", "uv1")


def _cast_pair(p, dtype):
    M = p["uv0"].shape[0]
    out = {}
    for k in _PAIR_KEYS:
        v = p.get(k)
        if v is None:                                    # no masks: all matches valid
            v = torch.ones(M)
        out[k] = v.detach().cpu().to(dtype)
    return out


def match_loss_ref(depth, pairs, width, height, dtype, upstream=1.0):
    """Sum over pairs of oracle.match_loss_oracle.match_loss_pair on inputs cast to `dtype`; the gradient is that of
    upstream * loss w.r.t. the depth (H,W).  Returns (loss: float, grad: (H,W) tensor in dtype)."""
    d = depth.detach().cpu().reshape(depth.shape[-2], depth.shape[-1]).to(dtype).clone().requires_grad_(True)
    total = torch.zeros((), dtype=dtype)
    for p in pairs:
        if p["uv0"].shape[0] == 0:
            continue
        c = _cast_pair(p, dtype)
        total = total + mlo.match_loss_pair(d, c["uv0"], c["rays_o"], c["rays_d"], c["cam_rays_d"], c["mask0"], c["mask1"],
                                            c["intr1"], c["w2c1"], c["uv1"], float(width), float(height))
    if total.requires_grad:
        (upstream * total).backward()
    grad = d.grad.detach() if d.grad is not None else torch.zeros_like(d.detach())
    return float(total.detach()), grad


def match_decisions(depth, p, width, height, dtype=torch.float64):
    """The step functions of one pair, evaluated as the oracle does, in `dtype`: the projected pixel xy (2,M), the in-image mask,
    the counting mask (in image and mask0 * mask1 > 0) and each match's distance in pixels to the nearest step (an image
    border of view 1 for every match; px = uv1.x / py = uv1.y, the L1 term's kinks, for the matches that count)."""
    d = depth.detach().cpu().reshape(depth.shape[-2], depth.shape[-1]).to(dtype)
    c = _cast_pair(p, dtype)
    nx, ny = (c["uv0"][:, 0] / width) * 2 - 1, (c["uv0"][:, 1] / height) * 2 - 1
    md = F.grid_sample(d[None, None], torch.stack([nx, ny], -1)[None, None], mode="bilinear", align_corners=False).reshape(-1)
    z = (md / c["cam_rays_d"][:, 2]).unsqueeze(-1)
    world = (c["rays_o"] + c["rays_d"] * z).permute(1, 0)
    cam = torch.matmul(c["w2c1"], torch.cat([world, torch.ones_like(world[:1])]))[:3]
    xyz = torch.matmul(c["intr1"], cam)
    xy = xyz[:2] / (xyz[2:] + 1e-8)
    in_img = (xy[0] > 0) & (xy[0] < width) & (xy[1] > 0) & (xy[1] < height)
    counts = in_img & ((c["mask0"] * c["mask1"]) > 0)
    border = torch.minimum(torch.minimum(xy[0].abs(), (xy[0] - width).abs()), torch.minimum(xy[1].abs(), (xy[1] - height).abs()))
    valid = (c["mask0"] * c["mask1"]) > 0
    border = torch.where(valid, border, torch.full_like(border, float("inf")))       # a masked-out match never counts
    kink = torch.minimum((xy[0] - c["uv1"][:, 0]).abs(), (xy[1] - c["uv1"][:, 1]).abs())
    kink = torch.where(counts, kink, torch.full_like(kink, float("inf")))
    return dict(xy=xy, z=xyz[2], in_img=in_img, counts=counts, margin=torch.minimum(border, kink))


# ---------------------------------------------------------------------------------------------------------------------- kNN

def knn_ref64(points) -> np.ndarray:
    """Mean squared distance to the 3 nearest other points in fp64 (scipy's kd-tree): scales to n where the brute force does not."""
    return ko.mean_dist2_kdtree(np.asarray(points, dtype=np.float64))


def lattice_cloud(n: int, spacing: float = 0.5) -> np.ndarray:
    """The first n points of a cubic lattice (x fastest): the three smallest distances of an interior point are equal."""
    side = max(2, int(math.ceil(n ** (1.0 / 3.0) - 1e-9)))
    while side ** 3 < n:
        side += 1
    i = np.arange(n)
    return (np.stack([i % side, (i // side) % side, i // (side * side)], 1) * spacing).astype(np.float32)


def identical_cloud(n: int) -> np.ndarray:
    return np.tile(np.array([[0.3, -1.7, 2.9]], dtype=np.float32), (n, 1))


def collinear_cloud(n: int, seed: int) -> np.ndarray:
    """Points on one line at random parameters, about 125 per unit length at every n (the squared distances stay well above the
    1e-7 absolute term of the bar)."""
    rng = np.random.default_rng(seed)
    t = np.sort(rng.uniform(-n / 250.0, n / 250.0, size=n))
    rng.shuffle(t)
    d = np.array([0.6, -0.3, 0.74])
    return (np.array([0.5, 1.0, -2.0])[None] + t[:, None] * d[None]).astype(np.float32)


def clusters_cloud(n: int, seed: int) -> np.ndarray:
    """Two clusters 200 units apart, the second holding a seventh of the points (at least two)."""
    rng = np.random.default_rng(seed)
    nb = min(max(2, n // 7), n)
    a = rng.normal(size=(n - nb, 3)) * 0.5
    b = rng.normal(size=(nb, 3)) * 0.05 + np.array([200.0, -50.0, 30.0])
    return np.concatenate([a, b]).astype(np.float32)


def offset_cloud(n: int, seed: int) -> np.ndarray:
    """A unit normal cloud offset by 1e3 in every coordinate: the fp32 coordinates carry 6e-5 of absolute resolution."""
    rng = np.random.default_rng(seed)
    return (rng.normal(size=(n, 3)) + 1.0e3).astype(np.float32)


def aniso_cloud(n: int, seed: int) -> np.ndarray:
    rng = np.random.default_rng(seed)
    return rng.normal(size=(n, 3)).astype(np.float32) * np.array([3.0, 1.0, 0.3], dtype=np.float32)


CLOUDS = {"lattice": lambda n, seed: lattice_cloud(n), "identical": lambda n, seed: identical_cloud(n),
          "collinear": collinear_cloud, "clusters": clusters_cloud, "offset1e3": offset_cloud, "aniso": aniso_cloud}


# ------------------------------------------------------------------------------------------------------------ bar + census

def held_to(what: str, err: float, e32: float, floor: float, elements: int = 1, factor: float = FACTOR) -> None:
    """Assert err <= max(factor * e32, floor) after recording the case: printed (pytest -s / -rA shows it) and appended to
    parity_utils.CENSUS, whose `worst_ratio` slot here holds  factor * err / bar  — that is err / e32 where 4 * e32 is the bar,
    and the same multiple of floor / 4 where the floor is; a case passes up to 4.0."""
    import parity_utils as pu
    bar = max(factor * e32, floor)
    ratio = factor * err / bar
    print(f"CENSUS {what}: err {err:.3e} e32 {e32:.3e} bar {bar:.3e} ratio {ratio:.3f}")
    pu.CENSUS.append((str(what), float(err), 0.0, float(ratio), int(elements)))
    assert math.isfinite(err), (what, err)
    assert err <= bar, (what, "err", err, "e32", e32, "bar = max(%g * e32, %g)" % (factor, floor), bar)

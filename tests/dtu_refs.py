"""Plain-torch restatements of what the reference's train.py runs only on DTU scenes, parametrised by dtype like loss_refs.py.

    bg_mask_loop          train.py:149-158   the reference's loop, statement for statement (device-agnostic: the timing tool runs it
                                             on the GPU)
    bg_mask_closed_form   the same mask as one rule per pixel (what csrc/dtumask.hip implements); tests/test_dtu_cpu.py holds the
                          two equal
    alpha_term_ref        train.py:167-168   rendered_alpha[bg_mask].mean() and its gradient
    eval_metrics_ref      train.py:252-265   clamp, l1_loss(image[:, mask], gt[:, mask]).mean(), psnr(...).mean()
                                             (utils/loss_utils.py:40, utils/image_utils.py:17-19)
    training_loss_torch   train.py:149-161 + :167-168 as the reference runs them per iteration, on whatever device the inputs live

Called with torch.float64 the value functions ARE the reference of tests/test_gpu_dtu.py; with torch.float32 they give `e32`, the
error of a plain fp32 evaluation, from which the bars follow (loss_refs.held_to).  tests/test_dtu_cpu.py pins eval_metrics_ref in
fp64 to numbers the reference's own l1_loss and psnr produced (tests/golden/ref_dtu.npz)."""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

import loss_refs as LR

THR, THR_SCAN110, RUN = 30 / 255, 15 / 255, 50


def dark_run_image(H, W, seed, dark_share=0.97) -> torch.Tensor:
    """(3,H,W) fp32: each pixel dark (all channels < 0.05, under both thresholds) with probability `dark_share`, otherwise bright
    (>= 0.2) in ONE channel only; the columns so hold dark runs of every length."""
    g = torch.Generator().manual_seed(seed)
    dark = torch.rand(H, W, generator=g) < dark_share
    hi = torch.rand(3, H, W, generator=g) * 0.8 + 0.2
    img = torch.rand(3, H, W, generator=g) * 0.05
    bright_channel = torch.randint(0, 3, (H, W), generator=g)
    for c in range(3):
        sel = (~dark) & (bright_channel == c)
        img[c][sel] = hi[c][sel]
    return img


def bg_mask_loop(gt: torch.Tensor, thr: float = THR, run: int = RUN):
    """train.py:149-158.  gt (3,H,W); NOT modified (the reference writes in place: the caller passes a clone for that).
    Returns (bg_mask bool (1,H,W), gt_masked, count: 0-dim int64)."""
    gt_image = gt.clone()
    bg_mask = (gt_image.max(0, keepdim=True).values < thr)
    bg_mask_clone = bg_mask.clone()
    for i in range(1, run):
        bg_mask[:, i:] *= bg_mask_clone[:, :-i]
    gt_image[bg_mask.repeat(3, 1, 1)] = 0.
    return bg_mask, gt_image, bg_mask.sum()


def bg_mask_closed_form(gt, thr: float = THR, run: int = RUN) -> np.ndarray:
    """mask[y, x] = dark[y, x] and (length of the run of dark pixels ending at row y in column x) >= min(y + 1, run); (H,W) bool.
    The threshold is compared in the image's dtype, as torch compares a tensor with a Python number."""
    g = np.asarray(gt)
    dark = g.max(axis=0) < g.dtype.type(thr)
    H, W = dark.shape
    mask = np.zeros((H, W), dtype=bool)
    length = np.zeros(W, dtype=np.int64)
    for y in range(H):
        length = np.where(dark[y], length + 1, 0)
        mask[y] = length >= min(y + 1, run)
    return mask


def alpha_term_ref(alpha, mask, dtype, upstream: float = 1.0):
    """rendered_alpha[bg_mask].mean() on the CPU in `dtype` and the gradient of upstream * that w.r.t. alpha.
    Returns (value: python float, grad: tensor of alpha's shape in dtype)."""
    a = alpha.detach().cpu().to(dtype).clone().requires_grad_(True)
    m = mask.detach().cpu().bool().reshape(a.shape)
    v = a[m].mean()
    (upstream * v).backward()
    return float(v.detach()), a.grad.detach()


def alpha_term_bars(alpha, mask, upstream: float = 1.0):
    v64, g64 = alpha_term_ref(alpha, mask, torch.float64, upstream)
    v32, _ = alpha_term_ref(alpha, mask, torch.float32, upstream)
    return v64, g64, abs(v32 - v64)


def eval_metrics_ref(image, gt, dtumask, dtype):
    """train.py:253-265 for one view on the CPU in `dtype`.  Returns dict(l1, psnr: python floats, mse: (C,) numpy in dtype)."""
    image = torch.clamp(image.detach().cpu().to(dtype), 0.0, 1.0)
    gt_image = torch.clamp(gt.detach().cpu().to(dtype), 0.0, 1.0)
    if dtumask is not None:
        mask = dtumask.detach().cpu().reshape(image.shape[-2], image.shape[-1]) > 0
        a, b = image[:, mask], gt_image[:, mask]
    else:
        a, b = image, gt_image
    l1 = torch.abs(a - b).mean().mean()
    mse = ((a - b) ** 2).reshape(a.shape[0], -1).mean(1, keepdim=True)
    psnr = (20 * torch.log10(1.0 / torch.sqrt(mse))).mean()
    return dict(l1=float(l1), psnr=float(psnr), mse=mse[:, 0].numpy())


def eval_metrics_bars(image, gt, dtumask):
    """fp64 reference and e32 per quantity (mse: per channel)."""
    r64, r32 = eval_metrics_ref(image, gt, dtumask, torch.float64), eval_metrics_ref(image, gt, dtumask, torch.float32)
    e32 = dict(l1=abs(r32["l1"] - r64["l1"]), psnr=abs(r32["psnr"] - r64["psnr"]),
               mse=np.abs(r32["mse"].astype(np.float64) - r64["mse"]))
    return r64, e32


def psnr_floor(mse64) -> float:
    """VALUE_FLOOR on an mse, passed through the derivative of 20 * log10(1 / sqrt(mse)) = -(10 / ln 10) * ln(mse)."""
    return (10.0 / np.log(10.0)) * LR.VALUE_FLOOR / float(np.min(mse64))


def ssim_torch(img1, img2):
    """utils/loss_utils.py:56-94 (11x11 window, sigma 1.5, mean over all) on the inputs' device and dtype."""
    C = img1.shape[-3]
    g = LR.window_1d(img1.dtype).to(img1.device)
    win = (g[:, None] @ g[None, :])[None, None].expand(C, 1, 11, 11).contiguous()
    x, y = (img1, img2) if img1.dim() == 4 else (img1[None], img2[None])
    conv = lambda t: F.conv2d(t, win, padding=5, groups=C)          # noqa: E731
    mu1, mu2 = conv(x), conv(y)
    mu1_sq, mu2_sq, mu1_mu2 = mu1.pow(2), mu2.pow(2), mu1 * mu2
    s1, s2, s12 = conv(x * x) - mu1_sq, conv(y * y) - mu2_sq, conv(x * y) - mu1_mu2
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    return (((2 * mu1_mu2 + C1) * (2 * s12 + C2)) / ((mu1_sq + mu2_sq + C1) * (s1 + s2 + C2))).mean()


def training_loss_torch(image, rendered_alpha, gt, thr: float = THR, lambda_dssim: float = 0.2, run: int = RUN):
    """One iteration's DTU image loss as the reference computes it: mask loop, ground truth zeroed, (1 - l) * L1 + l * (1 - SSIM),
    plus rendered_alpha[bg_mask].mean() (a boolean index: reads the host)."""
    bg_mask, gt_image, _ = bg_mask_loop(gt, thr, run)
    Ll1 = torch.abs(image - gt_image).mean()
    loss = (1.0 - lambda_dssim) * Ll1 + lambda_dssim * (1.0 - ssim_torch(image, gt_image))
    return loss + rendered_alpha[bg_mask].mean()

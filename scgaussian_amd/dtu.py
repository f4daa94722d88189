"""DTU scenes: the code the reference's train.py runs only when "dtu" is in the source path, host side (csrc/dtumask.hip).

    train.py:149-158   bg_mask = gt.max(0) < 30/255, ANDed with itself shifted down by 1..49 rows; gt[bg_mask] = 0
                                                                                        -> background_mask / DtuView
    train.py:167-168   loss += rendered_alpha[bg_mask].mean()                           -> alpha_term / training_loss
    train.py:252-265   clamped l1_loss and psnr under `dtumask > 0`                     -> eval_metrics

The reference pays about a hundred small launches and a boolean-index write per iteration for the first, a boolean index (a host
synchronisation, an index-put in the backward) for the second and two more boolean gathers per view for the third.  Here each is one
or two kernels that read counts and upstream gradients from device memory: nothing reads the host, so a DTU training step can be
captured (graph_step.CapturedStep).  CPU tensors raise ScgError: there is no CPU path."""
from __future__ import annotations

import torch

from . import _lib, losses
from ._lib import check

THRESHOLD = 30 / 255                 # train.py:152
THRESHOLD_SCAN110 = 15 / 255         # train.py:154
RUN = 50                             # train.py:156: shifts 1 .. 49


def threshold_for(source_path: str) -> float:
    """The darkness threshold train.py:151-154 picks from the scene's path."""
    return THRESHOLD_SCAN110 if "scan110" in str(source_path) else THRESHOLD


def background_mask(gt: torch.Tensor, threshold: float = THRESHOLD, run: int = RUN, inplace: bool = False):
    """train.py:149-158 in one launch.  gt: (3,H,W) fp32 on the GPU.  Returns (mask, gt_masked, count): mask bool (1,H,W) — true
    where the pixel is dark (max over the channels < threshold) and so are the min(row, run - 1) pixels above it —, gt_masked = gt
    with those pixels zeroed, count a 0-dim int32 device tensor holding the number of masked pixels (never read here).
    inplace=True writes into `gt` and returns it, as the reference does (needs a contiguous fp32 `gt` and threshold > 0)."""
    lib = _lib.load()
    stream = _lib.stream_of(gt, "background_mask")
    if gt.dim() != 3 or gt.shape[0] != 3:
        raise ValueError("gt must be (3,H,W)")
    if inplace:
        if gt.dtype != torch.float32 or not gt.is_contiguous():
            raise ValueError("inplace=True needs a contiguous float32 gt")
        src = dst = gt.detach()
    else:
        src = gt.detach().float().contiguous()
        dst = torch.empty_like(src)
    _, H, W = src.shape
    dev = src.device
    with torch.cuda.device(dev):
        mask = torch.empty((H, W), dtype=torch.uint8, device=dev)
        count = torch.empty((1,), dtype=torch.int32, device=dev)        # the library's one uint32: H * W < 2^31
        check(lib.scg_dtu_bg_mask(src.data_ptr(), H, W, float(threshold), int(run), mask.data_ptr(), dst.data_ptr(),
                                  count.data_ptr(), stream), "scg_dtu_bg_mask")
    return mask.view(torch.bool)[None], (gt if inplace else dst), count.reshape(())


class DtuView:
    """What a DTU camera needs of its ground-truth image, built ONCE: `mask` bool (1,H,W), `gt` (the image zeroed under the mask)
    and `count` (0-dim device tensor).  The reference rebuilds all three in every iteration that draws the camera (train.py:149-158),
    in place on the camera's own image.  The mask depends on the image alone, and the rule is idempotent — a zeroed pixel was dark
    and stays dark, so the second pass over the zeroed image finds the same mask and zeroes the same pixels —, so building it once per
    camera changes the schedule, not any result."""

    def __init__(self, gt_image: torch.Tensor, threshold: float = THRESHOLD, run: int = RUN, inplace: bool = False):
        self.threshold, self.run = float(threshold), int(run)
        self.mask, self.gt, self.count = background_mask(gt_image, threshold, run, inplace)
        self._mask_u8 = self.mask.view(torch.uint8).reshape(-1)

    @classmethod
    def for_scene(cls, gt_image: torch.Tensor, source_path: str) -> "DtuView":
        return cls(gt_image, threshold_for(source_path))


class _MaskedMean(torch.autograd.Function):
    """x[mask].mean() without the boolean index: two launches forward, one backward, count and upstream read on the device."""

    @staticmethod
    def forward(ctx, x, mask_u8, count):
        lib = _lib.load()
        xs = x.detach().float().contiguous()
        n = xs.numel()
        if mask_u8.numel() != n:
            raise ValueError("rendered_alpha and the view's mask differ in size")
        dev = xs.device
        with torch.cuda.device(dev):
            out = torch.empty((1,), dtype=torch.float32, device=dev)
            nbytes = lib.scg_masked_mean_scratch_bytes(n)
            scratch = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
            check(lib.scg_masked_mean_forward(xs.data_ptr(), mask_u8.data_ptr(), n, count.data_ptr(), out.data_ptr(),
                                              scratch.data_ptr(), nbytes, _lib.stream_of(dev, "alpha_term")), "scg_masked_mean_forward")
        ctx.mask_u8, ctx.count, ctx.shape, ctx.in_dtype = mask_u8, count, x.shape, x.dtype
        return out.reshape(())

    @staticmethod
    def backward(ctx, g):
        lib = _lib.load()
        mask_u8, count = ctx.mask_u8, ctx.count
        dev = mask_u8.device
        g = g.detach()
        if g.dtype != torch.float32 or g.device != dev:
            g = g.to(dev, torch.float32)
        g = g.contiguous()
        n = mask_u8.numel()
        with torch.cuda.device(dev):
            d_x = torch.empty((n,), dtype=torch.float32, device=dev)
            check(lib.scg_masked_mean_backward(mask_u8.data_ptr(), n, count.data_ptr(), g.data_ptr(), d_x.data_ptr(),
                                               _lib.stream_of(dev, "alpha_term")), "scg_masked_mean_backward")
        return d_x.reshape(ctx.shape).to(ctx.in_dtype), None, None


def alpha_term(rendered_alpha: torch.Tensor, view: DtuView) -> torch.Tensor:
    """train.py:168: rendered_alpha[bg_mask].mean() — NaN for an empty mask, as in torch.  No host read: capturable."""
    _lib.stream_of(rendered_alpha, "alpha_term")
    return _MaskedMean.apply(rendered_alpha, view._mask_u8, view.count)


def training_loss(image: torch.Tensor, rendered_alpha: torch.Tensor, view: DtuView, lambda_dssim=0.2) -> torch.Tensor:
    """The image part of a DTU iteration's loss: train.py:160-161 on the masked ground truth plus train.py:168."""
    return losses.image_loss(image, view.gt, lambda_dssim) + alpha_term(rendered_alpha, view)


def eval_metrics_all(image: torch.Tensor, gt: torch.Tensor, dtumask=None):
    """(l1, psnr, mse (C,)) of train.py:252-265 as device tensors from one fused pass: both images clamped to [0, 1], the pixels
    with dtumask > 0 selected (all of them without a mask).  NaN for an empty selection."""
    lib = _lib.load()
    stream = _lib.stream_of(image, "eval_metrics")
    if image.dim() != 3:
        raise ValueError("image must be (C,H,W)")
    a = image.detach().float().contiguous()
    b = gt.detach().to(a.device).float().contiguous()
    if a.shape != b.shape:
        raise ValueError("image and gt shapes differ")
    C, H, W = a.shape
    m = None
    if dtumask is not None:
        m = dtumask.detach().to(a.device).float().contiguous()
        if m.numel() != H * W:
            raise ValueError("dtumask must be (H,W) or (1,H,W)")
    dev = a.device
    with torch.cuda.device(dev):
        out = torch.empty((2 + C,), dtype=torch.float32, device=dev)
        nbytes = lib.scg_eval_metrics_scratch_bytes(C, H, W)
        scratch = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
        check(lib.scg_eval_metrics(a.data_ptr(), b.data_ptr(), _lib.ptr(m), C, H, W, out.data_ptr(), scratch.data_ptr(), nbytes,
                                   stream), "scg_eval_metrics")
    return out[0], out[1], out[2:]


def eval_metrics(image: torch.Tensor, gt: torch.Tensor, dtumask=None):
    """(l1, psnr) of one evaluation view as device scalars: l1_loss(image[:, mask], gt[:, mask]).mean() and
    psnr(image[:, mask], gt[:, mask]).mean() of train.py:261-262 (or :264-265 without a mask), clamping included."""
    l1, psnr, _ = eval_metrics_all(image, gt, dtumask)
    return l1, psnr

"""Plain-torch restatements of the reference's test-set evaluation, parametrised by dtype like loss_refs.py and dtu_refs.py.

    quantise              torchvision.utils.save_image's mul(255).add_(0.5).clamp_(0, 255).to(uint8) (the library is absent here);
                          the cast of NaN is undefined in torch and pinned to 0, as the kernel documents it
    pixel_loss_ref        utils/loss_utils.py:162-205   get_pixel_loss: L1 term + 5x5 box-window SSIM behind ReflectionPad2d(2)
    normalised_depth      render.py:143
    masked_images         metrics.py:36-44              to_tensor(PNG) * mask + (1 - mask), mask == 1.
    ssim_ref / psnr_ref   utils/loss_utils.py:56-94, utils/image_utils.py:17-19 as metrics.py:87-89 calls them
    view_ref              all of it for one view
    view_torch            the same arithmetic as the two scripts run it on a device, its five copies to the host included
                          (tools/eval_timing.py)

Called with torch.float64 the value functions ARE the reference of tests/test_gpu_eval.py; with torch.float32 they give `e_ref`, the
deviation of a plain fp32 evaluation.  tests/test_eval_cpu.py pins them to numbers the reference's own get_pixel_loss, ssim and
psnr produced (tests/golden/ref_eval.npz)."""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

import loss_refs as LR


def quantise(x: torch.Tensor) -> torch.Tensor:
    """q(x) = uint8(trunc(clamp(fl(fl(x * 255) + 0.5), 0, 255))) in fp32, q(NaN) = 0."""
    v = x.detach().float().mul(255).add_(0.5).clamp_(0, 255)
    return torch.nan_to_num(v, nan=0.0).to(torch.uint8)


def pixel_loss_ref(image, gt_image, dtype):
    """get_pixel_loss(image, gt_image) -> (H,W) in `dtype`, statement for statement."""
    image, gt_image = image.detach().to(dtype), gt_image.detach().to(dtype)
    l1 = (image - gt_image).abs().mean(dim=0)
    x, y = F.pad(image[None], (2, 2, 2, 2), mode="reflect"), F.pad(gt_image[None], (2, 2, 2, 2), mode="reflect")
    pool = lambda t: F.avg_pool2d(t, 5, 1)          # noqa: E731
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    mu_x, mu_y = pool(x), pool(y)
    sigma_x = pool(x ** 2) - mu_x ** 2
    sigma_y = pool(y ** 2) - mu_y ** 2
    sigma_xy = pool(x * y) - mu_x * mu_y
    SSIM_n = (2 * mu_x * mu_y + C1) * (2 * sigma_xy + C2)
    SSIM_d = (mu_x ** 2 + mu_y ** 2 + C1) * (sigma_x + sigma_y + C2)
    ssim_l = torch.clamp((1 - SSIM_n / SSIM_d) / 2, 0, 1).squeeze(0)
    return l1 * 0.5 + ssim_l.mean(dim=0) * 0.5


def normalised_depth(depth: torch.Tensor) -> torch.Tensor:
    return (depth - depth.min()) / (depth.max() - depth.min())


def masked_images(q_render, q_gt, q_mask, dtype=torch.float32):
    """metrics.py:36-44 from the uint8 arrays the PNGs hold: q_render, q_gt (H,W,3), q_mask (H,W) or None.
    Returns (render, gt: (1,3,H,W) in dtype, mask_bin: (1,3,H,W) bool).  to_tensor is uint8 -> float32 -> / 255."""
    to_tensor = lambda q: (q.permute(2, 0, 1).float() / 255)[None]          # noqa: E731
    r, g = to_tensor(q_render), to_tensor(q_gt)
    if q_mask is not None:
        mask = (q_mask.float() / 255)[None, None].expand(1, 3, -1, -1)
    else:
        mask = torch.ones_like(g)
    r, g, mask = r.to(dtype), g.to(dtype), mask.to(dtype)
    return r * mask + (1 - mask), g * mask + (1 - mask), mask == 1.


def ssim_ref(img1, img2):
    """utils/loss_utils.py:56-94 on (1,3,H,W): the 11x11 window is built, normalised and multiplied out in fp32 and then cast
    (create_window, type_as), whatever the images' dtype."""
    C = img1.shape[-3]
    g = LR.window_1d(torch.float32)
    win = (g[:, None] @ g[None, :])[None, None].expand(C, 1, 11, 11).contiguous().to(img1.device, img1.dtype)
    conv = lambda t: F.conv2d(t, win, padding=5, groups=C)          # noqa: E731
    mu1, mu2 = conv(img1), conv(img2)
    mu1_sq, mu2_sq, mu1_mu2 = mu1.pow(2), mu2.pow(2), mu1 * mu2
    s1, s2, s12 = conv(img1 * img1) - mu1_sq, conv(img2 * img2) - mu2_sq, conv(img1 * img2) - mu1_mu2
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    return (((2 * mu1_mu2 + C1) * (2 * s12 + C2)) / ((mu1_sq + mu2_sq + C1) * (s1 + s2 + C2))).mean()


def psnr_ref(img1, img2):
    mse = ((img1 - img2) ** 2).view(img1.shape[0], -1).mean(1, keepdim=True)
    return 20 * torch.log10(1.0 / torch.sqrt(mse))


def view_ref(render, gt, depth, dtumask, dtype):
    """One view on the CPU.  The quantised arrays are always formed in fp32 (they are what the PNGs hold); `dtype` is the precision
    of the error map and of everything metrics.py computes from the quantised pixels.  Returns a dict: renders, gt (H,W,3) uint8,
    depth, error_map, dtumask (H,W) uint8 or None, error_map_val (H,W) in dtype, renders_masked, gt_masked (3,H,W) in dtype,
    S, K (python ints), ssim, psnr (python floats)."""
    render, gt = render.detach().cpu().float(), gt.detach().cpu().float()
    H, W = render.shape[-2:]
    depth = depth.detach().cpu().float().reshape(H, W)
    err = pixel_loss_ref(render, gt, dtype)
    out = {"renders": quantise(render).permute(1, 2, 0).contiguous(), "gt": quantise(gt).permute(1, 2, 0).contiguous(),
           "depth": quantise(normalised_depth(depth)), "error_map": quantise(pixel_loss_ref(render, gt, torch.float32)),
           "dtumask": None if dtumask is None else quantise(dtumask.detach().cpu().float().reshape(H, W)), "error_map_val": err}
    r, g, mask_bin = masked_images(out["renders"], out["gt"], out["dtumask"], dtype)
    out["renders_masked"], out["gt_masked"] = r[0], g[0]
    diff = out["renders"].permute(2, 0, 1).to(torch.int64) - out["gt"].permute(2, 0, 1).to(torch.int64)
    out["S"], out["K"] = int((diff * diff)[mask_bin[0]].sum()), int(mask_bin.sum())
    out["ssim"] = float(ssim_ref(r, g))
    out["psnr"] = float(psnr_ref(r[mask_bin][None, ...], g[mask_bin][None, ...]))          # metrics.py:89
    return out


def view_torch(render, gt, depth, dtumask):
    """What render_set + evaluate compute for one view, as they compute it, on the inputs' device in fp32: five images quantised
    and copied to the host one by one (save_image), uploaded again (readImages), SSIM and PSNR read as python numbers."""
    dev = render.device
    depth_n = normalised_depth(depth)
    error_map = pixel_loss_ref(render, gt, torch.float32)
    host = [quantise(t).cpu() for t in (error_map, render, gt, depth_n)]
    q_mask = None if dtumask is None else quantise(dtumask.reshape(depth.shape[-2], depth.shape[-1])).cpu()
    q_r, q_g = host[1].permute(1, 2, 0).to(dev), host[2].permute(1, 2, 0).to(dev)
    r, g, mask_bin = masked_images(q_r, q_g, None if q_mask is None else q_mask.to(dev))
    return float(ssim_ref(r, g)), float(psnr_ref(r[mask_bin][None, ...], g[mask_bin][None, ...]))


def images(H, W, seed, spread=0.15, outside=False):
    """(render, gt, depth) of a test: gt in [0, 1], render = gt + noise (unclamped; `outside`: scaled to reach well outside [0, 1]),
    depth positive."""
    g = torch.Generator().manual_seed(seed)
    gt = torch.rand(3, H, W, generator=g)
    render = gt + spread * torch.randn(3, H, W, generator=g)
    if outside:
        render = render * 1.6 - 0.3
    depth = torch.rand(1, H, W, generator=g) * 5 + 0.5
    return render, gt, depth


def np_u8(t):
    return np.ascontiguousarray(t.detach().cpu().numpy())

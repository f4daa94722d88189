#!/usr/bin/env python3
"""Generate tests/golden/ref_eval.npz by CALLING the reference's own get_pixel_loss and ssim (utils/loss_utils.py:195-205, :56-94)
and psnr (utils/image_utils.py:17-19) on the CPU, in fp32 and in fp64.  Only numeric arrays are committed; no reference source
travels.  The reference is imported as make_golden_model.py imports it.

get_pixel_loss is called on the raw render and ground truth, as render.py:149 calls it.  ssim and psnr are called as
metrics.py:87-89 calls them: on `to_tensor(PNG) * mask + (1 - mask)` and on that under `mask == 1.`, the PNG contents being the
uint8 arrays of torchvision's save_image quantiser (the library is absent; it is restated here in one line:
mul(255).add_(0.5).clamp_(0, 255).to(uint8)).

Cases:
  plain       (3,12,9)   render = gt + noise, no mask
  binary      (3,17,33)  a 0 / 1 mask
  fractional  (3,40,70)  a mask with zeros, ones and values in between (only the pixels that quantise to 255 count for the PSNR)
  outside     (3,21,35)  a render with values well outside [0, 1], a 0 / 1 mask

Per case: the inputs, the error map in fp32 and fp64 and `e_ref`, the largest absolute difference between the two; SSIM and PSNR
in fp32 and fp64; S, K, the integers under the PSNR.

Run:  python tests/golden/make_golden_eval.py      (needs the reference tree; CPU only)
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_model as mgm                                                             # noqa: E402

OUT = os.path.join(HERE, "ref_eval.npz")


def quantise(x):
    return x.float().mul(255).add_(0.5).clamp_(0, 255).to(torch.uint8)


def cases():
    g = torch.Generator().manual_seed(13)

    def pair(H, W, spread=0.15):
        gt = torch.rand(3, H, W, generator=g)
        return gt + spread * torch.randn(3, H, W, generator=g), gt, torch.rand(1, H, W, generator=g) * 5 + 0.5
    out = {}
    r, gt, d = pair(12, 9)
    out["plain"] = (r, gt, d, None)
    r, gt, d = pair(17, 33)
    out["binary"] = (r, gt, d, (torch.rand(17, 33, generator=g) > 0.4).float())
    r, gt, d = pair(40, 70, 0.05)
    m = torch.rand(40, 70, generator=g)
    m = torch.where(m < 0.3, torch.zeros(()), torch.where(m > 0.6, torch.ones(()), m))
    out["fractional"] = (r, gt, d, m)
    r, gt, d = pair(21, 35)
    out["outside"] = (r * 1.6 - 0.3, gt, d, (torch.rand(21, 35, generator=g) > 0.3).float())
    return out


def main():
    sys.meta_path.insert(0, mgm._Finder())
    sys.path.insert(0, mgm.REF)
    from utils.loss_utils import get_pixel_loss, ssim
    from utils.image_utils import psnr
    out = {}
    for name, (render, gt, depth, dtumask) in cases().items():
        out[f"{name}_render"], out[f"{name}_gt"], out[f"{name}_depth"] = render.numpy(), gt.numpy(), depth.numpy()
        if dtumask is not None:
            out[f"{name}_mask"] = dtumask.numpy()
        e32, e64 = get_pixel_loss(render, gt), get_pixel_loss(render.double(), gt.double())          # render.py:149
        out[f"{name}_error_32"], out[f"{name}_error_64"] = e32.numpy(), e64.numpy()
        out[f"{name}_e_ref"] = np.float64((e32.double() - e64).abs().max())
        q_r, q_g = quantise(render), quantise(gt)                                                    # what the PNGs hold
        q_m = None if dtumask is None else quantise(dtumask)[None].expand(3, -1, -1)
        for tag, dtype in (("32", torch.float32), ("64", torch.float64)):
            to_tensor = lambda q: (q.float() / 255)[None].to(dtype)          # noqa: E731  (tf.to_tensor of a uint8 image)
            mask = torch.ones((1, 3) + tuple(gt.shape[1:]), dtype=dtype) if q_m is None else to_tensor(q_m)     # metrics.py:36-41
            mask_bin = (mask == 1.)
            r = to_tensor(q_r) * mask + (1 - mask)                                                   # metrics.py:43-44
            g_ = to_tensor(q_g) * mask + (1 - mask)
            out[f"{name}_ssim_{tag}"] = ssim(r, g_).double().numpy()                                 # metrics.py:87
            out[f"{name}_psnr_{tag}"] = psnr(r[mask_bin][None, ...], g_[mask_bin][None, ...]).double().reshape(()).numpy()
        d = q_r.long() - q_g.long()
        out[f"{name}_S"] = np.int64(int((d * d)[mask_bin[0]].sum()))
        out[f"{name}_K"] = np.int64(int(mask_bin.sum()))
        print(name, {k: v for k, v in out.items() if k.startswith(name) and v.ndim == 0})
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes;", len(out), "arrays")


if __name__ == "__main__":
    main()

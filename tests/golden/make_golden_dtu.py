#!/usr/bin/env python3
"""Generate tests/golden/ref_dtu.npz by CALLING the reference's own l1_loss (utils/loss_utils.py:40) and psnr / mse
(utils/image_utils.py:14-19) on the CPU, in fp32 and in fp64, the way train.py:253-265 calls them for an evaluation view:
both images clamped to [0, 1], then `image[:, mask]` / `gt[:, mask]` with mask = dtumask > 0 where the view has one.
Only numeric arrays are committed; no reference source travels.  The reference is imported as make_golden_model.py imports it.

Cases:
  plain    (3,12,9)  values in [0, 1], no mask
  masked   (3,12,9)  the same images under a mask with zeros, positive and negative entries (43 of 108 pixels selected)
  clamped  (3,10,7)  values in [-0.4, 1.4] (about a third outside [0, 1]), masked

The background-mask rule of train.py:149-158 is inline code of the training loop and cannot be imported: it rests on the
restatement tests/dtu_refs.py (bg_mask_loop), not on this file.

Run:  python tests/golden/make_golden_dtu.py      (needs the reference tree; CPU only)
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_model as mgm                                                             # noqa: E402

OUT = os.path.join(HERE, "ref_dtu.npz")


def cases():
    g = torch.Generator().manual_seed(24)
    img = torch.rand(3, 12, 9, generator=g)
    gt = (img + 0.15 * torch.randn(3, 12, 9, generator=g)).clamp(0, 1)
    mask = torch.randn(12, 9, generator=g)
    mask[mask.abs() < 0.3] = 0.0                         # zeros, negative and positive entries: selected where > 0
    img2 = torch.rand(3, 10, 7, generator=g) * 1.8 - 0.4
    gt2 = torch.rand(3, 10, 7, generator=g) * 1.8 - 0.4
    mask2 = (torch.rand(10, 7, generator=g) > 0.35).float() * 255.0
    return {"plain": (img, gt, None), "masked": (img, gt, mask), "clamped": (img2, gt2, mask2)}


def main():
    sys.meta_path.insert(0, mgm._Finder())
    sys.path.insert(0, mgm.REF)
    from utils.loss_utils import l1_loss
    from utils.image_utils import psnr, mse
    out = {}
    for name, (img, gt, dtumask) in cases().items():
        out[f"{name}_img"], out[f"{name}_gt"] = img.numpy(), gt.numpy()
        if dtumask is not None:
            out[f"{name}_mask"] = dtumask.numpy()
        for tag, dtype in (("32", torch.float32), ("64", torch.float64)):
            image = torch.clamp(img.to(dtype), 0.0, 1.0)                                   # train.py:253-254
            gt_image = torch.clamp(gt.to(dtype), 0.0, 1.0)
            if dtumask is not None:
                mask = dtumask > 0                                                         # train.py:260
                a, b = image[:, mask], gt_image[:, mask]
                out[f"{name}_selected"] = np.int64(int(mask.sum()))
            else:
                a, b = image, gt_image
            out[f"{name}_l1_{tag}"] = l1_loss(a, b).mean().double().numpy()                # train.py:261 / :264
            out[f"{name}_psnr_{tag}"] = psnr(a, b).mean().double().numpy()                 # train.py:262 / :265
            out[f"{name}_mse_{tag}"] = mse(a, b)[:, 0].double().numpy()
        print(name, {k: v for k, v in out.items() if k.startswith(name) and v.ndim == 0})
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes;", len(out), "arrays")


if __name__ == "__main__":
    main()

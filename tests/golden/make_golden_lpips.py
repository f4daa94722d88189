"""Records tests/golden/ref_lpips.npz from the restatement of the LPIPS rule in tests/lpips_refs.py, NOT from the reference's
lpipsPyTorch: that package imports torchvision and fetches its weights from the net, neither of which this project's stack has.
The weights are lpips_refs.make_weights(), the scenes lpips_refs.SCENES.  The sequential fp32 chain of a whole network is slow above about 20 x 20
(a minute for the whole set), which is why its results are recorded and the GPU tests recompute nothing slow.

    python tests/golden/make_golden_lpips.py

weight_seed; scenes (n,3): H, W, seed.  Per scene <tag> = s<H>x<W>: <tag>_value, <tag>_terms (5,) in fp64; <tag>_names and
<tag>_dev_torch32, <tag>_dev_chain32: per named tensor (value, terms, fx0..4, fy0..4) the largest deviation from fp64 of torch's
fp32 run and of the sequential chain; <tag>_max: per named tensor the largest magnitude in fp64 (the ulp's scale).  The feature maps
themselves are not stored (one scene's exceed the size a committed file may have): the fp64 run that yields them takes well under a
second at these sizes."""
import os
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import lpips_refs as LR                                                                     # noqa: E402


def main():
    torch.manual_seed(0)
    weights = LR.make_weights()
    out = {"weight_seed": np.int64(LR.WEIGHT_SEED), "scenes": np.array(LR.SCENES, dtype=np.int64)}
    for H, W, seed in LR.SCENES:
        t0 = time.time()
        x, y = LR.make_images(H, W, seed)
        r64 = LR.rule(x, y, weights)
        d32 = LR.deviations(r64, LR.rule(x, y, weights, torch.float32))
        dch = LR.deviations(r64, LR.chain32(x, y, weights))
        names = sorted(d32)
        t = LR.tag(H, W)
        out[f"{t}_value"], out[f"{t}_terms"] = np.float64(r64["value"]), r64["terms"].astype(np.float64)
        out[f"{t}_names"] = np.array(names)
        out[f"{t}_dev_torch32"] = np.array([d32[k] for k in names])
        out[f"{t}_dev_chain32"] = np.array([dch[k] for k in names])
        out[f"{t}_max"] = np.array([float(np.max(np.abs(v))) for _, v in sorted(LR.tensors_of(r64).items())])
        print(f"{t}: value {float(r64['value']):.6f} terms {r64['terms']} torch32 {d32['value']:.2e} chain32 {dch['value']:.2e} "
              f"({time.time() - t0:.1f} s)", flush=True)
    np.savez_compressed(LR.GOLDEN, **out)
    print(LR.GOLDEN, os.path.getsize(LR.GOLDEN), "bytes")


if __name__ == "__main__":
    main()

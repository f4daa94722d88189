"""Restatements of the LPIPS rule (include/lp/scg_lpips.h, scgaussian_amd/lpips.py) for the tests.  Own code, no kernel: the
reference's forward walked over a literal module list of vgg16().features,

    rule(x, y, weights, torch.float64)   the yardstick
    rule(x, y, weights, torch.float32)   the same through torch's fp32 convolution
    chain32(x, y, weights)               fp32 with every convolution sum run sequentially in k order: im2col, float32 products,
                                         added one by one as np.cumsum(dtype=float32) adds them — the error a fixed-order fp32 chain has

e_ref of a tensor is the larger of the two fp32 evaluations' deviations from fp64 on the same input; the bar is max(4 e_ref, 1 fp32
ulp of the tensor's largest magnitude) in the max norm, with no exclusion set.  Weights are random but fixed: He-scaled convolution
weights N(0, 2 / (9 cin)), biases N(0, 0.05^2), linear weights U(0, 1), from a seeded CPU generator."""
import os

import numpy as np
import torch
import torch.nn.functional as F

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_lpips.npz")
WEIGHT_SEED = 2024
MARGIN = 4.0

# torchvision's vgg16().features, module by module (cfg 'D': 64 64 M 128 128 M 256 256 256 M 512 512 512 M 512 512 512 M)
CFG = (64, 64, "M", 128, 128, "M", 256, 256, 256, "M", 512, 512, 512, "M", 512, 512, 512, "M")
MODULES = tuple(m for v in CFG for m in (("pool",) if v == "M" else (("conv", v), "relu")))
TARGET_LAYERS = (4, 9, 16, 23, 30)                      # networks.py:93, counted from 1
N_CHANNELS = (64, 128, 256, 512, 512)                   # networks.py:94
MEAN, STD = (-.030, -.088, -.188), (.458, .448, .450)   # networks.py:41-44

# the end-to-end scenes of the fixture: (H, W, seed).  25 x 41: 2 H W = 16 * 128 + 2; 21 x 53: 2 (H / 4)(W / 4) = 128 + 2.
SCENES = ((16, 16, 1), (16, 17, 2), (17, 16, 3), (17, 19, 4), (31, 33, 5), (32, 32, 6), (33, 47, 7), (48, 80, 8), (25, 41, 9),
          (21, 53, 10))


def tag(H, W):
    return f"s{H}x{W}"


def make_weights(seed=WEIGHT_SEED):
    """(convs, lins): 13 (weight (cout,cin,3,3), bias (cout,)) and 5 (1,C,1,1), fp32 CPU tensors."""
    g = torch.Generator().manual_seed(seed)
    convs, cin = [], 3
    for m in MODULES:
        if isinstance(m, tuple):
            cout = m[1]
            convs.append((torch.randn((cout, cin, 3, 3), generator=g) * (2.0 / (9 * cin)) ** 0.5, torch.randn((cout,), generator=g) * 0.05))
            cin = cout
    lins = [torch.rand((1, c, 1, 1), generator=g) for c in N_CHANNELS]
    return convs, lins


def state_dicts(weights, vgg_prefix="features.", published=True):
    """The weights under torchvision's keys (or without the prefix) and the published linear keys (or the reference's renamed)."""
    convs, lins = weights
    idx = [i for i, m in enumerate(MODULES) if isinstance(m, tuple)]
    vgg = {}
    for i, (w, b) in zip(idx, convs):
        vgg[f"{vgg_prefix}{i}.weight"], vgg[f"{vgg_prefix}{i}.bias"] = w, b
    lin = {(f"lin{l}.model.1.weight" if published else f"{l}.1.weight"): w for l, w in enumerate(lins)}
    return vgg, lin


def make_images(H, W, seed):
    """A smooth textured image in [0, 1] and a disturbed copy, (3,H,W) fp32 numpy."""
    rng = np.random.default_rng(seed)
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    x = np.full((3, H, W), 0.5)
    for c in range(3):
        for _ in range(3):
            fx, fy, ph = rng.uniform(-0.9, 0.9), rng.uniform(-0.9, 0.9), rng.uniform(0, 6.28)
            x[c] += 0.13 * np.sin(fx * xx + fy * yy + ph)
    x = np.clip(x + rng.uniform(-0.03, 0.03, x.shape), 0.0, 1.0)
    y = np.clip(x + 0.08 * np.sin(0.7 * xx - 0.4 * yy + rng.uniform(0, 6.28)) + rng.uniform(-0.05, 0.05, x.shape), 0.0, 1.0)
    return x.astype(np.float32), y.astype(np.float32)


def _conv_torch(x, w, b):
    return F.conv2d(x, w.to(x.dtype), b.to(x.dtype), padding=1)


def _conv_chain32(x, w, b):
    """x (1,cin,h,w) fp32 -> (1,cout,h,w): every output an fp32 sum of fp32 products added one after the other in the order
    k = (ky * 3 + kx) * cin + ci from 0, then the bias."""
    _, cin, h, ww = x.shape
    cout = w.shape[0]
    xp = np.pad(x[0].numpy(), ((0, 0), (1, 1), (1, 1)))
    cols = np.stack([xp[:, ky:ky + h, kx:kx + ww] for ky in range(3) for kx in range(3)])          # (9, cin, h, w)
    cols = np.ascontiguousarray(cols.reshape(9 * cin, h * ww).T)                                   # (P, K)
    wk = np.ascontiguousarray(w.numpy().transpose(2, 3, 1, 0).reshape(9 * cin, cout))              # (K, cout)
    # the additions of np.cumsum(products, axis=k, dtype=float32), bit for bit, as a loop over k that keeps the sums in cache
    out = cols[:, 0, None] * wk[0][None]
    for k in range(1, 9 * cin):
        out += cols[:, k, None] * wk[k][None]
    out = out + b.numpy()[None]
    return torch.from_numpy(np.ascontiguousarray(out.T.reshape(1, cout, h, ww)))


def features(x, convs, dtype=torch.float64, conv=_conv_torch):
    """networks.py:53-63 on one image (3,H,W): the five normalised maps, (1,C,h,w) tensors."""
    x = torch.as_tensor(x)[None].to(dtype)
    mean = torch.tensor(MEAN, dtype=torch.float32)[None, :, None, None].to(dtype)          # the buffers are fp32 tensors
    std = torch.tensor(STD, dtype=torch.float32)[None, :, None, None].to(dtype)
    x = (x - mean) / std
    out, it = [], iter(convs)
    for i, m in enumerate(MODULES, 1):
        if isinstance(m, tuple):
            x = conv(x, *next(it))
        elif m == "relu":
            x = torch.relu(x)
        else:
            x = F.max_pool2d(x, 2, 2)
        if i in TARGET_LAYERS:
            out.append(x / (torch.sqrt(torch.sum(x ** 2, dim=1, keepdim=True)) + 1e-10))
        if len(out) == len(TARGET_LAYERS):
            break
    return out


def rule(x, y, weights, dtype=torch.float64, conv=_conv_torch):
    """lpips.py:30-36.  Returns {"value": (), "terms": (5,), "fx": [5 arrays (C,h,w)], "fy": [...]} as numpy in `dtype`."""
    convs, lins = weights
    fx, fy = features(x, convs, dtype, conv), features(y, convs, dtype, conv)
    res = [F.conv2d((a - b) ** 2, l.to(dtype)).mean((2, 3), True) for a, b, l in zip(fx, fy, lins)]
    terms = torch.cat(res, 0)
    return {"value": torch.sum(terms, 0, True).reshape(()).numpy(), "terms": terms.reshape(-1).numpy(),
            "fx": [f[0].numpy() for f in fx], "fy": [f[0].numpy() for f in fy]}


def chain32(x, y, weights):
    return rule(x, y, weights, torch.float32, _conv_chain32)


def tensors_of(r):
    """The named tensors of a rule's result: value, terms, fx0..fx4, fy0..fy4."""
    out = {"value": r["value"], "terms": r["terms"]}
    for side in ("fx", "fy"):
        for l, f in enumerate(r[side]):
            out[f"{side}{l}"] = f
    return out


def deviations(r64, r32):
    """{name: max |r32 - r64|} over tensors_of."""
    a, b = tensors_of(r64), tensors_of(r32)
    return {k: float(np.max(np.abs(b[k].astype(np.float64) - a[k]))) for k in a}


def ulp(wide):
    return float(np.spacing(np.float32(np.max(np.abs(wide)))))


def bar(e_ref, wide):
    """max(4 e_ref, 1 fp32 ulp of the tensor's largest magnitude)."""
    return max(MARGIN * float(e_ref), ulp(wide))


# ---- one layer --------------------------------------------------------------------------------------------------------------
def layer(x, w, b, relu, pool, zscore, dtype=torch.float64, conv=_conv_torch):
    """scg_lp_conv3x3's rule on x (n,cin,h,w): the optional pool or z-score in front, the convolution, the optional ReLU."""
    x = torch.as_tensor(x).to(dtype)
    if zscore:
        x = (x - torch.tensor(MEAN, dtype=torch.float32)[None, :, None, None].to(dtype)) / \
            torch.tensor(STD, dtype=torch.float32)[None, :, None, None].to(dtype)
    if pool:
        x = F.max_pool2d(x, 2, 2)
    out = torch.cat([conv(x[i:i + 1], w, b) for i in range(x.shape[0])])
    return (torch.relu(out) if relu else out).numpy()


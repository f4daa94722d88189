#!/usr/bin/env python3
"""Generate tests/golden/ref_mono.npz by RUNNING the reference's own GaussianModel.create_from_mono (scene/gaussian_model.py:284-360)
on the CPU, through the finder and the device shim of make_golden_model.py.  Only arrays are stored: the inputs, the reference's
outputs, and the uniform numbers its torch.rand calls drew (replayed from the same seed).

The scene: three views of three sizes and FoVs whose names do not sort in the order of the camera list; noise images stored as
bytes; one view without a mask, one with a mask of fractional values and zeros, one with a 0/1 mask; pairs of 2, 65 and 257
matches, a few of them outside [0, 1].

(The smallest pair holds 2 matches, not 1: with a single match the reference's `.squeeze()` at :331 drops the match axis and :333
then fails with "too many indices" — the reference cannot run a pair of one match.  tests/test_gpu_mono.py has segments of 1.)

Asserted here, the seed advanced until both hold:
  * no match is a near tie: fp64 ix or iy within 1e-3 px of an integer AND the mask's taps around that integer differ in zero-ness
    (there the reference's fp32 rounding, not the rule, would decide `valid`);
  * the recorded z_val equals fl(fl(u * fl(far - near)) + near) on the replayed u, bit for bit.

Run:  python tests/golden/make_golden_mono.py      (needs the reference checkout next to the build container; CPU only)
"""
import math
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "ref_mono.npz")
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import make_golden_model as G                                                                # noqa: E402
import mono_refs as MR                                                                       # noqa: E402

SIZES = [(40, 56), (48, 64), (36, 60)]            # (H, W)
FOVS = [52.0, 61.0, 44.0]
NAMES = ["view_c", "view_a", "view_b"]            # the list's order is not the names' sorted order
COUNTS = {(0, 1): 2, (0, 2): 65, (1, 2): 257}
PER_PAIR = ("z_val", "rays_o", "rays_d", "cam_rays_d", "color", "uv", "match_pixel", "blender_mask")
PER_VIEW = ("image_color", "intr", "w2c", "near_far")


def scene(seed):
    rng = np.random.default_rng(seed)
    masks = []
    for i, (H, W) in enumerate(SIZES):
        if i == 0:
            masks.append(None)
        elif i == 1:                               # fractional values, a band of zeros
            m = rng.choice(np.array([0.0, 0.25, 0.5, 1.0]), size=(H, W), p=[0.15, 0.2, 0.2, 0.45])
            m[:, : W // 5] = 0.0
            masks.append(m)
        else:                                      # 0 / 1 with a hole
            m = np.ones((H, W))
            m[H // 3: H // 2, W // 4: W // 2] = 0.0
            masks.append(m)
    cams = MR.cameras(SIZES, rng, masks=masks, fovs=FOVS, names=NAMES)
    md = MR.match_data(cams, COUNTS, rng, lo=-0.03, hi=1.03)
    return cams, md


def near_ties(cams, md):
    """The number of matches at which the reference's rounding could decide the zero-ness of the sampled mask."""
    n = 0
    for cam in cams:
        H, W = np.asarray(cam.image).shape[:2]
        mask = np.ones((H, W)) if cam.blendermask is None else np.asarray(cam.blendermask, dtype=np.float64)
        pad = np.zeros((H + 4, W + 4), dtype=bool)
        pad[2:-2, 2:-2] = mask != 0                                      # outside the image: zero
        for other, m in md[cam.image_name].items():
            m32 = np.asarray(m, dtype=np.float64).astype(np.float32).astype(np.float64)
            ix, iy = ((m32[:, 0] * 2 - 1 + 1) * W - 1) / 2, ((m32[:, 1] * 2 - 1 + 1) * H - 1) / 2
            for x, y in zip(ix, iy):
                kx, ky = int(round(x)), int(round(y))
                if not (-1 <= kx <= W and -1 <= ky <= H):
                    continue
                window = pad[ky + 1: ky + 4, kx + 1: kx + 4]            # the 3 x 3 taps around the nearest integer corner
                if (abs(x - kx) < 1e-3 or abs(y - ky) < 1e-3) and window.any() and not window.all():
                    n += 1
    return n


def main():
    sys.meta_path.insert(0, G._Finder())
    G._cpu_device_shim()
    sys.path.insert(0, G.REF)
    from scene.gaussian_model import GaussianModel

    seed = 2024
    while True:
        cams, md = scene(seed)
        if near_ties(cams, md) == 0:
            break
        seed += 1
    gm = GaussianModel(3)
    torch.manual_seed(seed)
    gm.create_from_mono(cams, md, 1.0)
    torch.manual_seed(seed)
    out = {"seed": np.int64(seed), "sizes": np.array(SIZES), "names": np.array(NAMES)}
    assert list(gm.view_gs.keys()) == NAMES
    for i, cam in enumerate(cams):
        out[f"in_{i}_image"] = np.asarray(cam.image)
        out[f"in_{i}_R"], out[f"in_{i}_T"] = cam.R, cam.T
        out[f"in_{i}_fov"] = np.array([cam.FovX, cam.FovY])
        out[f"in_{i}_near_far"] = np.array(cam.near_far, dtype=np.float64)
        if cam.blendermask is not None:
            out[f"in_{i}_mask"] = np.asarray(cam.blendermask, dtype=np.float32)
            assert np.array_equal(out[f"in_{i}_mask"].astype(np.float64), cam.blendermask)
        v = gm.view_gs[cam.image_name]
        assert (v["height"], v["width"]) == SIZES[i] and set(v) == set(PER_VIEW) | {"height", "width", "match_infos"}
        for k in PER_VIEW:
            out[f"ref_{i}_{k}"] = v[k].detach().numpy().copy()
        for j, other in enumerate(cams):
            if i == j:
                continue
            info = v["match_infos"][other.image_name]
            assert set(info) == set(PER_PAIR)
            M = info["uv"].shape[0]
            u = torch.rand(M, 1).numpy().reshape(M)                        # the replay: same seed, same order of calls
            out[f"in_{i}{j}_match"] = np.asarray(md[cam.image_name][other.image_name], dtype=np.float64)
            out[f"in_{i}{j}_u"] = u
            for k in PER_PAIR:
                out[f"ref_{i}{j}_{k}"] = info[k].detach().numpy().copy()
            nf = v["near_far"].numpy()
            z = u * np.float32(nf[1] - nf[0]) + nf[0]
            assert z.dtype == np.float32 and np.array_equal(z, out[f"ref_{i}{j}_z_val"].reshape(M)), "z_val is not the formula on u"
    for i in range(3):
        for j in range(3):
            if i != j:                               # get_matchloss_from_base's valid_mask, from the reference's own samples
                out[f"ref_{i}{j}_valid"] = (out[f"ref_{i}{j}_blender_mask"] * out[f"ref_{j}{i}_blender_mask"]) > 0
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes;", len(out), "arrays; seed", seed)


if __name__ == "__main__":
    main()

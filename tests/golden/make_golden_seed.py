#!/usr/bin/env python3
"""Generate tests/golden/ref_seed.npz by RUNNING the reference's own GaussianModel.create_from_pcd (scene/gaussian_model.py:362-468)
on the CPU, imported read-only from /root/reference in the build container (stub finder and CPU device shim of
make_golden_model.py).  `distCUDA2`, the third-party extension the reference imports, is bound to oracle/knn_oracle.py's fp32
brute force.  Only input/output arrays are committed.

Scene A: the three 96 x 64 cameras of make_golden_model.py (read back from ref_model.npz); the unordered pairs hold 1, 65 and 257
matches (make_golden_init.make_view_gs) plus a colour per match, an image per view and a near/far pair.
Scene D: seven 96 x 64 views, 21 unordered pairs = 42 segments of 1, 2, 3 and 5 matches.

Planted in min_loss_state (values otherwise uniform in [0, 0.2): about half the matches are kept):
  float32(0.1) exactly (dropped), the float just below it (kept), NaN (dropped), -inf (kept), one whole pair dropped.
Planted in uv, on kept matches: a negative x, an x >= W, a y == H - 0.5, and one pixel hit from two different pairs of one view.

Determinism guard: within every single pair the kept matches hit distinct pixels (a kept match that would repeat a pixel of its
own pair is dropped by raising its min_loss), so the reference's output depends on no index_put order; across pairs the later
pair overwrites, which is the rule "latest in arena order wins".  Every kept point's dist2 is exactly 0 or at least 1e-3 (the seed
is advanced until that holds), so the 1e-7 clamp decides nothing by a rounding.

Inputs are stored flat in arena order (<tag>_in_<name>, <tag>_counts, <tag>_seg_view, <tag>_vhw); per-view images are a formula
(image_of) and are not stored.

Run:  python tests/golden/make_golden_seed.py      (needs /root/reference; CPU only)
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden_init as mgi                                                              # noqa: E402
import make_golden_model as mgm                                                             # noqa: E402  (finder + shim)

OUT = os.path.join(HERE, "ref_seed.npz")
W, H = mgi.W, mgi.H
IN_KEYS = ("rays_o", "rays_d", "color", "uv", "cam_rays_d", "z_val")
OUT_KEYS = ("zval", "rayo", "rayd", "points", "features_dc", "features_rest", "rotation", "opacity", "scaling", "max_radii2D",
            "sparse_depths", "masks", "dist2")


def image_of(v):
    """The (H*W, 3) image of view index v: a formula, so that the fixture need not carry it."""
    i = torch.arange(H * W * 3, dtype=torch.float32).reshape(H * W, 3)
    return ((i * 7 + 13 * v) % 256) / 255


def near_far_of(v):
    return torch.tensor([0.5 + 0.25 * v, 40.0 + v], dtype=torch.float32)


def build_scene(intr, w2c, pair_sizes, seed, order=None):
    """(view_gs in fp32 with the reference's per-view and per-match entries, min_loss_state)."""
    base = mgi.cast(mgi.make_view_gs(intr, w2c, pair_sizes, seed, order=order), torch.float32)
    g = torch.Generator().manual_seed(seed + 7)
    names = list(base)
    state = {}
    for a in names:
        v = int(a[4:])
        base[a]["image_color"], base[a]["near_far"] = image_of(v), near_far_of(v)
        base[a]["intr"], base[a]["w2c"] = base[a]["intr"].float(), base[a]["w2c"].float()
        state[a] = {}
        for b, mi in base[a]["match_infos"].items():
            M = mi["rays_o"].shape[0]
            mi["z_val"] = mi["z_val"].detach()
            mi["color"] = torch.rand(M, 3, generator=g)
            state[a][b] = torch.rand(M, generator=g) * 0.2
    return base, state


def plant(vg, state, big):
    """big: the name pair (a, b) of a segment with at least 12 matches, b2: another pair of the same source view."""
    names = list(vg)
    a, b = big
    s, uv = state[a][b], vg[a]["match_infos"][b]["uv"]
    tenth = torch.tensor(0.1, dtype=torch.float32)
    s[0] = tenth                                                                           # dropped: not below
    s[1] = torch.nextafter(tenth, torch.tensor(0.0))                                       # kept
    s[2] = float("nan")                                                                    # dropped
    s[3] = float("-inf")                                                                   # kept
    s[4:9] = 0.01
    uv[4, 0] = -3.25                                                                       # column 0
    uv[5, 0] = W + 2.5                                                                     # column W - 1
    uv[6, 0] = float(W)                                                                    # x == W: column W - 1
    uv[7, 1] = H - 0.5                                                                     # row H - 1 (the clamp, then truncation)
    uv[8, 1] = -0.75                                                                       # row 0
    # one pixel hit from two different pairs of the view `a`, both kept: the later pair must win
    others = [k for k in vg[a]["match_infos"] if k != b]
    b2 = others[-1]
    later_first = list(vg[a]["match_infos"]).index(b2) > list(vg[a]["match_infos"]).index(b)
    vg[a]["match_infos"][b2]["uv"][0] = torch.floor(uv[9]) + 0.5 + torch.tensor([0.2, -0.2]) * (1 if later_first else -1)
    assert tuple(mgi_pixel(vg[a]["match_infos"][b2]["uv"][0:1])) == tuple(mgi_pixel(uv[9:10]))
    s[9] = 0.02
    state[a][b2][0] = 0.03
    # one whole pair dropped
    for x in names:
        for y in vg[x]["match_infos"]:
            if (x, y) != (a, b) and (x, y) != (a, b2) and state[x][y].numel() >= 2:
                state[x][y][:] = 0.1 + state[x][y]
                return (x, y), b2
    raise SystemExit("no pair left to drop")


def plant_small(vg, state):
    """Scenes of short segments: the four threshold values in the first segment of five matches, the next such segment dropped."""
    tenth = torch.tensor(0.1, dtype=torch.float32)
    fives = [(a, b) for a in vg for b in vg[a]["match_infos"] if state[a][b].numel() == 5]
    (a, b), (x, y) = fives[0], fives[1]
    state[a][b][:4] = torch.stack([tenth, torch.nextafter(tenth, torch.tensor(0.0)), torch.tensor(float("nan")),
                                   torch.tensor(float("-inf"))])
    state[x][y][:] = 0.1 + state[x][y]
    return (x, y), None


def mgi_pixel(uv):
    return [int(t) for t in (uv[:, 1].clamp(0, H - 1).to(torch.int64)[0], uv[:, 0].clamp(0, W - 1).to(torch.int64)[0])]


def make_pairs_distinct(vg, state):
    """Within every pair: a kept match that repeats the pixel of an earlier kept match of the same pair is dropped."""
    dropped = 0
    for a in vg:
        for b, mi in vg[a]["match_infos"].items():
            seen = set()
            row = mi["uv"][:, 1].clamp(0, H - 1).to(torch.int64)
            col = mi["uv"][:, 0].clamp(0, W - 1).to(torch.int64)
            for k in range(row.shape[0]):
                if not bool(state[a][b][k] < 0.1):
                    continue
                px = (int(row[k]), int(col[k]))
                if px in seen:
                    state[a][b][k] = 0.5
                    dropped += 1
                seen.add(px)
    return dropped


def record(GaussianModel, out, tag, intr, w2c, pair_sizes, order, big_of):
    import seed_refs as S
    from oracle import knn_oracle as ko
    for seed in range(2000, 2200):
        vg, state = build_scene(intr, w2c, pair_sizes, seed, order)
        big = big_of(vg) if big_of is not None else None
        dropped_pair, b2 = plant(vg, state, big) if big is not None else plant_small(vg, state)
        n_dup = make_pairs_distinct(vg, state)
        arena = S.arena_from_view_gs(vg, state)
        want = S.seed(arena, S.knn_cpu)
        d2 = want["dist2"]
        if bool(((d2 > 0) & (d2 < 1e-3)).any()):
            print(f"scene {tag} seed {seed}: a dist2 in (0, 1e-3): next seed")
            continue
        break
    else:
        raise SystemExit("no seed keeps dist2 away from the clamp")
    # the guard: distinct pixels within every pair among the kept
    for a in vg:
        for b, mi in vg[a]["match_infos"].items():
            k = state[a][b] < 0.1
            row, col = S.pixel_of(mi["uv"][k], H, W)
            assert len({(int(r), int(c)) for r, c in zip(row, col)}) == int(k.sum()), (a, b)
    assert not bool((state[dropped_pair[0]][dropped_pair[1]] < 0.1).any())
    if big is not None:
        assert bool(state[big[0]][big[1]][9] < 0.1) and bool(state[big[0]][b2][0] < 0.1)
        hit = mgi_pixel(vg[big[0]]["match_infos"][big[1]]["uv"][9:10])
        later = vg[big[0]]["match_infos"][big[1]]
        assert float(want["sparse_depths"][list(vg).index(big[0]), hit[0], hit[1]]) == float(later["z_val"][9, 0] * later["cam_rays_d"][9, 2])

    gm = GaussianModel(3)
    gm.view_gs = vg
    gm.create_from_pcd(state)
    names = list(vg)
    n = gm._zval.shape[0]
    assert 0 < n < arena["z"].numel() and n == want["n"]
    ref = dict(zval=gm._zval, rayo=gm._rayo, rayd=gm._rayd, points=gm.get_xyz, features_dc=gm._features_dc,
               features_rest=gm._features_rest, rotation=gm._rotation, opacity=gm._opacity, scaling=gm._scaling,
               max_radii2D=gm.max_radii2D, sparse_depths=gm.sparse_depths, masks=gm.masks, dist2=d2)
    for k in ("_zval", "_features_dc", "_features_rest", "_scaling", "_rotation", "_opacity"):
        assert isinstance(getattr(gm, k), torch.nn.Parameter) and getattr(gm, k).requires_grad
    for k in ("bg_xyz", "bg_features_dc", "bg_features_rest", "bg_scaling", "bg_rotation", "bg_opacity"):
        assert tuple(getattr(gm, k).shape) == (0,)
    assert gm.curr_scale == 1 and gm.curr_patch_size == 5
    assert torch.equal(gm.img_colors, torch.stack([vg[k]["image_color"].reshape(H, W, 3).permute(2, 0, 1) for k in names]))
    assert torch.equal(gm.intrs, torch.stack([vg[k]["intr"] for k in names])) and gm.img_colors.is_contiguous()
    assert torch.equal(gm.near_fars, torch.stack([vg[k]["near_far"] for k in names]))
    # the restatement agrees with the reference it restates (the CPU test holds the same against the stored arrays)
    for k in S.OUT_KEYS:
        if k == "scaling":
            assert torch.allclose(want[k], ref[k].detach(), rtol=1e-6, atol=0), k
        else:
            assert torch.equal(want[k], ref[k].detach()), k
    # the same-pixel pair: the later pair's depth is what the image holds
    print(f"scene {tag}: seed {seed}, N = {arena['z'].numel()}, n = {n}, {n_dup} in-pair repeats dropped, "
          f"{int(gm.masks.sum())} depth pixels, dist2 min {float(d2.min()):.3e}")
    out[f"{tag}_seed"] = np.array(seed)
    out[f"{tag}_views"] = np.array([int(k[4:]) for k in names])
    out[f"{tag}_vhw"] = np.array([len(names), H, W])
    out[f"{tag}_counts"] = np.array(arena["counts"])
    out[f"{tag}_seg_view"] = np.array(arena["seg_view"])
    out[f"{tag}_pairs"] = np.array([(int(a[4:]), int(b[4:])) for a, b in S.pairs(vg)])
    out[f"{tag}_intr"] = np.stack([vg[k]["intr"].numpy() for k in names])
    out[f"{tag}_w2c"] = np.stack([vg[k]["w2c"].numpy() for k in names])
    for k in IN_KEYS:
        out[f"{tag}_in_{k}"] = np.ascontiguousarray(np.concatenate([vg[a]["match_infos"][b][k].numpy() for a, b in S.pairs(vg)]))
    out[f"{tag}_in_min_loss"] = arena["min_loss"].numpy()
    out[f"{tag}_n"] = np.array(n)
    for k in OUT_KEYS:
        out[f"{tag}_out_{k}"] = np.ascontiguousarray(ref[k].detach().numpy())


def main():
    sys.meta_path.insert(0, mgm._Finder())
    mgm._cpu_device_shim()
    sys.path.insert(0, mgm.REF)
    sys.path.insert(0, mgm.ROOT)
    import scene.gaussian_model as ref_gm
    from oracle import knn_oracle as ko
    ref_gm.distCUDA2 = lambda pts: torch.from_numpy(ko.mean_dist2_bruteforce(pts.detach().numpy()))
    cams = np.load(os.path.join(HERE, "ref_model.npz"))
    intr = [torch.from_numpy(k).double() for k in cams["cam_intr"]]
    w2c = [torch.from_numpy(m).double() for m in cams["cam_w2c"]]
    out = {}
    record(ref_gm.GaussianModel, out, "A", intr, w2c, {(0, 1): 1, (0, 2): 65, (1, 2): 257}, None,
           lambda vg: ("view2", "view1"))
    nv = 7
    intr_d = [mgi.pinhole(100.0 + 7 * i, 104.0 + 5 * i, W / 2 - 1 + 0.5 * i, H / 2 + 1 - 0.5 * i) for i in range(nv)]
    w2c_d = [mgi.look(0.03 * (i - 3) * (-1) ** i, 0.05 * (i - 3), (0.4 * (i - 3), 0.1 * ((3 * i) % 4 - 1.5), 0.05 * i)) for i in range(nv)]
    pairs_d = [(i, j) for i in range(nv) for j in range(i + 1, nv)]
    record(ref_gm.GaussianModel, out, "D", intr_d, w2c_d, {p: (1, 2, 3, 5)[n % 4] for n, p in enumerate(pairs_d)},
           [3, 0, 5, 1, 6, 2, 4], None)
    mgi.write(OUT, out)
    assert os.path.getsize(OUT) < os.path.getsize(os.path.join(HERE, "ref_densify.npz"))


if __name__ == "__main__":
    main()

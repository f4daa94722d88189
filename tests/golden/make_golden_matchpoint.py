#!/usr/bin/env python3
"""Generate tests/golden/ref_matchpoint.npz by RUNNING the reference's own GaussianModel.save_ply_at_matchpoint
(scene/gaussian_model.py:611-642) on the CPU, imported read-only from /root/reference in the build container (stub finder and CPU
device shim of make_golden_model.py).  Its three writers — np.save, torchvision.utils.save_image, storePly — and mkdir_p are
replaced by recorders for the call: the fixture holds the ARRAYS the reference hands them.  Only arrays are committed.

Inputs: scene A and scene D of tests/golden/ref_seed.npz, read back from that file and not stored again, as
tests/matchpoint_refs.golden_arena forms them: scene A's second view cropped to 40 x 70 (so the recorded scene has unequal views
and many matches clamp to its edges), the planted uv of make_golden_seed.py kept (a negative x, x >= W, x == W, y == H - 0.5,
y == -0.75, one pixel hit from two pairs of one view), repeats within a pair moved apart.

Guards: within every single pair all pixels are distinct, so the recording depends on no index_put order (across pairs the later
pair overwrites: "latest in arena order wins"); no plane holds a NaN or a negative zero, so torch's min and max are defined to the
bit; the pixel hit from two pairs holds the later pair's depth.

Per scene <tag>: <tag>_sizes (V,2); <tag>_xyz, <tag>_rgb (N,3) as storePly received them; <tag>_raw_<v>, <tag>_norm_<v> (H,W) as
np.save and save_image received them, v the view's position in the dictionary.

Run:  python tests/golden/make_golden_matchpoint.py      (needs /root/reference; CPU only)
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import make_golden_init as mgi                                                              # noqa: E402  (write)
import make_golden_model as mgm                                                             # noqa: E402  (finder + shim)
import matchpoint_refs as MR                                                                # noqa: E402

OUT = os.path.join(HERE, "ref_matchpoint.npz")


def record(ref_gm, out, fx, tag):
    arena = MR.golden_arena(fx, tag)
    assert MR.pair_pixels_distinct(arena), tag
    assert len(set(arena["sizes"])) == (2 if MR.CROP[tag] else 1)
    vg = MR.view_gs_of(arena)
    keys = list(vg)
    got = {"npy": {}, "png": {}, "dirs": []}

    def save(path, arr):
        got["npy"][os.path.basename(path)] = np.array(arr)

    def save_image(t, path):
        got["png"][os.path.basename(path)] = t.detach().numpy().copy()

    def store_ply(path, xyz, rgb):
        got["ply"] = (os.path.basename(path), np.array(xyz), np.array(rgb))

    gm = ref_gm.GaussianModel(3)
    gm.view_gs = vg
    saved = (np.save, ref_gm.torchvision, ref_gm.storePly, ref_gm.mkdir_p)
    np.save = save
    ref_gm.torchvision = types.SimpleNamespace(utils=types.SimpleNamespace(save_image=save_image))
    ref_gm.storePly, ref_gm.mkdir_p = store_ply, got["dirs"].append
    try:
        gm.save_ply_at_matchpoint(os.path.join("nowhere", "point_cloud_matchpoint.ply"))
    finally:
        np.save, ref_gm.torchvision, ref_gm.storePly, ref_gm.mkdir_p = saved
    assert got["dirs"] == ["nowhere"] and got["ply"][0] == "point_cloud_matchpoint.ply"
    assert sorted(got["npy"]) == sorted(f"{k}.npy" for k in keys) and sorted(got["png"]) == sorted(f"sparsedepth_{k}.png" for k in keys)
    xyz, rgb = got["ply"][1], got["ply"][2]
    N = arena["z"].shape[0]
    assert xyz.dtype == rgb.dtype == np.float32 and xyz.shape == rgb.shape == (N, 3)
    out[f"{tag}_sizes"] = np.array(arena["sizes"])
    out[f"{tag}_xyz"], out[f"{tag}_rgb"] = xyz, rgb
    want = MR.restate(arena)
    hit = 0
    for v, k in enumerate(keys):
        raw, norm = got["npy"][f"{k}.npy"], got["png"][f"sparsedepth_{k}.png"]
        assert raw.dtype == norm.dtype == np.float32 and raw.shape == norm.shape == tuple(arena["sizes"][v])
        assert not np.isnan(raw).any() and not (np.signbit(raw) & (raw == 0)).any() and raw.min() < raw.max()
        out[f"{tag}_raw_{v}"], out[f"{tag}_norm_{v}"] = raw, norm
        hit += int((raw != 0).sum())
        # the restatement agrees with the reference it restates (the CPU test holds the same against the stored arrays)
        assert MR.same_bits(want["planes"][v], raw) and MR.same_bits(want["norm"][v], norm), (tag, k)
    assert MR.same_bits(want["xyz"], xyz) and MR.same_bits(want["rgb"], rgb)
    if tag == "A":                                             # the pixel hit from two pairs of view 2: the later pair's depth stays
        pairs = [tuple(int(x) for x in p) for p in fx["A_pairs"]]
        offs = np.concatenate([[0], np.cumsum(arena["counts"])])
        s_big, s_b2 = pairs.index((2, 1)), pairs.index((2, 0))
        i_big, i_b2 = int(offs[s_big]) + 9, int(offs[s_b2])
        v = arena["seg_view"][s_big]
        H, W = arena["sizes"][v]
        px = MR.pixel_of(*arena["uv"][i_big], H, W)
        assert px == MR.pixel_of(*arena["uv"][i_b2], H, W) and arena["seg_view"][s_b2] == v
        later = max(i_big, i_b2)
        assert got["npy"][f"{keys[v]}.npy"][px] == np.float32(arena["z"][later] * arena["cam_z"][later])
    print(f"scene {tag}: N = {N}, sizes {sorted(set(arena['sizes']))}, {hit} depth pixels")


def main():
    sys.meta_path.insert(0, mgm._Finder())
    mgm._cpu_device_shim()
    sys.path.insert(0, mgm.REF)
    sys.path.insert(0, mgm.ROOT)
    import scene.gaussian_model as ref_gm
    fx = np.load(MR.SEED_GOLDEN)
    out = {}
    for tag in MR.SCENES:
        record(ref_gm, out, fx, tag)
    mgi.write(OUT, out)
    assert os.path.getsize(OUT) < os.path.getsize(MR.SEED_GOLDEN), (os.path.getsize(OUT), os.path.getsize(MR.SEED_GOLDEN))


if __name__ == "__main__":
    main()

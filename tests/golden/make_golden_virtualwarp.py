"""Records tests/golden/ref_virtualwarp.npz from the reference's OWN functions on the CPU in fp32: get_virtual_warp_loss and
get_smooth_loss (utils/loss_utils.py) with both gradients by autograd on a few small scenes of tests/virtualwarp_refs.py, and
get_near_virtual_pose (utils/virtual_poses.py) under a fixed np.random.seed.  The reference tree is needed to run this, not to run
the tests: the fixture is data.

    python tests/golden/make_golden_virtualwarp.py

Per scene <tag> of `scenes`: <tag>_<input> for the seven inputs of the warp loss, <tag>_loss, <tag>_d_img, <tag>_d_depth (upstream
1); <tag>_guide (3,H,W), <tag>_smooth / <tag>_smooth_d_depth per guide form g0 (none), g2 ((H,W): channel 0), g3 ((3,H,W)).
pose_c2ws (n,4,4), pose_near_far, pose_seed, pose_out (3,4)."""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden_model as mgm                                                             # noqa: E402  (where the reference lies)
import virtualwarp_refs as VR                                                               # noqa: E402

OUT = VR.GOLDEN
# H, W, nv, seed: the lowest seed at which the reference's fp32 run has no near tie against fp64 at four times the tests' margin
# (virtualwarp_refs.near_ties with tie = 64)
SCENES = {"a": (13, 17, 3, 36), "b": (9, 11, 2, 1), "c": (20, 19, 1, 1), "d": (3, 5, 3, 1)}


def _load(rel, name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(mgm.REF, rel))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    lu = _load("utils/loss_utils.py", "ref_loss_utils")
    vp = _load("utils/virtual_poses.py", "ref_virtual_poses")
    rec = {"scenes": np.array(list(SCENES))}
    for tag, (H, W, nv, seed) in SCENES.items():
        sc = VR.make_scene(H, W, nv, seed)
        t = VR.tensors(sc)
        img, depth = t["virtual_img"].requires_grad_(True), t["virtual_depth"].reshape(1, H, W).requires_grad_(True)
        loss = lu.get_virtual_warp_loss(img, depth, sc["vir_c2w"], t["intrs"], t["w2cs"], t["img_colors"], t["vir_mask"].reshape(1, H, W))
        loss.backward()
        rec.update({f"{tag}_{k}": sc[k] for k in VR.KEYS})
        rec.update({f"{tag}_loss": loss.detach().numpy(), f"{tag}_d_img": img.grad.numpy(), f"{tag}_d_depth": depth.grad.numpy()[0]})
        guide = VR.make_scene(H, W, 1, seed + 100)["virtual_img"]
        rec[f"{tag}_guide"] = guide
        for form, g in (("g0", None), ("g2", guide[0]), ("g3", guide)):
            d = torch.from_numpy(sc["virtual_depth"]).clone().requires_grad_(True)
            sm = lu.get_smooth_loss(d, None if g is None else torch.from_numpy(g))
            sm.backward()
            rec[f"{tag}_smooth_{form}"], rec[f"{tag}_smooth_d_depth_{form}"] = sm.detach().numpy(), d.grad.numpy()
    rng = np.random.default_rng(3)
    c2ws = np.stack([np.eye(4)] * 4)
    for k in range(4):
        c2ws[k, :3, :3] = VR._rot(rng.uniform(-0.3, 0.3, 3))
        c2ws[k, :3, 3] = rng.uniform(-1.5, 1.5, 3)
    near_far = np.array([[1.2, 7.5], [0.9, 6.0], [1.4, 9.0], [1.1, 8.0]])
    np.random.seed(12345)
    rec.update({"pose_c2ws": c2ws, "pose_near_far": near_far, "pose_seed": np.int64(12345),
                "pose_out": vp.get_near_virtual_pose(c2ws, near_far)})
    np.savez_compressed(OUT, **rec)
    print(OUT, os.path.getsize(OUT), "bytes,", len(SCENES), "scenes")


if __name__ == "__main__":
    main()

"""The reference's init stage as a plain torch loop, and the scenes of tests/golden/ref_init.npz as view_gs dictionaries.

`matchloss_from_base` restates GaussianModel.get_matchloss_from_base (scene/gaussian_model.py:175-239) and `torch_init_loop` the
loop around it (train.py:57-95) in this project's words; tests/test_init_stage_cpu.py holds both to the arrays the reference's
own code produced.  tools/init_stage_timing.py times this loop as the torch leg."""
from __future__ import annotations

import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FLOOR = 2e-5                       # values: floor * max(1, max|ref|)   (the match-loss tests' value floor)
GRAD_FLOOR = 1e-4                  # gradients: floor * max|g|           (the match-loss tests' gradient floor)


def fixture():
    return np.load(os.path.join(GOLDEN, "ref_init.npz"))


def load_scene(fx, tag: str, device="cpu", dtype=torch.float32):
    """view_gs of scene `tag` ("A" or "B") with fresh z_val leaves."""
    cams = np.load(os.path.join(GOLDEN, "ref_model.npz"))
    W, H = (int(v) for v in fx["wh"])
    t = lambda a: torch.from_numpy(np.asarray(a)).to(dtype).to(device)                     # noqa: E731
    vg = {f"view{i}": {"width": W, "height": H, "intr": t(cams["cam_intr"][i]), "w2c": t(cams["cam_w2c"][i]), "match_infos": {}}
          for i in fx[f"{tag}_views"]}
    for a, b in fx[f"{tag}_pairs"]:
        mi = {k: t(fx[f"{tag}_in_{a}{b}_{k}"]) for k in ("uv", "rays_o", "rays_d", "cam_rays_d", "blender_mask", "z_val")}
        mi["z_val"] = mi["z_val"].clone().requires_grad_(True)
        vg[f"view{a}"]["match_infos"][f"view{b}"] = mi
    return vg


def arena(vg):
    return [(a, b) for a in vg for b in vg[a]["match_infos"]]


def flat(vg, nested) -> torch.Tensor:
    return torch.cat([nested[a][b].detach().reshape(-1) for a, b in arena(vg)])


def _reproject(src, dst_view, target_uv, width, height):
    """Loss term of every match of `src` (one direction of a pair) seen from dst_view."""
    pts = src["rays_o"] + src["rays_d"] * src["z_val"]                                      # (M,3)
    cam = pts @ dst_view["w2c"][:3, :3].t() + dst_view["w2c"][:3, 3]
    xyz = cam @ dst_view["intr"].t()
    xy = xyz[:, :2] / (xyz[:, 2:] + 1e-8)
    size = torch.tensor([width, height], dtype=xy.dtype, device=xy.device)
    return ((xy - target_uv).abs() / size).mean(dim=1)


def matchloss_from_base(vg):
    keys = list(vg)
    total, state = 0, {k: {} for k in keys}
    for i, a in enumerate(keys[:-1]):
        for b in keys[i + 1:]:
            ab, ba = vg[a]["match_infos"][b], vg[b]["match_infos"][a]
            width, height = vg[a]["width"], vg[a]["height"]
            valid = (ab["blender_mask"] * ba["blender_mask"]) > 0
            state[a][b] = _reproject(ab, vg[b], ba["uv"], width, height)
            state[b][a] = _reproject(ba, vg[a], ab["uv"], width, height)
            total = total + state[a][b][valid].mean() + state[b][a][valid].mean()
    return total, state


def torch_init_loop(vg, iters, halve_at=(), lr=0.5, loss_scale=5.0, loss_fn=matchloss_from_base, optimizer_cls=torch.optim.Adam,
                    record_losses=True, item_each_iteration=False):
    """train.py:57-95.  Returns dict(losses (list of 0-d tensors), best, min_loss (nested), optimizer).  item_each_iteration: read
    the loss on the host in every iteration, as the reference does for its progress bar (train.py:84)."""
    groups = [{"params": [mi["z_val"] for mi in v["match_infos"].values()], "lr": lr, "name": f"z_val_{k}"} for k, v in vg.items()]
    opt = optimizer_cls(groups, lr=0.0, eps=1e-15)
    z_data = lambda: {a: {b: mi["z_val"].data for b, mi in v["match_infos"].items()} for a, v in vg.items()}   # noqa: E731
    best = min_loss = None
    losses = []
    for it in range(iters):
        if it in halve_at:
            for g in opt.param_groups:
                g["lr"] = g["lr"] * 0.5
        matchloss, state = loss_fn(vg)
        loss = loss_scale * matchloss
        if best is None:
            best, min_loss = z_data(), state                       # aliases the parameters until the first torch.where below
        else:
            cur = z_data()
            for a in state:
                for b in state[a]:
                    keep = min_loss[a][b] < state[a][b]
                    best[a][b] = torch.where(keep.unsqueeze(-1), best[a][b], cur[a][b])
                    min_loss[a][b] = torch.where(keep, min_loss[a][b], state[a][b])
        loss.backward()
        if record_losses:
            losses.append(loss.detach())
        if item_each_iteration:
            loss.item()
        opt.step()
        opt.zero_grad(set_to_none=True)
    return dict(losses=losses, best=best, min_loss=min_loss, optimizer=opt)

"""The reference's init stage as a plain torch loop, and the scenes of tests/golden/ref_init.npz and ref_init_edges.npz as view_gs
dictionaries.

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


def fixture_edges():
    return np.load(os.path.join(GOLDEN, "ref_init_edges.npz"))


_IN_KEYS = ("uv", "rays_o", "rays_d", "cam_rays_d", "blender_mask", "z_val")


def load_scene(fx, tag: str, device="cpu", dtype=torch.float32):
    """view_gs of scene `tag` with fresh z_val leaves, the views in the fixture's dictionary order.  Scenes "A" and "B"
    (ref_init.npz) share one size and take the cameras of ref_model.npz; a scene that carries <tag>_wh / <tag>_intr / <tag>_w2c
    (one row per view, in that order: "C" and "D" of ref_init_edges.npz) has its own, and its inputs flat in arena order."""
    t = lambda a: torch.from_numpy(np.asarray(a)).to(dtype).to(device)                     # noqa: E731
    views = [int(i) for i in fx[f"{tag}_views"]]
    if f"{tag}_wh" in fx.files:
        wh, intr, w2c = fx[f"{tag}_wh"], fx[f"{tag}_intr"], fx[f"{tag}_w2c"]
        vg = {f"view{i}": {"width": int(wh[n][0]), "height": int(wh[n][1]), "intr": t(intr[n]), "w2c": t(w2c[n]), "match_infos": {}}
              for n, i in enumerate(views)}
    else:
        cams = np.load(os.path.join(GOLDEN, "ref_model.npz"))
        W, H = (int(v) for v in fx["wh"])
        vg = {f"view{i}": {"width": W, "height": H, "intr": t(cams["cam_intr"][i]), "w2c": t(cams["cam_w2c"][i]), "match_infos": {}}
              for i in views}
    off = 0
    for n, (a, b) in enumerate(fx[f"{tag}_pairs"]):
        if f"{tag}_counts" in fx.files:
            M = int(fx[f"{tag}_counts"][n])
            mi = {k: t(fx[f"{tag}_in_{k}"][off:off + M]) for k in _IN_KEYS}
            off += M
        else:
            mi = {k: t(fx[f"{tag}_in_{a}{b}_{k}"]) for k in _IN_KEYS}
        mi["z_val"] = mi["z_val"].clone().requires_grad_(True)
        vg[f"view{a}"]["match_infos"][f"view{b}"] = mi
    return vg


def z_of(vg):
    """{a: {b: z_val}}: the depths of view_gs in the nested shape `flat` takes."""
    return {a: {b: mi["z_val"] for b, mi in v["match_infos"].items()} for a, v in vg.items()}


def held(what, got, r64, r32, grad=False):
    """max|got - r64| <= max(4 * e32, floor) (loss_refs.held_to): e32 = max|r32 - r64|, floor = GRAD_FLOOR * max|r64| for a gradient,
    FLOOR * max(1, max|r64|) for every other array."""
    import loss_refs
    as64 = lambda a: np.asarray(a.detach().cpu() if torch.is_tensor(a) else a, dtype=np.float64)          # noqa: E731
    got, r64, r32 = as64(got), as64(r64), as64(r32)
    assert got.shape == r64.shape == r32.shape, (what, got.shape, r64.shape, r32.shape)
    scale = float(np.abs(r64).max())
    floor = GRAD_FLOOR * scale if grad else FLOOR * max(1.0, scale)
    loss_refs.held_to(f"init {what}", float(np.abs(got - r64).max()), float(np.abs(r32 - r64).max()), floor, r64.size)


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

"""Plain-torch restatement of the rule of GaussianModel.create_from_pcd (reference scene/gaussian_model.py:362-468), for the tests
of scgaussian_amd/seed.py and for tools/seed_timing.py.  Test infrastructure: the product never imports it.

Two forms of the same rule:
  seed(arena, dist2_fn)                 flat, over the arena of all ordered pairs; sparse_depths under the rule "the kept match
                                        latest in arena order wins its pixel", formed with an integer amax (any device)
  seed_per_pair(view_gs, state, ...)    the reference's shape: a loop over the ordered pairs with a boolean mask, six gathers and
                                        an indexed write per pair, then the concatenations.  On the CPU the indexed write is serial,
                                        so it gives the flat form's result; on a GPU it is the cost that tools/seed_timing.py times.
An arena is a dict of flat tensors in arena order (for a in views, for b in match_infos[a]): rays_o, rays_d, color (N,3), uv (N,2),
z, cam_z (N), min_loss (N) or None, counts (S) and seg_view (S) as Python lists, and V, H, W.
"""
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "ref_seed.npz")
C0 = 0.28209479177387814                          # utils/sh_utils.py
THRESHOLD = 0.1
SCENES = ("A", "D")
OUT_KEYS = ("zval", "rayo", "rayd", "points", "features_dc", "features_rest", "rotation", "opacity", "scaling", "max_radii2D",
            "sparse_depths", "masks")


def fixture():
    return np.load(GOLDEN)


def pairs(view_gs):
    return [(a, b) for a in view_gs for b in view_gs[a]["match_infos"]]


def arena_from_view_gs(view_gs, min_loss_state=None, device=None):
    keys = list(view_gs)
    ps = pairs(view_gs)
    infos = [view_gs[a]["match_infos"][b] for a, b in ps]
    dev = device if device is not None else infos[0]["rays_o"].device
    cat = lambda k: torch.cat([i[k].detach().float().to(dev) for i in infos])              # noqa: E731
    sizes = {(int(view_gs[k]["height"]), int(view_gs[k]["width"])) for k in keys}
    assert len(sizes) == 1, sizes
    (H, W), = sizes
    return dict(rays_o=cat("rays_o"), rays_d=cat("rays_d"), color=cat("color"), uv=cat("uv"), z=cat("z_val").reshape(-1),
                cam_z=cat("cam_rays_d")[:, 2].contiguous(),
                min_loss=None if min_loss_state is None else torch.cat([min_loss_state[a][b].detach().float().reshape(-1).to(dev)
                                                                        for a, b in ps]),
                counts=[int(i["rays_o"].shape[0]) for i in infos], seg_view=[keys.index(a) for a, _b in ps], V=len(keys), H=H, W=W)


def load_arena(fx, tag, device="cpu"):
    t = lambda k: torch.from_numpy(fx[f"{tag}_in_{k}"]).contiguous().to(device)           # noqa: E731
    return dict(rays_o=t("rays_o"), rays_d=t("rays_d"), color=t("color"), uv=t("uv"), z=t("z_val").reshape(-1),
                cam_z=t("cam_rays_d")[:, 2].contiguous(), min_loss=t("min_loss"), counts=[int(c) for c in fx[f"{tag}_counts"]],
                seg_view=[int(v) for v in fx[f"{tag}_seg_view"]], V=int(fx[f"{tag}_vhw"][0]), H=int(fx[f"{tag}_vhw"][1]),
                W=int(fx[f"{tag}_vhw"][2]))


def view_gs_of(arena, extras=None):
    """A reference-shaped view_gs around the arena's tensors (views of the flat tensors, in arena order).  The partner of pair
    (a, b) is named by walking each source view's pairs over the other views in order, as the golden scenes are built.  extras:
    {view index: dict of further per-view entries}."""
    V, H, W = arena["V"], arena["H"], arena["W"]
    dev = arena["z"].device
    names = [f"view{v}" for v in range(V)]
    vg = {n: {"height": H, "width": W, "match_infos": {}, "intr": torch.eye(3, device=dev), "w2c": torch.eye(4, device=dev),
              "near_far": torch.tensor([0.5, 50.0], device=dev), "image_color": torch.zeros(H * W, 3, device=dev)} for n in names}
    for v, e in (extras or {}).items():
        vg[names[v]].update(e)
    off, seen = 0, {}
    cam = torch.zeros(arena["z"].numel(), 3, device=dev)
    cam[:, 2] = arena["cam_z"]
    for M, a in zip(arena["counts"], arena["seg_view"]):
        k = seen.get(a, 0)
        seen[a] = k + 1
        others = [v for v in range(V) if v != a]
        b = names[others[k]] if k < len(others) else f"extra{k}"
        sl = slice(off, off + M)
        vg[names[a]]["match_infos"][b] = dict(rays_o=arena["rays_o"][sl], rays_d=arena["rays_d"][sl], color=arena["color"][sl],
                                              uv=arena["uv"][sl], z_val=arena["z"][sl].view(M, 1), cam_rays_d=cam[sl],
                                              blender_mask=torch.ones(M, device=dev))
        off += M
    return vg


def nested_state(view_gs, flat):
    out, off = {}, 0
    for a, b in pairs(view_gs):
        M = view_gs[a]["match_infos"][b]["rays_o"].shape[0]
        out.setdefault(a, {})[b] = flat[off:off + M]
        off += M
    return out


def keep_mask(arena, threshold=THRESHOLD):
    if arena["min_loss"] is None:
        return torch.ones_like(arena["z"], dtype=torch.bool)
    return arena["min_loss"] < threshold                            # fp32 against float32(threshold); a NaN compares false


def raw_opacity(n, device):
    x = 0.1 * torch.ones((n, 1), dtype=torch.float32, device=device)
    return torch.log(x / (1 - x))


def scales_of(dist2):
    return torch.log(torch.sqrt(torch.clamp_min(dist2, 0.0000001)))[..., None].repeat(1, 3)


def rgb2sh(color):
    """(rgb - 0.5) / C0 with a correctly rounded fp32 division on every device: the reference's tensor / Python-scalar form divides
    on the CPU, where the fixtures are recorded, but a GPU's scalar division multiplies by the rounded reciprocal.  A tensor
    divisor is divided by everywhere."""
    return (color - 0.5) / torch.full_like(color, C0)


def pixel_of(uv, H, W):
    return uv[:, 1].clamp(0, H - 1).to(torch.int64), uv[:, 0].clamp(0, W - 1).to(torch.int64)


def seed(arena, dist2_fn, threshold=THRESHOLD):
    """Every tensor create_from_pcd derives from the matches, the flat way.  dist2_fn: points (n,3) -> (n)."""
    dev = arena["z"].device
    V, H, W = arena["V"], arena["H"], arena["W"]
    N = arena["z"].numel()
    keep = keep_mask(arena, threshold)
    idx = keep.nonzero()[:, 0]
    n = idx.numel()
    z = arena["z"][idx]
    rayo, rayd = arena["rays_o"][idx], arena["rays_d"][idx]
    points = rayo + rayd * z[:, None]
    out = dict(n=n, keep=keep, zval=z[:, None], rayo=rayo, rayd=rayd, points=points,
               features_dc=rgb2sh(arena["color"][idx])[:, None, :],
               features_rest=torch.zeros(n, 15, 3, device=dev), rotation=torch.zeros(n, 4, device=dev),
               opacity=raw_opacity(n, dev), max_radii2D=torch.zeros(n, device=dev))
    out["rotation"][:, 0] = 1
    out["dist2"] = dist2_fn(points) if n > 0 else torch.zeros(0, device=dev)
    out["scaling"] = scales_of(out["dist2"])
    # sparse depths: the kept match latest in arena order wins its pixel
    view = torch.repeat_interleave(torch.tensor(arena["seg_view"], dtype=torch.int64, device=dev),
                                   torch.tensor(arena["counts"], dtype=torch.int64, device=dev), output_size=N)
    writes = keep & torch.isfinite(arena["uv"]).all(dim=1)
    wi = writes.nonzero()[:, 0]
    row, col = pixel_of(torch.nan_to_num(arena["uv"][wi]), H, W)
    lin = (view[wi] * H + row) * W + col
    winner = torch.full((V * H * W,), -1, dtype=torch.int64, device=dev)
    winner.scatter_reduce_(0, lin, wi, reduce="amax", include_self=True)
    depth = arena["z"] * arena["cam_z"]
    sparse = torch.where(winner >= 0, depth[winner.clamp_min(0)], torch.zeros((), device=dev)) if N > 0 else \
        torch.zeros(V * H * W, device=dev)
    out["sparse_depths"] = sparse.reshape(V, H, W)
    out["masks"] = out["sparse_depths"] > 0
    return out


def seed_per_pair(view_gs, min_loss_state, dist2_fn, threshold=THRESHOLD):
    """The same rule in the reference's shape: per ordered pair a mask, six boolean gathers and an indexed write."""
    zvals, rayos, rayds, colors, points, sparse = [], [], [], [], [], []
    for a, vgs in view_gs.items():
        H, W = vgs["height"], vgs["width"]
        sd = None
        for b, m in vgs["match_infos"].items():
            if sd is None:
                sd = torch.zeros(H, W, dtype=torch.float32, device=m["rays_o"].device)
            keep = (min_loss_state[a][b] < threshold) if min_loss_state is not None else torch.ones_like(m["rays_o"][:, 0]) > 0
            o, d, z, c, uv, cr = (m[k][keep] for k in ("rays_o", "rays_d", "z_val", "color", "uv", "cam_rays_d"))
            sd[pixel_of(uv, H, W)] = z.squeeze(-1) * cr[:, 2]
            points.append(o + d * z)
            zvals.append(z)
            rayos.append(o)
            rayds.append(d)
            colors.append(c)
        sparse.append(sd if sd is not None else torch.zeros(H, W))
    zval, rayo, rayd, color, pts = (torch.cat(t) for t in (zvals, rayos, rayds, colors, points))
    n, dev = zval.shape[0], zval.device
    sh = rgb2sh(color)
    features = torch.zeros((n, 3, 16), dtype=torch.float32, device=dev)
    features[:, :3, 0] = sh
    dist2 = dist2_fn(pts) if n > 0 else torch.zeros(0, device=dev)
    rotation = torch.zeros((n, 4), device=dev)
    rotation[:, 0] = 1
    sparse_depths = torch.stack(sparse)
    return dict(n=n, zval=zval, rayo=rayo, rayd=rayd, points=pts, features_dc=features[:, :, 0:1].transpose(1, 2).contiguous(),
                features_rest=features[:, :, 1:].transpose(1, 2).contiguous(), rotation=rotation, opacity=raw_opacity(n, dev),
                dist2=dist2, scaling=scales_of(dist2), max_radii2D=torch.zeros(n, device=dev), sparse_depths=sparse_depths,
                masks=sparse_depths > 0)


def knn_cpu(points):
    """distCUDA2 on the CPU: the oracle's fp32 brute force."""
    from oracle import knn_oracle as ko
    return torch.from_numpy(ko.mean_dist2_bruteforce(points.detach().cpu().numpy())).to(points.device)


def ulp_distance(a, b):
    """Element-wise distance in units in the last place between two fp32 tensors of finite values."""
    def ordered(t):
        i = t.contiguous().view(torch.int32).to(torch.int64)
        return torch.where(i < 0, -(i & 0x7FFFFFFF), i)
    return (ordered(a) - ordered(b)).abs()

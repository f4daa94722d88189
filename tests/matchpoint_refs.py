"""The init stage's snapshot restated in numpy, for tests/test_matchpoint_cpu.py and tests/test_gpu_matchpoint.py
(include/mp/scg_matchpoint.h states the rule).  Written here from the rule; test infrastructure: the product never imports it.

An arena is a dict of flat float32 arrays in arena order (for a in views, for b in match_infos[a]): rays_o, rays_d, color (N,3),
uv (N,2), z, cam_z (N); counts (S) and seg_view (S) as lists; sizes: the views' [(H, W)].  restate(arena) walks it one match at a
time in arena order (a later match overwrites an earlier one: "latest in arena order wins") and gives

    xyz (N,3), rgb (N,3)      what storePly is handed: rays_o + rays_d * z and color * 255, one rounding per operation
    body (N,27) uint8         the PLY records: x y z, zero normals, the byte rule of tests/ply_refs.py on rgb
    planes [(H,W)]            the sparse depths
    norm [(H,W)]              (d - min) / (max - min), what save_image is handed
    bytes [(H,W)] uint8       the quantiser of tests/eval_refs.py on norm
    ranges (V,2)              (min, max): a NaN wins; among zeros of both signs min is -0.0 and max +0.0

golden_arena(fx, tag) is the recorded scene of tests/golden/ref_matchpoint.npz: scene `tag` of tests/golden/ref_seed.npz read
back, one view cropped, repeats within a pair moved apart.  make_golden_matchpoint.py and the tests build it from here.
"""
import os

import numpy as np
import torch

import eval_refs as E
import ply_refs as P

f32 = np.float32
HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "ref_matchpoint.npz")
SEED_GOLDEN = os.path.join(HERE, "golden", "ref_seed.npz")
SCENES = ("A", "D")
IN_KEYS = ("rays_o", "rays_d", "color", "uv", "z", "cam_z")
CROP = {"A": {1: (40, 70)}, "D": {}}                     # view index -> (H, W): scene A's second view is smaller than the others
# the uv make_golden_seed.py planted, as {(source view, partner view): match indices}: they stay where they are
PLANTED = {"A": {(2, 1): range(4, 10), (2, 0): [0]}, "D": {}}


def bits(a):
    return np.ascontiguousarray(a, dtype=f32).view(np.uint32)


def same_bits(a, b):
    """Equal bit patterns, or NaN on both sides (the payload of a NaN an operation produces is the processor's choice)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind != "f":
        return bool(np.array_equal(a, b))
    return bool(np.all((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))))


def pixel_of(u, v, H, W):
    """(row, col) of a finite uv: the clamp acts on the float, the cast truncates."""
    return int(min(max(float(v), 0.0), float(H - 1))), int(min(max(float(u), 0.0), float(W - 1)))


def view_of_match(arena):
    return np.repeat(np.asarray(arena["seg_view"], dtype=np.int64), np.asarray(arena["counts"], dtype=np.int64))


def plane_range(p):
    """(min, max) of a plane as float32: a NaN wins; -0.0 lies below +0.0."""
    if np.isnan(p).any():
        return f32(np.nan), f32(np.nan)
    mn, mx = p.min(), p.max()
    zeros = p[p == 0]
    if mn == 0:
        mn = f32(-0.0) if np.signbit(zeros).any() else f32(0.0)
    if mx == 0:
        mx = f32(0.0) if (~np.signbit(zeros)).any() else f32(-0.0)
    return f32(mn), f32(mx)


def normalise(p, mn, mx):
    with np.errstate(all="ignore"):
        num = (p - mn).astype(f32)
        den = f32(mx - mn)
        return (num / den).astype(f32)


def records(xyz, rgb_bytes):
    n = xyz.shape[0]
    rec = np.zeros((n, 27), np.uint8)
    rec[:, :12] = bits(xyz).view(np.uint8).reshape(n, 12)
    rec[:, 24:] = rgb_bytes
    return rec


def restate(arena):
    a = {k: np.ascontiguousarray(arena[k], dtype=f32) for k in IN_KEYS}
    N = a["z"].shape[0]
    assert sum(arena["counts"]) == N and len(arena["counts"]) == len(arena["seg_view"])
    with np.errstate(all="ignore"):
        prod = (a["rays_d"] * a["z"][:, None]).astype(f32)                 # one rounding
        xyz = (a["rays_o"] + prod).astype(f32)                             # and another
        rgb = (a["color"] * f32(255.0)).astype(f32)
        depth = (a["z"] * a["cam_z"]).astype(f32)
    planes = [np.zeros((H, W), f32) for H, W in arena["sizes"]]
    view = view_of_match(arena)
    for i in range(N):                                                     # arena order: the latest write stays
        u, v = a["uv"][i]
        if np.isfinite(u) and np.isfinite(v):
            H, W = arena["sizes"][view[i]]
            planes[view[i]][pixel_of(u, v, H, W)] = depth[i]
    ranges = np.array([plane_range(p) for p in planes], dtype=f32).reshape(len(planes), 2)
    norm = [normalise(p, mn, mx) for p, (mn, mx) in zip(planes, ranges)]
    q = [E.quantise(torch.from_numpy(n)).numpy() for n in norm]
    return dict(xyz=xyz, rgb=rgb, body=records(xyz, P.byte_rule(rgb)), planes=planes, norm=norm, bytes=q, ranges=ranges)


def ply_bytes(r):
    """The point-cloud file of a restatement: header and records."""
    n = r["body"].shape[0]
    return P.header(P.COLOR_NAMES, n, ["float"] * 6 + ["uchar"] * 3) + r["body"].tobytes()


def random_arena(counts, seg_view, sizes, seed=0, spill=2.0):
    """Ordinary values: uv up to `spill` pixels outside its view on every side, depths of both signs away from zero."""
    rng = np.random.default_rng(seed)
    N = int(sum(counts))
    view = np.repeat(np.asarray(seg_view, dtype=np.int64), np.asarray(counts, dtype=np.int64))
    hw = np.asarray(sizes, dtype=np.float64).reshape(-1, 2)[view] if N else np.zeros((0, 2))
    uv = np.stack([rng.uniform(-spill, hw[:, 1] + spill), rng.uniform(-spill, hw[:, 0] + spill)], 1).astype(f32)
    d = rng.normal(size=(N, 3))
    return dict(rays_o=rng.uniform(-1, 1, (N, 3)).astype(f32), rays_d=(d / np.linalg.norm(d, axis=1, keepdims=True)).astype(f32),
                color=rng.uniform(0, 1, (N, 3)).astype(f32), uv=uv, z=(rng.uniform(2, 8, N) * rng.choice([1, 1, 1, -1], N)).astype(f32),
                cam_z=rng.uniform(0.5, 1.0, N).astype(f32), counts=[int(c) for c in counts], seg_view=[int(v) for v in seg_view],
                sizes=[(int(h), int(w)) for h, w in sizes])


def view_gs_of(arena, device="cpu"):
    """A reference-shaped view_gs over the arena: views "view<v>", each pair's partner named by the order of the pairs of its
    source view ("to<k>"), every tensor a slice of one flat tensor per input."""
    t = {k: torch.from_numpy(np.ascontiguousarray(arena[k], dtype=f32)).to(device) for k in IN_KEYS}
    cam = torch.zeros(t["z"].numel(), 3, device=device)
    cam[:, 2] = t["cam_z"]
    vg = {f"view{v}": {"height": H, "width": W, "match_infos": {}} for v, (H, W) in enumerate(arena["sizes"])}
    off = 0
    for M, v in zip(arena["counts"], arena["seg_view"]):
        mi = vg[f"view{v}"]["match_infos"]
        sl = slice(off, off + M)
        mi[f"to{len(mi)}"] = dict(rays_o=t["rays_o"][sl], rays_d=t["rays_d"][sl], color=t["color"][sl], uv=t["uv"][sl],
                                  z_val=t["z"][sl].view(M, 1), cam_rays_d=cam[sl])
        off += M
    return vg


def golden_arena(fx, tag):
    """Scene `tag` of ref_seed.npz (fx: the loaded file) as the recorded snapshot scene: the views of CROP[tag] made smaller, and
    within every pair a match that repeats the pixel of another match of its pair moved to the centre of the next pixel no match
    of the pair uses (row-major, wrapping), the planted matches left where they are.  The recording then depends on no
    index_put order.  Every match counts here: the snapshot has no threshold."""
    V, H, W = (int(x) for x in fx[f"{tag}_vhw"])
    sizes = [CROP[tag].get(v, (H, W)) for v in range(V)]
    arena = dict(rays_o=fx[f"{tag}_in_rays_o"], rays_d=fx[f"{tag}_in_rays_d"], color=fx[f"{tag}_in_color"],
                 uv=np.array(fx[f"{tag}_in_uv"], dtype=f32), z=fx[f"{tag}_in_z_val"].reshape(-1),
                 cam_z=np.ascontiguousarray(fx[f"{tag}_in_cam_rays_d"][:, 2]), counts=[int(c) for c in fx[f"{tag}_counts"]],
                 seg_view=[int(v) for v in fx[f"{tag}_seg_view"]], sizes=sizes)
    views = [int(v) for v in fx[f"{tag}_views"]]                           # arena view index -> the number in its name
    pairs = [(int(a), int(b)) for a, b in fx[f"{tag}_pairs"]]
    off = 0
    for (a, b), M, v in zip(pairs, arena["counts"], arena["seg_view"]):
        assert views[v] == a
        Hv, Wv = sizes[v]
        uv = arena["uv"][off:off + M]
        fixed = set(PLANTED[tag].get((a, b), ()))
        px = [pixel_of(uv[k, 0], uv[k, 1], Hv, Wv) for k in range(M)]
        used = {px[k] for k in fixed}
        assert len(used) == len(fixed)
        for k in range(M):
            if k in fixed:
                continue
            r, c = px[k]
            while (r, c) in used:
                lin = (r * Wv + c + 1) % (Hv * Wv)
                r, c = divmod(lin, Wv)
            if (r, c) != px[k]:
                uv[k] = (c + 0.5, r + 0.5)
            used.add((r, c))
        off += M
    return arena


def pair_pixels_distinct(arena):
    off = 0
    for M, v in zip(arena["counts"], arena["seg_view"]):
        H, W = arena["sizes"][v]
        px = {pixel_of(u, w, H, W) for u, w in arena["uv"][off:off + M]}
        if len(px) != M:
            return False
        off += M
    return True

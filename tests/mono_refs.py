"""The scene setup (include/scg_mono.h) restated in numpy, operation by operation, and a plain-torch form of the reference's loop.

restate(plan)            what the three kernels write, from a mono.MonoPlan's staged inputs: the sampler in float32 with every
                         operation rounded on its own, the ray chain in float64 with explicit sums (no BLAS call, which may fuse).
                         The GPU tests demand these bits.
restate(plan, wide=True) the same rule with the sampler in float64 and no rounding of the rays on the store: the yardstick both
                         the kernels and the reference's fp32 operators are measured against.
torch_loop(...)          scene/gaussian_model.py:284-360 in plain torch, operator for operator, for tools/mono_timing.py.
cameras(...)             simple camera objects for tests and the timing tool.
"""
import math
import types

import numpy as np
import torch

F = np.float32


def camera(name, image, R, T, FovX, FovY, near_far, blendermask=None):
    return types.SimpleNamespace(image_name=name, image=image, R=np.asarray(R, dtype=np.float64), T=np.asarray(T, dtype=np.float64),
                                 FovX=float(FovX), FovY=float(FovY), near_far=list(near_far), blendermask=blendermask)


def rot(ax, ay, az=0.0):
    cx, sx, cy, sy, cz, sz = math.cos(ax), math.sin(ax), math.cos(ay), math.sin(ay), math.cos(az), math.sin(az)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def cameras(sizes, rng, masks=None, fovs=None, names=None):
    """One camera per (H, W) of `sizes` with a noise image; masks: per view None or an (H, W) array."""
    cams = []
    for i, (H, W) in enumerate(sizes):
        fovx = math.radians(fovs[i] if fovs else 50.0 + 7.0 * i)
        fovy = 2 * math.atan(math.tan(fovx / 2) * H / W)
        img = rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)
        cams.append(camera(names[i] if names else f"view{i}", img, rot(0.03 * i, -0.08 * i, 0.02 * i), (0.4 * i, -0.1 * i, 0.05 * i),
                           fovx, fovy, (0.5 + 0.25 * i, 7.0 + i), None if masks is None else masks[i]))
    return cams


def match_data(cams, counts, rng, lo=-0.02, hi=1.02):
    """{a: {b: (M, 2) float64 in [lo, hi)}}; counts: {(i, j) with i < j: M} (both directions get M) or one int for every pair."""
    out = {c.image_name: {} for c in cams}
    for i, a in enumerate(cams):
        for j, b in enumerate(cams):
            if i != j:
                M = counts if isinstance(counts, int) else counts[(min(i, j), max(i, j))]
                out[a.image_name][b.image_name] = rng.uniform(lo, hi, size=(M, 2))
    return out


def sample(img, msk, mp, H, W, dt=F):
    """grid_sample(bilinear, zeros, align_corners=False) in its device form at the (M, 2) fp32 match pixels `mp`, in dtype `dt`.
    img: (H, W, 3) fp32; msk: (H, W) fp32 or None (a plane of ones).  Returns colour (M, 3) and mask (M) in `dt`."""
    one, two = dt(1), dt(2)
    with np.errstate(all="ignore"):
        m = mp.astype(dt)
        gx, gy = m[:, 0] * two - one, m[:, 1] * two - one
        ix = ((gx + one) * dt(W) - one) / two
        iy = ((gy + one) * dt(H) - one) / two
        xf, yf = np.floor(ix), np.floor(iy)
        ok = ~(np.isnan(ix) | np.isnan(iy)) & (np.abs(xf) < dt(2147483648.0)) & (np.abs(yf) < dt(2147483648.0))
        x1, y1 = xf + one, yf + one
        weights = ((x1 - ix) * (y1 - iy), (ix - xf) * (y1 - iy), (x1 - ix) * (iy - yf), (ix - xf) * (iy - yf))      # nw ne sw se
        col, bm = np.zeros((len(m), 3), dtype=dt), np.zeros(len(m), dtype=dt)
        for q, w in enumerate(weights):
            x, y = xf.astype(np.float64) + (q & 1), yf.astype(np.float64) + (q >> 1)
            inb = ok & (x >= 0) & (x < W) & (y >= 0) & (y < H)
            xi, yi = np.where(inb, x, 0).astype(np.int64), np.where(inb, y, 0).astype(np.int64)
            v = img[yi, xi].astype(dt)
            mv = msk[yi, xi].astype(dt) if msk is not None else np.ones(len(m), dtype=dt)
            for c in range(3):
                col[:, c] = np.where(inb, col[:, c] + v[:, c] * w, col[:, c])
            bm = np.where(inb, bm + mv * w, bm)
    return col, bm


def rays(c, uv32):
    """The fp64 chain of scene/gaussian_model.py:330-336 on the fp32 uv, from view_constants: explicit sums, left to right.
    Returns rays_o, rays_d, cam_rays_d (M, 3) in float64."""
    K, Rc, Rw, o = c["Kinv"], c["c2w"][:3, :3], c["Rw2c"], c["c2w"][:3, 3]
    u, v = uv32[:, 0].astype(np.float64), uv32[:, 1].astype(np.float64)
    with np.errstate(all="ignore"):
        p = [K[r, 0] * u + K[r, 1] * v + K[r, 2] for r in range(3)]
        n = np.sqrt(p[0] * p[0] + p[1] * p[1] + p[2] * p[2]) + 1e-8
        d = [p[r] / n for r in range(3)]
        rd = [Rc[r, 0] * d[0] + Rc[r, 1] * d[1] + Rc[r, 2] * d[2] for r in range(3)]
        cd = [Rw[r, 0] * rd[0] + Rw[r, 1] * rd[1] + Rw[r, 2] * rd[2] for r in range(3)]
    return np.broadcast_to(o, (len(u), 3)).copy(), np.stack(rd, 1), np.stack(cd, 1)


def _staged(plan, name):
    off, shape, dtype = plan.regions[name]
    raw = plan._staged[name]
    return raw.view({torch.float32: np.float32, torch.uint8: np.uint8}[dtype]).reshape(shape)


def restate(plan, wide=False):
    """Every array the kernels write, flat in arena order, as numpy; wide: the float64 yardstick (see the module's docstring)."""
    dt = np.float64 if wide else F
    out_t = (lambda a: a) if wide else (lambda a: a.astype(F))
    mp, u, bytes_ = _staged(plan, "match_pixel"), _staged(plan, "u"), _staged(plan, "image_bytes")
    masks = _staged(plan, "masks")
    tab = plan._staged["tab_views"].view(plan_view_dtype())
    image_color = bytes_.astype(F) / F(255)
    N = plan.N
    res = {k: np.zeros((N, 3), dtype=dt) for k in ("color", "rays_o", "rays_d", "cam_rays_d")}
    res.update(uv=np.zeros((N, 2), dtype=F), blender_mask=np.zeros(N, dtype=dt), z=np.zeros(N, dtype=F))
    for (a, _b, off, M) in plan.segments:
        i = plan.keys.index(a)
        c, rec = plan.consts[i], tab[i]
        H, W = c["H"], c["W"]
        m = mp[off:off + M]
        with np.errstate(all="ignore"):
            uv = np.stack([m[:, 0] * F(W), m[:, 1] * F(H)], 1)
        p0 = int(rec["image_off"])
        img = image_color[3 * p0:3 * (p0 + H * W)].reshape(H, W, 3)
        msk = masks[int(rec["mask_off"]):int(rec["mask_off"]) + H * W].reshape(H, W) if rec["mask_off"] >= 0 else None
        col, bm = sample(img, msk, m, H, W, dt)
        ro, rd, cd = rays(c, uv)
        near, far = plan.near_far[i]
        with np.errstate(all="ignore"):
            z = u[off:off + M] * F(far - near) + near
        s = slice(off, off + M)
        res["uv"][s], res["color"][s], res["blender_mask"][s], res["z"][s] = uv, col, bm, z
        res["rays_o"][s], res["rays_d"][s], res["cam_rays_d"][s] = out_t(ro), out_t(rd), out_t(cd)
    res["cam_z"] = res["cam_rays_d"][:, 2].copy()
    res["image_color"] = image_color.reshape(-1, 3)
    # ---- the pairs ------------------------------------------------------------------------------------------------------------
    index = {(a, b): s for s, (a, b, _o, _M) in enumerate(plan.segments)}
    res["uv_t"], res["valid"], res["wgt"] = np.zeros((N, 2), dtype=F), np.zeros(N, dtype=F), np.zeros(N, dtype=F)
    res["counts"] = np.zeros(plan.nseg, dtype=np.int32)
    bm32 = res["blender_mask"].astype(F)
    for s, (a, b, off, M) in enumerate(plan.segments):
        _a, _b, poff, _M = plan.segments[index[(b, a)]]
        res["uv_t"][off:off + M] = res["uv"][poff:poff + M]
        with np.errstate(all="ignore"):
            valid = ((bm32[off:off + M] * bm32[poff:poff + M]) > 0).astype(F)
        n = int(valid.sum(dtype=np.float64))
        res["valid"][off:off + M], res["counts"][s] = valid, n
        res["wgt"][off:off + M] = valid / F(n) if n > 0 else 0
    return res


def fixture_scene(z):
    """tests/golden/ref_mono.npz -> (cams, match_data, u (N) in arena order, ref): ref holds the reference's per-pair outputs flat
    in arena order under the kernels' names (z for z_val; valid as float32) and its per-view ones as lists."""
    names = [str(n) for n in z["names"]]
    V = len(names)
    cams = [camera(names[i], z[f"in_{i}_image"], z[f"in_{i}_R"], z[f"in_{i}_T"], *z[f"in_{i}_fov"], z[f"in_{i}_near_far"],
                   z[f"in_{i}_mask"].astype(np.float64) if f"in_{i}_mask" in z else None) for i in range(V)]
    pairs = [(i, j) for i in range(V) for j in range(V) if i != j]
    md = {n: {} for n in names}
    for i, j in pairs:
        md[names[i]][names[j]] = z[f"in_{i}{j}_match"]
    cat = lambda k: np.concatenate([z[f"ref_{i}{j}_{k}"] for i, j in pairs])                # noqa: E731
    ref = {k: cat(k) for k in ("rays_o", "rays_d", "cam_rays_d", "color", "uv", "blender_mask")}
    ref["z"] = cat("z_val").reshape(-1)
    ref["valid"] = cat("valid").astype(F)
    for k in ("image_color", "intr", "w2c", "near_far"):
        ref[k] = [z[f"ref_{i}_{k}"] for i in range(V)]
    return cams, md, np.concatenate([z[f"in_{i}{j}_u"] for i, j in pairs]), ref


def bar(ref, wide):
    """The tolerance of an array against the float64 yardstick `wide`: max(4 e_ref, 1 fp32 ulp), e_ref the reference's own largest
    deviation from it, the ulp that of the array's largest magnitude.  Returns (bar, e_ref)."""
    e_ref = float(np.max(np.abs(ref.astype(np.float64) - wide)))
    return max(4 * e_ref, float(np.spacing(F(np.max(np.abs(wide)))))), e_ref


def plan_view_dtype():
    from scgaussian_amd import mono
    return mono._VIEW_DTYPE


def torch_loop(cams, match_data, device):
    """scene/gaussian_model.py:284-360 in plain torch: the parent commit's route to a view_gs (tools/mono_timing.py, leg one)."""
    view_gs = {}
    for ci, cam in enumerate(cams):
        near_far = torch.tensor(cam.near_far).float().to(device)
        image = torch.from_numpy(np.array(cam.image)).float().to(device) / 255.0
        H, W = image.shape[:2]
        mask = torch.tensor(cam.blendermask).float().to(device) if cam.blendermask is not None else torch.ones_like(image[..., 0])
        fx, fy = W / (2 * math.tan(cam.FovX / 2)), H / (2 * math.tan(cam.FovY / 2))
        intr = torch.tensor([[fx, 0, W / 2.0], [0, fy, H / 2.0], [0, 0, 1]]).float().to(device)
        w2c = torch.zeros((4, 4)).float().to(device)
        w2c[:3, :3] = torch.tensor(cam.R).float().to(device).transpose(0, 1)
        w2c[:3, 3] = torch.tensor(cam.T).float().to(device)
        w2c[3, 3] = 1.0
        infos = {}
        for cj, other in enumerate(cams):
            if cj == ci:
                continue
            mp = torch.tensor(match_data[cam.image_name][other.image_name]).type_as(image)
            uv = torch.stack([mp[:, 0] * W, mp[:, 1] * H], dim=-1)
            grid = (mp * 2 - 1)[None, None]
            color = torch.nn.functional.grid_sample(image.permute(2, 0, 1)[None], grid, mode="bilinear", align_corners=False)
            color = color.reshape(3, -1).permute(1, 0)
            bm = torch.nn.functional.grid_sample(mask[None, None], grid, mode="bilinear", align_corners=False).reshape(-1)
            homo = torch.cat([uv, torch.ones_like(uv[:, :1])], dim=-1).float()
            p = torch.matmul(intr.inverse()[None, :3, :3], homo[:, :, None])[..., 0]
            d = p / (torch.linalg.norm(p, ord=2, dim=-1, keepdim=True) + 1e-8)
            rays_d = torch.matmul(w2c.inverse()[None, :3, :3], d[:, :, None])[..., 0]
            rays_o = w2c.inverse()[None, :3, 3].expand(rays_d.shape)
            cam_rays_d = torch.matmul(w2c[None, :3, :3], rays_d[:, :, None])[..., 0]
            z = torch.rand(cam_rays_d.shape[0], 1).type_as(cam_rays_d) * (near_far[1] - near_far[0]) + near_far[0]
            infos[other.image_name] = {"z_val": torch.nn.Parameter(z.requires_grad_(True)), "rays_o": rays_o, "rays_d": rays_d,
                                       "cam_rays_d": cam_rays_d, "color": color, "uv": uv, "match_pixel": mp, "blender_mask": bm}
        view_gs[cam.image_name] = {"image_color": image, "intr": intr, "w2c": w2c, "height": H, "width": W, "match_infos": infos,
                                   "near_far": near_far}
    return view_gs

#!/usr/bin/env python3
"""Generate tests/golden/ref_init.npz and tests/golden/ref_init_edges.npz by RUNNING the reference's own Python for its ray-depth init stage (train.py:49-95):
GaussianModel.get_matchloss_from_base, training_setup_init, update_learning_rate_init, get_z_val and load_z_val of
scene/gaussian_model.py, imported read-only from /root/reference in the build container (stub finder and CPU device shim of
make_golden_model.py).  The loop around them is written here; only input/output arrays are committed.

Scene A: the three 96 x 64 cameras of make_golden_model.py (read back from ref_model.npz); the unordered pairs hold 1, 65 and 257
matches (different sizes, a wave boundary, a workgroup boundary); about 20 % of the matches are masked out; most depths start
11-14 units from where their match is met (more than 40 iterations at these learning rates can travel: their L1 terms keep
their signs), four start 1-3 units away and oscillate around it, a few start at 0.2-0.5 (they project outside the other view)
and a few at -15...-25 (Z < 0 in the other view).
Scene B: two views, one pair, mask0 * mask1 == 0 everywhere: no valid match.

ref_init_edges.npz (cameras built here, stored per view as <tag>_wh / <tag>_intr / <tag>_w2c in dictionary order; the inputs are
stored flat in arena order, <tag>_in_<name>, with <tag>_counts, because 42 segments of six arrays each would cost more in zip
headers than in data):
Scene C: three views of three sizes (96 x 64, 80 x 48, 64 x 96) and three intrinsics (fx != fy, off-centre principal points), in
the dictionary order view2, view0, view1; the unordered pairs hold 63, 64 and 2 matches; 12 iterations, learning rate halved
before iteration 6.  The reference normalises a pair by the size of its EARLIER view in dictionary order and projects with the
TARGET view's camera: with these views every swap changes the record.
Scene D: seven views, 21 unordered pairs = 42 segments of 1, 2, 3, 5, 1, ... matches, N = 112, one segment across element 64; 12
iterations.

Recorded in fp32 and in fp64 (the view_gs tensors cast to double): iteration 0 (scalar 5 * matchloss, loss_state, z_val.grad); a
40-iteration run with the learning rate halved before iterations 10, 20 and 30 (per-iteration scalars; z, best, min_loss at the
end and after 1 and 2 iterations); the depths after load_z_val(best).  Flat arrays follow the arena order: for a in keys, for b
in match_infos[a].

Asserted on the fp64 run, at EVERY iteration: no valid match has |px - u| or |py - v| below 1e-3 px, or |Z| below 1e-2 (the seed
is advanced until that holds).  Held on the fp32 run (the seed is advanced until it does): scalars, z, best and min_loss lie within
2e-5 * max(1, max|fp64|) of the fp64 run and the gradient within 1e-4 * max|g| — the floors of tests/test_gpu_init_stage.py — so
the reference alone passes every bar there.

A fixture whose arrays come out as the committed file holds them is left untouched (a zip member carries its time stamp).

Run:  python tests/golden/make_golden_init.py      (needs /root/reference; CPU only)
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_model as mgm                                                             # noqa: E402  (finder + shim)

REF = mgm.REF
OUT = os.path.join(HERE, "ref_init.npz")
OUT_EDGES = os.path.join(HERE, "ref_init_edges.npz")
W, H = 96, 64
ITERS, HALVE_AT = 40, (10, 20, 30)
MARGIN_PX, MARGIN_Z = 1e-3, 1e-2
FLOOR, GRAD_FLOOR = 2e-5, 1e-4
IN_KEYS = ("uv", "rays_o", "rays_d", "cam_rays_d", "blender_mask", "z_val")
VALUE_KEYS = ("losses", "final_z", "final_best", "final_min", "after1_z", "after1_best", "after1_min", "after2_z", "after2_best",
              "after2_min", "it0_loss", "it0_loss_state")


def rays_of(K, w2c, uv):
    """Rays of pixels uv (M,2) as create_from_mono forms them (scene/gaussian_model.py:330-336), in double."""
    c2w = torch.linalg.inv(w2c)
    p = (torch.linalg.inv(K) @ torch.cat([uv, torch.ones(uv.shape[0], 1, dtype=uv.dtype)], 1).t()).t()
    cam_rays = p / (torch.linalg.norm(p, dim=-1, keepdim=True) + 1e-8)
    return c2w[:3, 3][None].repeat(uv.shape[0], 1), (c2w[:3, :3] @ cam_rays.t()).t(), cam_rays


def project(K, w2c, pts):
    cam = (w2c[:3, :3] @ pts.t()).t() + w2c[:3, 3][None]
    xyz = (K @ cam.t()).t()
    return xyz[:, :2] / (xyz[:, 2:] + 1e-8), xyz[:, 2]


def make_view_gs(intr, w2c, pair_sizes, seed, no_valid=False, sizes=None, order=None):
    """A view_gs dictionary in double (cast later).  pair_sizes: {(i, j): M} over unordered view index pairs.  sizes: {i: (width,
    height)} (default: every view W x H); order: the view indices in dictionary order (default: ascending)."""
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64)                      # noqa: E731
    views = list(order) if order is not None else sorted({i for p in pair_sizes for i in p})
    assert sorted(views) == sorted({i for p in pair_sizes for i in p})
    names = {i: f"view{i}" for i in views}
    wh = {i: (sizes[i] if sizes is not None else (W, H)) for i in views}
    vg = {names[i]: {"width": wh[i][0], "height": wh[i][1], "intr": intr[i], "w2c": w2c[i], "match_infos": {}} for i in views}
    for (i, j), M in pair_sizes.items():
        uv_i = torch.stack([rnd(M) * (wh[i][0] - 16) + 8, rnd(M) * (wh[i][1] - 12) + 6], 1)
        o_i, d_i, cr_i = rays_of(intr[i], w2c[i], uv_i)
        depth = rnd(M) * 6 + 14
        t_i = depth / cr_i[:, 2]                                                           # distance along the ray of view i
        P = o_i + d_i * t_i[:, None]
        n = torch.stack([(rnd(M) * 0.15 + 0.05) * torch.sign(rnd(M) - 0.5), (rnd(M) * 2 + 2) * torch.sign(rnd(M) - 0.5)], 1)
        uv_j = project(intr[j], w2c[j], P)[0] + n
        o_j, d_j, cr_j = rays_of(intr[j], w2c[j], uv_j)
        t_j = torch.linalg.norm(P - o_j, dim=-1)

        def start(t):
            z = t + (rnd(M) * 3 + 11) * torch.sign(rnd(M) - 0.5)
            kind = rnd(M)
            if M > 100:                                                                    # two meet their match and oscillate
                z[5:7] = t[5:7] + (rnd(2) * 2 + 1) * torch.sign(rnd(2) - 0.5)
                kind[5:7] = 1.0
            z = torch.where((kind >= 0.02) & (kind < 0.08), rnd(M) * 0.3 + 0.2, z)         # projects outside the other view
            z = torch.where((kind >= 0.08) & (kind < 0.14), -(rnd(M) * 10 + 15), z)        # behind the other view
            return z
        if no_valid:
            m_i = (rnd(M) > 0.5).double()
            m_j = 1.0 - m_i
        else:
            m_i, m_j = (rnd(M) > 0.1).double(), (rnd(M) > 0.1).double()
            m_i[0] = m_j[0] = 1.0
        z_i, z_j = start(t_i), start(t_j)
        if M == 1:                                                                         # the single match is an ordinary one
            z_i, z_j = t_i + 12.0, t_j - 12.0
        vg[names[i]]["match_infos"][names[j]] = dict(uv=uv_i, rays_o=o_i, rays_d=d_i, cam_rays_d=cr_i, blender_mask=m_i,
                                                     z_val=z_i[:, None])
        vg[names[j]]["match_infos"][names[i]] = dict(uv=uv_j, rays_o=o_j, rays_d=d_j, cam_rays_d=cr_j, blender_mask=m_j,
                                                     z_val=z_j[:, None])
    return vg


def cast(vg, dtype):
    out = {}
    for a, v in vg.items():
        out[a] = {"width": v["width"], "height": v["height"], "intr": v["intr"].to(dtype), "w2c": v["w2c"].to(dtype),
                  "match_infos": {}}
        for b, mi in v["match_infos"].items():
            # the stored inputs are the fp32 values: the fp64 run starts from exactly those
            out[a]["match_infos"][b] = {k: t.float().to(dtype).clone() for k, t in mi.items()}
            out[a]["match_infos"][b]["z_val"] = torch.nn.Parameter(out[a]["match_infos"][b]["z_val"], requires_grad=True)
    return out


def arena(vg):
    return [(a, b) for a in vg for b in vg[a]["match_infos"]]


def flat(vg, nested, column=False):
    return torch.cat([nested[a][b].detach().reshape(-1) for a, b in arena(vg)]).numpy().copy()


def margins(vg):
    """Over the valid matches of every ordered pair, at the current depths: min |px - u|, |py - v| (pixels) and min |Z|."""
    keys = list(vg)
    m_px, m_z = float("inf"), float("inf")
    for a, b in arena(vg):
        mi, back = vg[a]["match_infos"][b], vg[b]["match_infos"][a]
        valid = (mi["blender_mask"] * back["blender_mask"]) > 0
        if not bool(valid.any()):
            continue
        pts = (mi["rays_o"] + mi["rays_d"] * mi["z_val"].detach()).double()
        xy, Z = project(vg[b]["intr"].double(), vg[b]["w2c"].double(), pts)
        d = (xy - back["uv"].double()).abs()[valid]
        m_px, m_z = min(m_px, float(d.min())), min(m_z, float(Z[valid].abs().min()))
    assert keys
    return m_px, m_z


def run_reference(GaussianModel, vg, iters, halve_at, check_margins):
    """The init stage of train.py:49-95 around the reference's methods.  Returns the recorded arrays."""
    gm = GaussianModel(3)
    gm.view_gs = vg
    gm.training_setup_init()
    rec, losses = {}, []
    best, min_loss = None, None
    worst_px, worst_z = float("inf"), float("inf")
    for it in range(iters):
        if it in halve_at:
            gm.update_learning_rate_init(0.5)
        if check_margins:
            m_px, m_z = margins(vg)
            worst_px, worst_z = min(worst_px, m_px), min(worst_z, m_z)
        matchloss, loss_state = gm.get_matchloss_from_base()
        loss = 5 * matchloss
        if best is None:
            best, min_loss = gm.get_z_val(), loss_state
        else:
            current = gm.get_z_val()
            for a in loss_state:
                for b in loss_state[a]:
                    keep = min_loss[a][b] < loss_state[a][b]
                    best[a][b] = torch.where(keep.unsqueeze(-1), best[a][b], current[a][b])
                    min_loss[a][b] = torch.where(keep, min_loss[a][b], loss_state[a][b])
        loss.backward()
        losses.append(float(loss.detach()))
        if it == 0:
            rec["it0_loss"] = np.array(float(loss.detach()))
            rec["it0_loss_state"] = flat(vg, loss_state)
            rec["it0_grad"] = flat(vg, {a: {b: vg[a]["match_infos"][b]["z_val"].grad for b in vg[a]["match_infos"]} for a in vg})
        with torch.no_grad():
            gm.optimizer_init.step()
            gm.optimizer_init.zero_grad(set_to_none=True)
        tag = {iters - 1: "final", 0: "after1", 1: "after2"}.get(it)
        if tag is not None:
            rec[tag + "_z"] = flat(vg, gm.get_z_val())
            rec[tag + "_best"] = flat(vg, best)
            rec[tag + "_min"] = flat(vg, min_loss)
    rec["losses"] = np.array(losses)
    gm.load_z_val(best)
    rec["loaded_z"] = flat(vg, gm.get_z_val())
    return rec, worst_px, worst_z


def pinhole(fx, fy, cx, cy):
    return torch.tensor([[fx, 0.0, cx], [0.0, fy, cy], [0.0, 0.0, 1.0]], dtype=torch.float64).float().double()


def look(ax, ay, centre):
    """w2c (4,4) of a camera at `centre` whose camera->world rotation is _rot(ax, ay); fp32-representable."""
    R = torch.from_numpy(mgm._rot(ax, ay))
    m = torch.eye(4, dtype=torch.float64)
    m[:3, :3] = R.t()
    m[:3, 3] = -(R.t() @ torch.tensor(centre, dtype=torch.float64))
    return m.float().double()


def within_floors(r32, r64, report):
    """The fp32 record against the fp64 one: every value within FLOOR * max(1, max|ref|), the gradient within GRAD_FLOOR * max|g|."""
    ok = True
    for k in VALUE_KEYS:
        a64, a32 = np.asarray(r64[k], dtype=np.float64), np.asarray(r32[k], dtype=np.float64)
        e32, floor = float(np.abs(a32 - a64).max()), FLOOR * max(1.0, float(np.abs(a64).max()))
        if report:
            print(f"  {k:16s} e32 {e32:.3e} floor {floor:.3e}")
        ok = ok and e32 <= floor
    g64 = r64["it0_grad"]
    eg = float(np.abs(r32["it0_grad"].astype(np.float64) - g64).max()) / float(np.abs(g64).max())
    if report:
        print(f"  it0_grad         e32 {eg:.3e} (of max|g|) floor {GRAD_FLOOR:.0e}")
    return ok and eg <= GRAD_FLOOR


def record_scene(GaussianModel, out, tag, sc, intr, w2c, flat_inputs):
    """Find the seed of scene `tag`, run the reference in fp64 and fp32 and put the arrays into `out`."""
    for seed in range(1000, 1400):
        base = make_view_gs(intr, w2c, sc["pair_sizes"], seed, sc["no_valid"], sc.get("sizes"), sc.get("order"))
        r64, m_px, m_z = run_reference(GaussianModel, cast(base, torch.float64), sc["iters"], sc["halve_at"], True)
        if sc["no_valid"]:
            break
        if not (m_px >= MARGIN_PX and m_z >= MARGIN_Z):
            print(f"scene {tag} seed {seed}: margin {m_px:.2e} px, |Z| {m_z:.2e}: next seed")
            continue
        r32, _, _ = run_reference(GaussianModel, cast(base, torch.float32), sc["iters"], sc["halve_at"], False)
        if within_floors(r32, r64, False):
            break
        print(f"scene {tag} seed {seed}: the fp32 record leaves the floors: next seed")
    else:
        raise SystemExit("no seed keeps every valid match away from the steps")
    r32, _, _ = run_reference(GaussianModel, cast(base, torch.float32), sc["iters"], sc["halve_at"], False)
    print(f"scene {tag}: seed {seed}, margin {m_px:.3e} px, min |Z| {m_z:.3e}")
    out[f"{tag}_seed"] = np.array(seed)
    names = list(base)
    out[f"{tag}_views"] = np.array([int(n[4:]) for n in names])
    out[f"{tag}_pairs"] = np.array([(int(a[4:]), int(b[4:])) for a, b in arena(base)])
    if flat_inputs:
        out[f"{tag}_iters"], out[f"{tag}_halve_at"] = np.array(sc["iters"]), np.array(sc["halve_at"], dtype=np.int64)
        out[f"{tag}_wh"] = np.array([(base[n]["width"], base[n]["height"]) for n in names])
        out[f"{tag}_intr"] = np.stack([base[n]["intr"].float().numpy() for n in names])
        out[f"{tag}_w2c"] = np.stack([base[n]["w2c"].float().numpy() for n in names])
        out[f"{tag}_counts"] = np.array([base[a]["match_infos"][b]["z_val"].shape[0] for a, b in arena(base)])
        for k in IN_KEYS:
            out[f"{tag}_in_{k}"] = np.concatenate([base[a]["match_infos"][b][k].float().numpy() for a, b in arena(base)])
    else:
        for a, b in arena(base):
            for k, t in base[a]["match_infos"][b].items():
                out[f"{tag}_in_{a[4:]}{b[4:]}_{k}"] = t.float().numpy()
    for k in r64:
        out[f"{tag}_f64_{k}"] = np.asarray(r64[k], dtype=np.float64)
        out[f"{tag}_f32_{k}"] = np.asarray(r32[k], dtype=np.float32)
    if sc["no_valid"]:
        assert np.isnan(r64["it0_loss"]) and np.isnan(r32["it0_loss"]) and not r64["it0_grad"].any() and not r32["it0_grad"].any()
        assert np.isfinite(r64["it0_loss_state"]).all()
        return
    assert within_floors(r32, r64, True)
    # the aliasing quirk of get_z_val(): after two iterations best is z after the first, min the smaller of L0 and L1
    assert np.array_equal(r64["after2_best"], r64["after1_z"]) and np.array_equal(r64["after1_best"], r64["after1_z"])


def same_arrays(path, out):
    if not os.path.exists(path):
        return False
    old = np.load(path)
    if sorted(old.files) != sorted(out):
        return False
    return all(old[k].dtype == np.asarray(v).dtype and old[k].shape == np.asarray(v).shape
               and old[k].tobytes() == np.ascontiguousarray(v).tobytes() for k, v in out.items())


def write(path, out):
    if same_arrays(path, out):
        print("unchanged", path, os.path.getsize(path), "bytes;", len(out), "arrays")
        return
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes;", len(out), "arrays")


def main():
    sys.meta_path.insert(0, mgm._Finder())
    mgm._cpu_device_shim()
    sys.path.insert(0, REF)
    from scene.gaussian_model import GaussianModel
    cams = np.load(os.path.join(HERE, "ref_model.npz"))
    intr = [torch.from_numpy(k).double() for k in cams["cam_intr"]]
    w2c = [torch.from_numpy(m).double() for m in cams["cam_w2c"]]
    out = {"wh": np.array([W, H]), "iters": np.array(ITERS), "halve_at": np.array(HALVE_AT)}
    scenes = {"A": dict(pair_sizes={(0, 1): 1, (0, 2): 65, (1, 2): 257}, iters=ITERS, halve_at=HALVE_AT, no_valid=False),
              "B": dict(pair_sizes={(0, 1): 33}, iters=3, halve_at=(), no_valid=True)}
    for tag, sc in scenes.items():
        record_scene(GaussianModel, out, tag, sc, intr, w2c, False)
    write(OUT, out)

    # ---- the edge scenes: their own cameras
    sizes3 = [(96, 64), (80, 48), (64, 96)]
    intr_c = [pinhole(110.0, 105.0, 47.5, 31.0), pinhole(90.0, 95.0, 41.0, 23.5), pinhole(120.0, 125.0, 30.5, 49.0)]
    scene_c = dict(pair_sizes={(2, 0): 63, (2, 1): 64, (0, 1): 2}, iters=12, halve_at=(6,), no_valid=False,
                   sizes={i: sizes3[i] for i in range(3)}, order=[2, 0, 1])
    nv = 7
    sizes_d = {i: sizes3[i % 3] for i in range(nv)}
    intr_d = [pinhole(100.0 + 7 * i, 104.0 + 5 * i, sizes_d[i][0] / 2 - 1 + 0.5 * i, sizes_d[i][1] / 2 + 1 - 0.5 * i) for i in range(nv)]
    w2c_d = [look(0.03 * (i - 3) * (-1) ** i, 0.05 * (i - 3), (0.4 * (i - 3), 0.1 * ((3 * i) % 4 - 1.5), 0.05 * i)) for i in range(nv)]
    pairs_d = [(i, j) for i in range(nv) for j in range(i + 1, nv)]
    scene_d = dict(pair_sizes={p: (1, 2, 3, 5)[n % 4] for n, p in enumerate(pairs_d)}, iters=12, halve_at=(), no_valid=False,
                   sizes=sizes_d, order=[3, 0, 5, 1, 6, 2, 4])
    edges = {}
    record_scene(GaussianModel, edges, "C", scene_c, intr_c, w2c, True)
    record_scene(GaussianModel, edges, "D", scene_d, intr_d, w2c_d, True)
    assert list(edges["C_views"]) == [2, 0, 1] and sorted(edges["C_counts"]) == [2, 2, 63, 63, 64, 64]
    counts, n_d = edges["D_counts"], int(edges["D_counts"].sum())
    offs = np.concatenate([[0], np.cumsum(counts)[:-1]])
    assert len(counts) == 42 and 64 < n_d < 128 and set(counts) == {1, 2, 3, 5}
    assert bool(((offs < 64) & (offs + counts > 64)).any()), "no segment of scene D lies across element 64"
    print(f"scene D: N = {n_d}, segment offsets around 64: {[(int(o), int(c)) for o, c in zip(offs, counts) if o <= 64 < o + c]}")
    write(OUT_EDGES, edges)


if __name__ == "__main__":
    main()

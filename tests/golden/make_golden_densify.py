#!/usr/bin/env python3
"""Generate tests/golden/ref_densify.npz by RUNNING the reference's own GaussianModel.training_setup, one Adam step of both
optimizers, densify_and_prune and reset_opacity (scene/gaussian_model.py:486-515, 644-651, 758-930) on the CPU.  Only arrays are
committed; no reference source travels.  The reference is imported exactly as make_golden_model.py imports it (stub finder for the
import-time-only packages, `device="cuda"` redirected to the CPU).

torch.normal is patched for the duration of the call so that the split's samples are std * U[copy, selected row] for a recorded
U of shape (2, P, 3): on the CPU torch.normal(0, std) IS randn * std, so this is the reference's arithmetic with known samples.

Cases (about 96 + 64 Gaussians, moments non-zero after one Adam step):
  mss20    densify_and_prune(max_grad, min_opacity, extent, 20)
  mssnone  the same inputs, max_screen_size None
  nobg     no background Gaussians before the call
  reset    reset_opacity() on the result of mss20
Planted: two rows whose accum / denom equals max_grad bit for bit (both must be selected), one row 0 / 0 (NaN -> 0), one row x / 0
(inf: selected), rows only the world-size term removes, rows below min_opacity in either set, max_radii2D huge everywhere.
Asserted: no row within 1e-5 relative of a threshold behind a transcendental (an exp one ulp apart must not flip a row).

Run:  python tests/golden/make_golden_densify.py      (needs the reference tree; CPU only)
"""
import os
import sys
from argparse import ArgumentParser

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_model as mgm                                                             # noqa: E402

OUT = os.path.join(HERE, "ref_densify.npz")
NR, NB = 96, 64
MAX_GRAD, MIN_OPACITY, EXTENT = 0.0004, 0.005, 5.0
RAY = (("_zval", "zval"), ("_features_dc", "f_dc"), ("_features_rest", "f_rest"), ("_opacity", "opacity"), ("_scaling", "scaling"),
       ("_rotation", "rotation"))
BG = (("bg_xyz", "bg_xyz"), ("bg_features_dc", "bg_f_dc"), ("bg_features_rest", "bg_f_rest"), ("bg_opacity", "bg_opacity"),
      ("bg_scaling", "bg_scaling"), ("bg_rotation", "bg_rotation"))
LIVE_COLUMNS = 6                     # features_rest, its gradient and so its moments are zero beyond (keeps the file small)


def coarse(t):
    """Values with a short mantissa (exactly representable in fp16): the file compresses, copies stay bit-exact copies."""
    return t.to(torch.float16).to(torch.float32)


def inputs(g, nb):
    r = lambda *s: torch.randn(*s, generator=g)                                             # noqa: E731
    P = NR + nb

    def one_set(n, spread):
        rest = torch.zeros(n, 45)
        rest[:, :LIVE_COLUMNS] = r(n, LIVE_COLUMNS) * 0.15
        return dict(features_dc=coarse(torch.rand(n, 1, 3, generator=g) * 3 - 1.5), features_rest=coarse(rest).reshape(n, 15, 3),
                    opacity=coarse(r(n, 1) * 2), scaling=coarse(r(n, 3) * 0.6 - spread), rotation=coarse(r(n, 4)))
    ray, bg = one_set(NR, 3.0), one_set(nb, 2.8)
    d = coarse(r(NR, 3))
    ray.update(zval=coarse(torch.rand(NR, 1, generator=g) * 6 + 3), rayo=coarse(r(NR, 3) * 0.1),
               rayd=d / d.norm(dim=1, keepdim=True))
    bg.update(xyz=coarse(r(nb, 3) * 3))
    # planted rows: large (only the world-size term can remove them; their children are / are not small enough), transparent
    if nb:
        bg["scaling"][3] = torch.tensor([0.3, -1.0, -2.0])          # s = 1.35 > 1: child 0.84 survives
        bg["scaling"][4] = torch.tensor([0.7, 0.1, -2.0])           # s = 2.01: child 1.26 goes too
        bg["scaling"][5] = torch.tensor([0.25, -1.0, -1.5])
        bg["scaling"][6] = torch.tensor([0.75, 0.0, -1.5])
        bg["opacity"][7:11] = torch.tensor([[-6.0], [-7.0], [-6.5], [-8.0]])
    ray["scaling"][3] = torch.tensor([0.3, -1.0, -2.0])
    ray["scaling"][4] = torch.tensor([0.7, 0.1, -2.0])
    ray["opacity"][7:11] = torch.tensor([[-6.0], [-7.0], [-6.5], [-8.0]])
    denom = torch.randint(1, 6, (P, 1), generator=g).float()
    accum = denom * torch.rand(P, 1, generator=g) * 0.0008
    hot = torch.tensor([3, 4, 7, 8] + ([NR + 3, NR + 4, NR + 7, NR + 8] if nb else []))      # planted rows: half hot, half not
    cold = torch.tensor([9, 10] + ([NR + 5, NR + 6, NR + 9, NR + 10] if nb else []))
    accum[hot] = denom[hot] * 0.0007
    accum[cold] = denom[cold] * 0.0001
    tie = torch.tensor(MAX_GRAD, dtype=torch.float32)
    for row in (20, NR + 20 if nb else 21):                                                   # accum / denom == max_grad exactly
        denom[row], accum[row] = 2.0, tie * 2
    denom[30], accum[30] = 0.0, 0.0                                                           # NaN -> 0
    denom[31], accum[31] = 0.0, 0.003                                                         # inf stays
    stats = dict(xyz_gradient_accum=accum, denom=denom, max_radii2D=torch.rand(P, generator=g) * 500 + 100)
    return ray, bg, stats


def snapshot(gm, out, tag):
    for a, n in RAY + BG:
        p = getattr(gm, a)
        out[f"{tag}_{a}"] = p.detach().numpy().copy()
        opt = gm.optimizer if (a, n) in RAY else gm.optimizer_bg
        grp = next(x for x in opt.param_groups if x["name"] == n)
        assert grp["params"][0] is p, (tag, a)
        st = opt.state.get(p)
        if st:
            out[f"{tag}_step_{n}"] = np.float32(float(st["step"]))
            out[f"{tag}_m_{n}"] = st["exp_avg"].numpy().copy()
            out[f"{tag}_v_{n}"] = st["exp_avg_sq"].numpy().copy()
    for a in ("_rayo", "_rayd", "xyz_gradient_accum", "denom", "max_radii2D"):
        out[f"{tag}_{a}"] = getattr(gm, a).detach().numpy().copy()


def main():
    sys.meta_path.insert(0, mgm._Finder())
    mgm._cpu_device_shim()
    sys.path.insert(0, mgm.REF)
    from scene.gaussian_model import GaussianModel
    from arguments import OptimizationParams
    opt_args = OptimizationParams(ArgumentParser())
    real_normal = torch.normal
    out = {"percent_dense": np.float32(opt_args.percent_dense)}

    def model(seed, nb):
        g = torch.Generator().manual_seed(seed)
        ray, bg, stats = inputs(g, nb)
        gm = GaussianModel(3)
        gm.spatial_lr_scale = 1.0
        for k, v in ray.items():
            setattr(gm, "_" + k, torch.nn.Parameter(v.clone()) if k not in ("rayo", "rayd") else v.clone())
        for k, v in bg.items():
            setattr(gm, "bg_" + k, torch.nn.Parameter(v.clone() if nb else torch.empty(0)))
        gm.training_setup(opt_args)
        gm.max_radii2D = stats["max_radii2D"]
        # one Adam step of both optimizers: moments non-zero, features_rest live in its first columns only
        for a, _n in RAY + (BG if nb else ()):
            p = getattr(gm, a)
            grad = torch.randn(p.shape, generator=g) * 1e-3
            if a.endswith("features_rest"):
                grad.reshape(p.shape[0], 45)[:, LIVE_COLUMNS:] = 0
            p.grad = grad
        gm.optimizer.step()
        gm.optimizer_bg.step()
        for a, _n in RAY + BG:
            getattr(gm, a).grad = None
        gm.xyz_gradient_accum, gm.denom = stats["xyz_gradient_accum"], stats["denom"]
        return gm, torch.randn(2, NR + nb, 3, generator=g)

    def knife_edges(gm, mss):
        with torch.no_grad():
            s = gm.get_scaling.max(dim=1).values
            child = torch.exp(torch.log(gm.get_scaling / 1.6)).max(dim=1).values
            o = gm.get_opacity[:, 0]
            rel = lambda x, t: ((x - t).abs() / t).min().item()                            # noqa: E731
            edges = {"s vs dense": rel(s, opt_args.percent_dense * EXTENT), "o vs min_opacity": rel(o, MIN_OPACITY),
                     "s vs big": rel(s, 0.2 * EXTENT), "child vs big": rel(child, 0.2 * EXTENT)}
        assert all(v > 1e-5 for v in edges.values()), edges
        return edges

    def run(tag, seed, nb, mss):
        gm, U = model(seed, nb)
        print(tag, "closest relative distance to a threshold:", knife_edges(gm, mss))
        snapshot(gm, out, f"{tag}_in")
        out[f"{tag}_noise"] = U.numpy()
        out[f"{tag}_args"] = np.array([MAX_GRAD, MIN_OPACITY, EXTENT, np.nan if mss is None else mss], dtype=np.float64)
        P = NR + nb
        g = (gm.xyz_gradient_accum / gm.denom)[:, 0]
        assert int((g == torch.tensor(MAX_GRAD, dtype=torch.float32)).sum()) == 2 and int(g.isnan().sum()) == 1

        def normal(mean, std):
            # the rows the reference selected, recovered from the activated scales it passes as std (N = 2 copies of them)
            n = std.shape[0] // 2
            act = gm.get_scaling.detach()[:P]
            rows = [int((act == std[k]).all(dim=1).nonzero()[0, 0]) for k in range(n)]
            assert torch.equal(act[rows], std[:n]) and torch.equal(std[:n], std[n:]) and float(mean.abs().max()) == 0
            assert len(set(rows)) == n
            return std * torch.cat([U[0, rows], U[1, rows]])
        torch.normal = normal
        try:
            gm.densify_and_prune(MAX_GRAD, MIN_OPACITY, EXTENT, mss)
        finally:
            torch.normal = real_normal
        snapshot(gm, out, f"{tag}_out")
        print(tag, "background rows", nb, "->", gm.bg_xyz.shape[0])
        return gm

    gm = run("mss20", 11, NB, 20)
    gm.reset_opacity()
    snapshot(gm, out, "reset_out")
    out["reset_in_is"] = np.array("mss20_out")
    gm2 = run("mssnone", 11, NB, None)
    for k in [k for k in out if k.startswith("mssnone_in_")]:                                 # the same inputs, stored once
        assert np.array_equal(out[k], out[k.replace("mssnone_in_", "mss20_in_")], equal_nan=True)
        del out[k]
    out["mssnone_in_is"] = np.array("mss20_in")
    assert gm2.bg_xyz.shape[0] > out["mss20_out_bg_xyz"].shape[0], "the world-size term removed nothing"
    run("nobg", 12, 0, 20)
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes;", len(out), "arrays")


if __name__ == "__main__":
    main()

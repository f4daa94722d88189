"""The reference's densify_and_prune and reset_opacity as plain torch, a stand-in model class with the reference model's attribute
names, and the cases of tests/golden/ref_densify.npz.

`densify_and_prune` restates GaussianModel.densify_and_prune (scene/gaussian_model.py:758-930) and `reset_opacity` :644-651 in this
project's words, taking the split's unit normal samples explicitly (noise[copy, source]); tests/test_densify_cpu.py holds both to the
arrays the reference's own code produced.  tools/densify_timing.py times the restatement as the torch leg.

Below the restatement: the header's rule in fp64 (`densify_truth`, `reset_truth`), the margins of its decisions (`near_threshold`), a
NaN- and inf-aware row comparison (`compare_rows`), a bitwise check of everything that is copied (`assert_copied`) and the pattern
scenes of tests/test_gpu_densify_edges.py; tests/test_densify_edges_cpu.py holds the scenes to what they claim."""
from __future__ import annotations

import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# (attribute, group name, row shape, learning rate) of the two optimizers (scene/gaussian_model.py:491-509, arguments/__init__.py)
RAY = (("_zval", "zval", (1,), 1.6e-4), ("_features_dc", "f_dc", (1, 3), 2e-3), ("_features_rest", "f_rest", (15, 3), 1e-4),
       ("_opacity", "opacity", (1,), 5.5e-2), ("_scaling", "scaling", (3,), 5.5e-3), ("_rotation", "rotation", (4,), 1.5e-3))
BG = (("bg_xyz", "bg_xyz", (3,), 1.6e-4), ("bg_features_dc", "bg_f_dc", (1, 3), 2e-3), ("bg_features_rest", "bg_f_rest", (15, 3), 1e-4),
      ("bg_opacity", "bg_opacity", (1,), 5.5e-2), ("bg_scaling", "bg_scaling", (3,), 5.5e-3), ("bg_rotation", "bg_rotation", (4,), 1.5e-3))
FIXED = (("_rayo", (3,)), ("_rayd", (3,)))
STATS = (("xyz_gradient_accum", (1,)), ("denom", (1,)), ("max_radii2D", ()))
CASES = ("mss20", "mssnone", "nobg")              # densify_and_prune cases of the fixture; "reset" follows "mss20"


def fixture():
    return np.load(os.path.join(GOLDEN, "ref_densify.npz"))


class StandIn:
    """What densify / optim need of the reference's GaussianModel: its attribute names, percent_dense and the two optimizers."""

    def __init__(self, tensors, percent_dense=0.01, optimizer_cls=torch.optim.Adam, device="cpu"):
        """tensors: {attribute: array or tensor} for the 14 model tensors and the three statistics tensors."""
        dev = torch.device(device)
        t = lambda a: torch.as_tensor(np.asarray(a) if not torch.is_tensor(a) else a).detach().to(torch.float32).to(dev).clone()   # noqa: E731
        for a, _n, tail, _lr in RAY + BG:
            x = t(tensors[a])
            setattr(self, a, torch.nn.Parameter(x.reshape((x.shape[0],) + tail).contiguous()))
        for a, tail in FIXED + STATS:
            x = t(tensors[a])
            setattr(self, a, x.reshape((x.shape[0],) + tail).contiguous())
        self.percent_dense = percent_dense
        self.optimizer = optimizer_cls([{"params": [getattr(self, a)], "lr": lr, "name": n} for a, n, _t, lr in RAY], lr=0.0, eps=1e-15)
        self.optimizer_bg = optimizer_cls([{"params": [getattr(self, a)], "lr": lr, "name": n} for a, n, _t, lr in BG], lr=0.0,
                                          eps=1e-15)

    def set_state(self, name, step, exp_avg, exp_avg_sq):
        """Give the group called `name` the optimizer state (step, exp_avg, exp_avg_sq)."""
        for opt in (self.optimizer, self.optimizer_bg):
            for g in opt.param_groups:
                if g["name"] == name:
                    p = g["params"][0]
                    on_device = bool(opt.defaults.get("capturable")) and p.is_cuda
                    conv = lambda a: torch.as_tensor(np.asarray(a) if not torch.is_tensor(a) else a).detach().to(torch.float32) \
                        .to(p.device).reshape(p.shape).clone()                                                # noqa: E731
                    opt.state[p] = {"step": torch.tensor(float(step), dtype=torch.float32, device=p.device if on_device else "cpu"),
                                    "exp_avg": conv(exp_avg), "exp_avg_sq": conv(exp_avg_sq)}
                    return
        raise KeyError(name)

    def group_state(self, name):
        for opt in (self.optimizer, self.optimizer_bg):
            for g in opt.param_groups:
                if g["name"] == name:
                    return opt.state.get(g["params"][0]) or None
        raise KeyError(name)

    @property
    def P(self):
        return self._zval.shape[0] + self.bg_xyz.shape[0]


def load_case(fx, tag: str, side: str = "in", device="cpu", optimizer_cls=torch.optim.Adam) -> StandIn:
    """The model of case `tag` before ("in") or after ("out") the reference's call, optimizer state included."""
    src = f"{tag}_{side}"
    while f"{src}_is" in fx.files:                 # a snapshot recorded once under another name
        src = str(fx[f"{src}_is"])
    tensors = {a: fx[f"{src}_{a}"] for a in [r[0] for r in RAY + BG] + [f[0] for f in FIXED + STATS]}
    m = StandIn(tensors, float(fx["percent_dense"]), optimizer_cls, device)
    for _a, n, _t, _lr in RAY + BG:
        if f"{src}_step_{n}" in fx.files:
            m.set_state(n, float(fx[f"{src}_step_{n}"]), fx[f"{src}_m_{n}"], fx[f"{src}_v_{n}"])
    return m


def case_args(fx, tag: str):
    """(max_grad, min_opacity, extent, max_screen_size) of a densify case, as Python numbers / None."""
    max_grad, min_opacity, extent, mss = (float(x) for x in fx[f"{tag}_args"])
    return max_grad, min_opacity, extent, (None if np.isnan(mss) else mss)


def origins(before: StandIn, after: StandIn) -> torch.Tensor:
    """For every background row of `after` the source index in `before` it came from: features_dc is copied bit for bit on every
    path (kept original, clone, child) and the test models make its rows unique."""
    src = torch.cat([before._features_dc.detach(), before.bg_features_dc.detach()]).cpu().reshape(-1, 3).numpy()
    table = {row.tobytes(): i for i, row in enumerate(src)}
    assert len(table) == src.shape[0], "features_dc rows are not unique"
    out = after.bg_features_dc.detach().cpu().reshape(-1, 3).numpy()
    return torch.tensor([table.get(row.tobytes(), -1) for row in out], dtype=torch.int64)


# ---------------------------------------------------------------------------------------------------------------------------------
def _both(ray, bg):
    return torch.cat([ray, bg]) if bg.shape[0] else ray


def rotation_matrices(q):
    """build_rotation (utils/general_utils.py:84-105): normalises q = (r, x, y, z) itself."""
    norm = torch.sqrt(q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1] + q[:, 2] * q[:, 2] + q[:, 3] * q[:, 3])
    q = q / norm[:, None]
    r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    return torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
                        2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
                        2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], dim=1).reshape(-1, 3, 3)


def _rekey(opt, group, tensor, exp_avg=None, exp_avg_sq=None):
    """A new Parameter in `group`, the state entry moved to it with the given moments (when there is state)."""
    old = group["params"][0]
    st = opt.state.get(old) or None
    new = torch.nn.Parameter(tensor.requires_grad_(True))
    if old in opt.state:
        del opt.state[old]
    group["params"][0] = new
    if st is not None:
        st["exp_avg"], st["exp_avg_sq"] = exp_avg, exp_avg_sq
        opt.state[new] = st
    return new


@torch.no_grad()
def densify_and_prune(g: StandIn, max_grad, min_opacity, extent, max_screen_size, noise):
    """Returns {"origin": source index of every new background row, "sections": (originals, clones, children per copy)}."""
    nr = g._zval.shape[0]
    dev = g._zval.device
    grad = g.xyz_gradient_accum / g.denom
    grad[grad.isnan()] = 0.0
    grad = grad[:, 0]
    P = grad.shape[0]
    raw = {a: _both(getattr(g, r).detach(), getattr(g, b).detach())
           for a, r, b in (("dc", "_features_dc", "bg_features_dc"), ("rest", "_features_rest", "bg_features_rest"),
                           ("opacity", "_opacity", "bg_opacity"), ("scaling", "_scaling", "bg_scaling"),
                           ("rotation", "_rotation", "bg_rotation"))}
    xyz = _both(g._rayo + g._rayd * g._zval.detach(), g.bg_xyz.detach())
    size = torch.exp(raw["scaling"]).max(dim=1).values
    opac = torch.sigmoid(raw["opacity"])[:, 0]
    shrink = torch.full((), 1.6, dtype=torch.float32, device=dev)          # a tensor: a true fp32 division on every device

    def gone(o, s):
        m = o < min_opacity
        return m | (s > 0.2 * extent) if max_screen_size else m

    dense = g.percent_dense * extent
    clone = (grad.abs() >= max_grad) & (size <= dense)
    split = (grad >= max_grad) & (size > dense)
    is_bg = torch.arange(P, device=dev) >= nr
    keep = (is_bg & ~split & ~gone(opac, size)).nonzero()[:, 0]
    clones = (clone & ~gone(opac, size)).nonzero()[:, 0]
    cand = split.nonzero()[:, 0]
    activated = torch.exp(raw["scaling"][cand])
    child_scaling = torch.log(activated / shrink)
    ok = ~gone(opac[cand], torch.exp(child_scaling).max(dim=1).values)
    parents, activated, child_scaling = cand[ok], activated[ok], child_scaling[ok]
    R = rotation_matrices(raw["rotation"][parents])
    child_xyz = [torch.bmm(R, (activated * noise[c, parents]).unsqueeze(-1)).squeeze(-1) + xyz[parents] for c in (0, 1)]

    origin = torch.cat([keep, clones, parents, parents])
    new = {"bg_xyz": torch.cat([xyz[keep], xyz[clones]] + child_xyz),
           "bg_features_dc": raw["dc"][origin], "bg_features_rest": raw["rest"][origin], "bg_opacity": raw["opacity"][origin],
           "bg_scaling": torch.cat([raw["scaling"][keep], raw["scaling"][clones], child_scaling, child_scaling]),
           "bg_rotation": raw["rotation"][origin]}
    fresh = origin.shape[0] - keep.shape[0]
    for a, n, tail, _lr in BG:
        grp = next(x for x in g.optimizer_bg.param_groups if x["name"] == n)
        st = g.optimizer_bg.state.get(grp["params"][0]) or None
        m = v = None
        if st is not None:
            pad = torch.zeros((fresh,) + tail, dtype=torch.float32, device=dev)
            m = torch.cat([st["exp_avg"][keep - nr], pad])
            v = torch.cat([st["exp_avg_sq"][keep - nr], pad])
        setattr(g, a, _rekey(g.optimizer_bg, grp, new[a].contiguous(), m, v))
    # a split ray-bound Gaussian stays; its raw log-scale row is divided
    scaling = g._scaling.detach().clone()
    hit = split[:nr]
    scaling[hit] = scaling[hit] / shrink
    grp = next(x for x in g.optimizer.param_groups if x["name"] == "scaling")
    g._scaling = _rekey(g.optimizer, grp, scaling, torch.zeros_like(scaling), torch.zeros_like(scaling))
    rows = nr + origin.shape[0]
    g.xyz_gradient_accum = torch.zeros((rows, 1), device=dev)
    g.denom = torch.zeros((rows, 1), device=dev)
    g.max_radii2D = torch.zeros((rows,), device=dev)
    return {"origin": origin, "sections": (keep.shape[0], clones.shape[0], parents.shape[0])}


@torch.no_grad()
def reset_opacity(g: StandIn):
    for opt, attr, name in ((g.optimizer, "_opacity", "opacity"), (g.optimizer_bg, "bg_opacity", "bg_opacity")):
        x = getattr(g, attr).detach()
        if x.shape[0] == 0:
            continue
        o = torch.min(torch.sigmoid(x), torch.ones_like(x) * 0.01)
        new = torch.log(o / (1 - o))
        grp = next(q for q in opt.param_groups if q["name"] == name)
        setattr(g, attr, _rekey(opt, grp, new, torch.zeros_like(new), torch.zeros_like(new)))


# ---------------------------------------------------------------------------------------------------------------------------------
def assert_same_model(got: StandIn, want: StandIn, before: StandIn, what: str, reset: bool = False):
    """`got` against `want` (both results of one call on `before`): integer structure identical, everything that is a copy or a
    single IEEE operation torch.equal, what goes through exp / log / a rotation (child xyz, child scaling, reset opacities) through
    parity_utils.assert_close."""
    from parity_utils import assert_close
    cpu = lambda t: t.detach().cpu()                                                          # noqa: E731
    nr = want._zval.shape[0]
    assert got._zval.shape[0] == nr and got.bg_xyz.shape[0] == want.bg_xyz.shape[0], \
        (what, "rows", got._zval.shape[0], got.bg_xyz.shape[0], "expected", nr, want.bg_xyz.shape[0])
    if not reset:
        origin = origins(before, want)
        assert (origin >= 0).all() and torch.equal(origins(before, got), origin), (what, "source of the new rows")
        src_scaling = torch.cat([cpu(before._scaling), cpu(before.bg_scaling)])[origin]
        child = (cpu(want.bg_scaling) != src_scaling).any(dim=1)
    else:
        child = torch.zeros(want.bg_xyz.shape[0], dtype=torch.bool)
    computed = {"bg_xyz": child, "bg_scaling": child}
    for a, n, _tail, _lr in RAY + BG:
        g, w = cpu(getattr(got, a)), cpu(getattr(want, a))
        assert g.shape == w.shape, (what, a, g.shape, w.shape)
        if reset and a in ("_opacity", "bg_opacity"):
            if w.numel():
                assert_close(g, w, f"{what} {a}")
        elif a in computed and bool(computed[a].any()):
            rows = computed[a]
            assert torch.equal(g[~rows], w[~rows]), (what, a, "copied rows")
            assert_close(g[rows], w[rows], f"{what} {a} of the children")
        else:
            assert torch.equal(g, w), (what, a)
        sg, sw = got.group_state(n), want.group_state(n)
        assert (sg is None) == (sw is None), (what, n, "optimizer state present")
        if sw is not None:
            assert float(sg["step"]) == float(sw["step"]), (what, n, "step")
            for k in ("exp_avg", "exp_avg_sq"):
                assert sg[k].shape == getattr(got, a).shape, (what, n, k, sg[k].shape)
                assert torch.equal(cpu(sg[k]), cpu(sw[k])), (what, n, k)
    for a, _tail in FIXED + STATS:
        g, w = cpu(getattr(got, a)), cpu(getattr(want, a))
        assert g.shape == w.shape and torch.equal(g, w), (what, a, g.shape, w.shape)


# ---- the header's rule in fp64, the margins of its decisions and a NaN- / inf-aware comparison ----------------------------------
# (tests/test_densify_edges_cpu.py holds the conditions on the inputs, tests/test_gpu_densify_edges.py the kernels to these)
MARGIN, NEAR, NEAR_CPU = 4.0, 16.0, 64.0          # the factor on e_ref of the float bar; the near-threshold margin on the GPU / here
SHRINK = 1.6
F32_TINY = float(np.finfo(np.float32).tiny)


def prev32(x):
    return np.nextafter(np.float32(x), np.float32(-np.inf))


def next32(x):
    return np.nextafter(np.float32(x), np.float32(np.inf))


def _t32(a, tail):
    a = a.detach().cpu() if torch.is_tensor(a) else torch.as_tensor(np.asarray(a))
    a = a.to(torch.float32)
    return a.reshape((a.shape[0],) + tail)


def _quantities(t, max_grad, min_opacity, dense_scale, big_scale, noise, dtype):
    """Every quantity of the rule for every source, the expressions of densify_and_prune above evaluated in `dtype` on the fp32
    inputs (torch.float32: the restatement's own arithmetic; torch.float64: the truth).  The thresholds are fp32 values."""
    c = lambda a, tail: _t32(t[a], tail).to(dtype)                                            # noqa: E731
    nr = _t32(t["_zval"], (1,)).shape[0]
    thr = {k: torch.tensor(float(np.float32(v)), dtype=dtype) for k, v in
           (("max_grad", max_grad), ("min_opacity", min_opacity), ("dense_scale", dense_scale))}
    use_big = big_scale is not None and float(big_scale) >= 0.0
    big = torch.tensor(float(np.float32(big_scale)) if use_big else float("inf"), dtype=dtype)
    g = (c("xyz_gradient_accum", (1,)) / c("denom", (1,)))[:, 0]
    g = torch.where(g.isnan(), torch.zeros_like(g), g)
    scaling = _both(c("_scaling", (3,)), c("bg_scaling", (3,)))
    opacity = _both(c("_opacity", (1,)), c("bg_opacity", (1,)))[:, 0]
    rotation = _both(c("_rotation", (4,)), c("bg_rotation", (4,)))
    xyz = _both(c("_rayo", (3,)) + c("_rayd", (3,)) * c("_zval", (1,)), c("bg_xyz", (3,)))
    e = torch.exp(scaling)
    smax = e.max(dim=1).values                                            # torch.max over a dimension: a NaN wins
    o = torch.sigmoid(opacity)
    shrink = torch.tensor(SHRINK, dtype=torch.float32).to(dtype) if dtype == torch.float32 else torch.tensor(SHRINK, dtype=dtype)
    child_scaling = torch.log(e / shrink)
    child_smax = torch.exp(child_scaling).max(dim=1).values
    clone = (g.abs() >= thr["max_grad"]) & (smax <= thr["dense_scale"])
    split = (g >= thr["max_grad"]) & (smax > thr["dense_scale"])
    gone = (o < thr["min_opacity"]) | (smax > big)
    child_gone = (o < thr["min_opacity"]) | (child_smax > big)
    u = _t32(noise, (noise.shape[1], 3)).to(dtype)                        # (2, P, 3)
    R = rotation_matrices(rotation)
    arm = e[None] * u                                                     # exp(scaling) * noise[c]
    child_xyz = torch.stack([torch.bmm(R, arm[k].unsqueeze(-1)).squeeze(-1) + xyz for k in (0, 1)])
    ray_scaling = scaling[:nr] / shrink
    return {"nr": nr, "g": g, "smax": smax, "o": o, "child_smax": child_smax, "clone": clone, "split": split, "gone": gone,
            "child_gone": child_gone, "xyz": xyz, "scaling": scaling, "child_xyz": child_xyz, "child_scaling": child_scaling,
            "arm": arm, "ray_scaling": ray_scaling, "thr": dict(thr, big_scale=big), "use_big": use_big}


def _sections(q):
    """(keep, clones, parents): the source indices of the three sections from the four decisions."""
    P = q["g"].shape[0]
    is_bg = torch.arange(P) >= q["nr"]
    return ((is_bg & ~q["split"] & ~q["gone"]).nonzero()[:, 0], (q["clone"] & ~q["gone"]).nonzero()[:, 0],
            (q["split"] & ~q["child_gone"]).nonzero()[:, 0])


@torch.no_grad()
def densify_truth(tensors, max_grad, min_opacity, dense_scale, big_scale, noise):
    """The header's rule (include/scg_raster.h, "Densify-and-prune and the opacity reset") in fp64 on the fp32 inputs; the
    thresholds are the fp32 values the binding passes (big_scale None or < 0: no world-size term).  numpy arrays per source:
      g, smax, o, child_smax            the decision quantities (fp64)
      clone, split, gone, child_gone    the four decisions: the two selections, the prune of the original and its clone, the
                                        prune of the children
      margin                            {name: quantity - threshold} for g_split (g - max_grad), g_clone (|g| - max_grad),
                                        dense (smax - dense_scale), big / child_big (smax, child smax - big_scale; absent without the
                                        world-size term), opacity (o - min_opacity)
      e_ref                             {g, smax, child_smax, o}: |fp32 restatement - fp64| of each quantity on this input, as near_threshold
                                        uses it (see there)
      keep, clones, parents, origin     the sections' source indices and their concatenation (keep, clones, parents, parents)
      child_xyz (2, P, 3), child_scaling (P, 3), ray_scaling (nr, 3)   what a split computes, for EVERY source (rows of other
                                        sources are not meaningful), child_term (2, P) and scaling_term (P,): the largest term of the row
    and under "ref32" the same dictionary's arrays from the fp32 run (the restatement's arithmetic), "agree": whether the two runs
    take the same four decisions everywhere."""
    noise = torch.as_tensor(np.asarray(noise) if not torch.is_tensor(noise) else noise.detach().cpu())
    q64 = _quantities(tensors, max_grad, min_opacity, dense_scale, big_scale, noise, torch.float64)
    q32 = _quantities(tensors, max_grad, min_opacity, dense_scale, big_scale, noise, torch.float32)

    def pack(q):
        keep, clones, parents = _sections(q)
        out = {k: q[k].numpy() for k in ("g", "smax", "o", "child_smax", "clone", "split", "gone", "child_gone", "child_xyz",
                                          "child_scaling", "ray_scaling", "xyz", "scaling")}
        out.update(keep=keep.numpy(), clones=clones.numpy(), parents=parents.numpy(),
                   origin=torch.cat([keep, clones, parents, parents]).numpy(), nr=q["nr"])
        return out
    tr, ref = pack(q64), pack(q32)
    thr = {k: float(v) for k, v in q64["thr"].items()}
    with np.errstate(invalid="ignore"):
        m = {"g_split": tr["g"] - thr["max_grad"], "g_clone": np.abs(tr["g"]) - thr["max_grad"],
             "dense": tr["smax"] - thr["dense_scale"], "opacity": tr["o"] - thr["min_opacity"]}
        if q64["use_big"]:
            m["big"], m["child_big"] = tr["smax"] - thr["big_scale"], tr["child_smax"] - thr["big_scale"]

        def rel(k):                                                       # the largest relative deviation over the normal finite sources
            a, b = tr[k], ref[k].astype(np.float64)
            ok = np.isfinite(a) & np.isfinite(b) & (np.abs(a) >= F32_TINY)
            return float((np.abs(b[ok] - a[ok]) / np.abs(a[ok])).max()) if ok.any() else 0.0
        ok = np.isfinite(tr["o"]) & np.isfinite(ref["o"])
        e_ref = {"g": rel("g"), "smax": rel("smax"), "child_smax": rel("child_smax"),
                 "o": float(np.abs(ref["o"].astype(np.float64) - tr["o"])[ok].max()) if ok.any() else 0.0}
        arm, xyz = np.abs(q64["arm"].numpy()), np.abs(tr["xyz"])
        fin = lambda a: np.where(np.isfinite(a), a, 0.0)                                      # noqa: E731
        child_term = np.maximum(fin(arm).max(axis=2), fin(xyz).max(axis=1)[None])
        scaling_term = np.maximum(fin(np.abs(tr["scaling"])).max(axis=1), fin(np.abs(tr["child_scaling"])).max(axis=1))
    agree = all(np.array_equal(tr[k], ref[k]) for k in ("clone", "split", "gone", "child_gone")) and \
        np.array_equal(tr["origin"], ref["origin"])
    tr.update(margin=m, e_ref=e_ref, thr=thr, use_big=q64["use_big"], child_term=child_term, scaling_term=scaling_term, ref32=ref,
              agree=agree)
    return tr


def near_threshold(truth, k):
    """The sources (indices) with a decision quantity within k times its own e_ref of its threshold.  e_ref is |fp32 restatement -
    fp64| of that quantity on this input: for g, smax and the child smax (which span many binades) the largest RELATIVE deviation
    over the input's sources times the threshold, for o (in [0, 1], subnormal at its lower end) the largest absolute one.  A NaN or
    an infinite quantity is on no edge: every comparison with it comes out the same in any arithmetic.  An exact tie is always near."""
    m, e, thr = truth["margin"], truth["e_ref"], truth["thr"]
    band = {"g_split": e["g"] * thr["max_grad"], "g_clone": e["g"] * thr["max_grad"], "dense": e["smax"] * thr["dense_scale"],
            "opacity": e["o"]}
    if truth["use_big"]:
        band.update(big=e["smax"] * thr["big_scale"], child_big=e["child_smax"] * thr["big_scale"])
    near = np.zeros(truth["g"].shape[0], dtype=bool)
    with np.errstate(invalid="ignore"):
        for name, width in band.items():
            near |= np.isfinite(m[name]) & (np.abs(m[name]) <= k * width)
    return np.nonzero(near)[0]


def reset_truth(x):
    """logit(min(sigmoid(x), fl32(0.01))) in fp64 on fp32 x (any shape); a NaN stays."""
    x = np.asarray(x, dtype=np.float32).astype(np.float64)
    with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
        s = 1.0 / (1.0 + np.exp(-x))
        s = np.where(s < float(np.float32(0.01)), s, np.where(np.isnan(s), s, float(np.float32(0.01))))
        return np.log(s / (1.0 - s))


def reset_ref32(x):
    """The fp32 restatement of reset_opacity above on an array."""
    x = torch.as_tensor(np.asarray(x, dtype=np.float32))
    o = torch.min(torch.sigmoid(x), torch.ones_like(x) * 0.01)
    return torch.log(o / (1 - o)).numpy()


def _class(a):
    """0 finite, 1 +inf, 2 -inf, 3 NaN."""
    a = np.asarray(a, dtype=np.float64)
    return np.where(np.isnan(a), 3, np.where(np.isposinf(a), 1, np.where(np.isneginf(a), 2, 0)))


def compare_rows(got, truth64, ref32, term=None, what=""):
    """Rows (n, w) of a kernel's fp32 output against fp64, NaN- and inf-aware.  The class of every element (finite, +inf, -inf,
    NaN) must be the fp32 restatement's.  Elements finite on all three sides are measured in fp32 ulps of their ROW's largest term
    (`term` (n,), default the row's largest finite |truth64|; never below the smallest normal number): the kernel's deviation from
    fp64 may be max(4 e_ref, 1) of them, e_ref being the restatement's largest deviation from fp64 over the same rows in the same
    unit.  Prints the kernel's deviation beside e_ref; returns (deviation, e_ref, bound) in ulps."""
    g = np.asarray(got, dtype=np.float32).astype(np.float64)
    a = np.asarray(truth64, dtype=np.float64)
    b = np.asarray(ref32, dtype=np.float32).astype(np.float64)
    assert g.shape == a.shape == b.shape, (what, g.shape, a.shape, b.shape)
    g, a, b = (x.reshape(x.shape[0], -1) for x in (g, a, b))
    bad = np.nonzero(_class(g) != _class(b))
    assert len(bad[0]) == 0, (what, "class (finite, +inf, -inf, NaN) differs from the fp32 restatement's", len(bad[0]), "elements, first",
                              (int(bad[0][0]), int(bad[1][0])), "kernel", g[bad][0], "restatement", b[bad][0], "fp64", a[bad][0])
    fin = np.isfinite(g) & np.isfinite(a) & np.isfinite(b)
    if term is None:
        term = np.where(np.isfinite(a), np.abs(a), 0.0).max(axis=1) if a.shape[1] else np.zeros(a.shape[0])
    unit = np.spacing(np.maximum(np.asarray(term, dtype=np.float64), F32_TINY).astype(np.float32)).astype(np.float64)[:, None]
    with np.errstate(invalid="ignore"):
        dev = np.where(fin, np.abs(g - a) / unit, 0.0)
        ref = np.where(fin, np.abs(b - a) / unit, 0.0)
    e_ref = float(ref.max()) if ref.size else 0.0
    worst = float(dev.max()) if dev.size else 0.0
    bound = max(MARGIN * e_ref, 1.0)
    print(f"{what}: {int(fin.sum())} finite of {fin.size} elements, kernel deviation {worst:.3f} ulp  e_ref {e_ref:.3f} ulp  "
          f"bound {bound:.3f} ulp")
    if worst > bound:
        r, k = np.unravel_index(np.argmax(dev), dev.shape)
        raise AssertionError((what, "deviation from fp64", worst, "ulp of the row's largest term > bound", bound, "e_ref", e_ref,
                              "row", int(r), "element", int(k), "kernel", g[r, k], "fp64", a[r, k], "restatement", b[r, k]))
    return worst, e_ref, bound


# ---- pattern scenes: fates planted per row, clear of every threshold ------------------------------------------------------------
# thresholds of the pattern scenes: dense_scale = fl32(0.05), big_scale = fl32(1.0)
P_MAX_GRAD, P_MIN_OPACITY, P_EXTENT, P_PERCENT = 4e-4, 0.005, 5.0, 0.01
# fate: (hot, log-scale of the largest axis, raw opacity).  On a background row: keep = it stays; clone = it stays and a copy
# appears; split = it goes and two children appear; prune = it goes; split_gone = it goes and (with the world-size term) so do
# its children.  On a ray-bound row: keep and prune change nothing, clone and split add rows, a split divides its raw scaling.
FATES = {"keep": (False, -2.0, 1.0), "clone": (True, -4.5, 1.0), "split": (True, -1.5, 1.0), "prune": (False, -2.0, -7.0),
         "split_gone": (True, 1.0, 1.0)}
FATE_NAMES = tuple(FATES)


def thresholds32(percent_dense, extent, max_screen_size, max_grad, min_opacity):
    """(max_grad, min_opacity, dense_scale, big_scale or None) as the binding rounds them to fp32."""
    return (np.float32(max_grad), np.float32(min_opacity), np.float32(float(percent_dense) * float(extent)),
            np.float32(0.2 * float(extent)) if max_screen_size else None)


def plant(fates, nr, seed, overrides=None, state_nan=False):
    """(tensors, optimizer states, noise) of a model whose source i has fate fates[i] (a name of FATES) under the pattern
    thresholds, the first nr sources ray-bound.  Row values are jittered (seeded) but stay clear of every threshold: |g| / max_grad
    is 1.75 or 0.25, the largest axis lies within 0.3 of its fate's log-scale, the opacity within 0.2.  features_dc is unique per
    row (origins() finds every row's source).  overrides: {source: {"scaling": (3,), "opacity": x, "rotation": (4,), "accum": x,
    "denom": x, "noise": (2, 3)}} written after the pattern.  state_nan: the ray "scaling" moments hold NaN and inf."""
    P = len(fates)
    nb = P - nr
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)                                               # noqa: E731
    u = lambda *s: torch.rand(*s, generator=g)                                                # noqa: E731
    hot = torch.tensor([FATES[f][0] for f in fates], dtype=torch.bool)
    top = torch.tensor([FATES[f][1] for f in fates], dtype=torch.float32)
    opa = torch.tensor([FATES[f][2] for f in fates], dtype=torch.float32)
    scaling = top[:, None] - u(P, 3) * 1.5                                # the other axes below the largest
    axis = torch.randint(0, 3, (P,), generator=g)
    scaling[torch.arange(P), axis] = top + (u(P) - 0.5) * 0.6
    opacity = (opa + (u(P) - 0.5) * 0.4)[:, None]
    rotation = r(P, 4)
    rotation[rotation.norm(dim=1) < 0.1] = torch.tensor([1.0, 0.0, 0.0, 0.0])
    dc = (torch.arange(3 * P, dtype=torch.float32).reshape(P, 1, 3) - 1.5 * P) / 1024.0      # unique, exact
    rest = r(P, 15, 3) * 0.15
    denom = torch.randint(1, 6, (P, 1), generator=g).float()
    accum = denom * torch.where(hot, 1.75, 0.25)[:, None] * P_MAX_GRAD
    d = r(nr, 3)
    noise = r(2, P, 3)
    t = {"_zval": u(nr, 1) * 6 + 3, "_rayo": r(nr, 3) * 0.1, "_rayd": d / d.norm(dim=1, keepdim=True).clamp_min(1e-6),
         "bg_xyz": r(nb, 3) * 3, "_features_dc": dc[:nr], "bg_features_dc": dc[nr:], "_features_rest": rest[:nr],
         "bg_features_rest": rest[nr:], "_opacity": opacity[:nr], "bg_opacity": opacity[nr:], "_scaling": scaling[:nr],
         "bg_scaling": scaling[nr:], "_rotation": rotation[:nr], "bg_rotation": rotation[nr:],
         "xyz_gradient_accum": accum, "denom": denom, "max_radii2D": torch.full((P,), 1e9)}
    t = {k: v.clone().contiguous() for k, v in t.items()}
    for i, o in (overrides or {}).items():
        pre, j = ("_", i) if i < nr else ("bg_", i - nr)
        for k in ("scaling", "opacity", "rotation"):
            if k in o:
                t[pre + k][j] = torch.as_tensor(o[k], dtype=torch.float32)
        if "xyz" in o:
            assert i >= nr
            t["bg_xyz"][j] = torch.as_tensor(o["xyz"], dtype=torch.float32)
        if "accum" in o:
            t["xyz_gradient_accum"][i] = float(o["accum"])
        if "denom" in o:
            t["denom"][i] = float(o["denom"])
        if "noise" in o:
            noise[:, i] = torch.as_tensor(o["noise"], dtype=torch.float32)
    states = {}
    for a, n, _tail, _lr in RAY + BG:
        if t[a].shape[0]:
            states[n] = (3.0, r(*t[a].shape) * 1e-3, u(*t[a].shape) * 1e-6)
    if state_nan and nr:
        m, v = states["scaling"][1].clone(), states["scaling"][2].clone()
        m[0::3], v[1::3] = float("nan"), float("inf")
        states["scaling"] = (3.0, m, v)
    return t, states, noise


def make_model(t, states, device="cpu", optimizer_cls=torch.optim.Adam, percent_dense=P_PERCENT):
    m = StandIn(t, percent_dense, optimizer_cls, device)
    for n, (step, exp_avg, exp_avg_sq) in states.items():
        m.set_state(n, step, exp_avg, exp_avg_sq)
    return m


def fate_of(truth, i):
    """The benign fate (a name of FATES) that does to source i what the truth says happened to it."""
    if truth["split"][i]:
        return "split_gone" if truth["child_gone"][i] else "split"
    if truth["gone"][i]:
        return "prune"
    return "clone" if truth["clone"][i] else "keep"


def counts_of(truth):
    """(plain, children) per source: how often it appears among the new background rows as a kept original or a clone, and as a
    child."""
    P = truth["g"].shape[0]
    plain = np.bincount(np.concatenate([truth["keep"], truth["clones"]]), minlength=P)
    return plain, 2 * np.bincount(truth["parents"], minlength=P)


def counts_in(before: StandIn, after: StandIn):
    """counts_of from a model pair: a new row whose scaling is not its source's, bit for bit, is a child."""
    origin = origins(before, after).numpy()
    assert (origin >= 0).all(), "a new row whose features_dc is no source's"
    src = torch.cat([before._scaling.detach(), before.bg_scaling.detach()]).cpu().numpy().view(np.uint32)[origin]
    child = (after.bg_scaling.detach().cpu().numpy().view(np.uint32) != src).any(axis=1)
    return np.bincount(origin[~child], minlength=before.P), np.bincount(origin[child], minlength=before.P)


# the non-finite and extreme rows of part C: name -> overrides of a source (hot rows are given twice the planted value's fate)
C_ROWS = {
    "scaling_nan0": {"scaling": (float("nan"), -2.0, -3.0)}, "scaling_nan1": {"scaling": (-2.0, float("nan"), -3.0)},
    "scaling_nan2": {"scaling": (-3.0, -2.0, float("nan"))}, "scaling_pinf": {"scaling": (-2.0, float("inf"), -3.0)},
    "scaling_ninf": {"scaling": (float("-inf"),) * 3},
    "opacity_nan": {"opacity": float("nan")}, "opacity_pinf": {"opacity": float("inf")}, "opacity_ninf": {"opacity": float("-inf")},
    "opacity_m100": {"opacity": -100.0},
    "quat_zero": {"rotation": (0.0, 0.0, 0.0, 0.0)}, "quat_1e-30": {"rotation": (0.6e-30, -0.5e-30, 0.4e-30, 0.48e-30)},
    "quat_nan": {"rotation": (0.5, float("nan"), 0.2, 0.1)},
    "noise_nan": {"noise": ((0.5, float("nan"), -1.0), (float("nan"), 0.25, 1.0)), "rotation": (0.9, 0.3, -0.2, 0.4)},
    "noise_inf": {"noise": ((float("inf"), 0.5, -1.0), (0.25, float("-inf"), 1.0)), "rotation": (0.9, 0.3, -0.2, 0.4)},
}
C_NR, C_P, C_SEED = 150, 300, 11


def nonfinite_scene():
    """(tensors, states, noise, planted): about 300 sources with each row of C_ROWS planted on a ray-bound and on a background row,
    hot and cold, between benign neighbours of every fate.  planted: {(name, "ray" | "bg", "hot" | "cold"): source}.  The quaternion
    and noise rows sit on big sources (hot: a split), the others on their fate's pattern row."""
    gen = np.random.default_rng(C_SEED)
    fates = [FATE_NAMES[k] for k in gen.integers(0, len(FATE_NAMES), C_P)]
    planted, over = {}, {}
    slots = {"ray": iter(range(5, C_NR, 2)), "bg": iter(range(C_NR + 4, C_P, 2))}
    for name, o in C_ROWS.items():
        for side in ("ray", "bg"):
            for heat in ("hot", "cold"):
                i = next(slots[side])
                big = name.startswith(("quat", "noise")) or (name.startswith("opacity") and side == "bg")
                fates[i] = ("split" if big else "clone") if heat == "hot" else "keep"
                planted[(name, side, heat)], over[i] = i, dict(o)
    t, states, noise = plant(fates, C_NR, C_SEED, over)
    return t, states, noise, planted


def benign_twin(truth, planted, seed=C_SEED):
    """The scene of nonfinite_scene with every planted source replaced by a benign row of the same fate (by the truth)."""
    gen = np.random.default_rng(C_SEED)
    fates = [FATE_NAMES[k] for k in gen.integers(0, len(FATE_NAMES), C_P)]
    for i in planted.values():
        fates[i] = fate_of(truth, i)
    return plant(fates, C_NR, seed)


def split_scene(seed):
    """Part B: 3 x 256 + 1 hot sources that all split (dense_scale below every scale, no world-size term, opaque): log-scales from
    -12 to 12 per axis with anisotropy up to 1e6, quaternions of norm 1e-3 .. 1e3, some axis-aligned and some 180-degree rotations,
    noise with rows of 0 and of +-4.  Returns (tensors, states, noise, rows) with rows = {"zero_noise", "dyadic", "isotropic"}: the
    sources of the exact checks.  The thresholds: B_ARGS."""
    P, nr = 3 * 256 + 1, 300
    t, states, noise = plant(["split"] * P, nr, seed)
    g = torch.Generator().manual_seed(seed + 1000)
    u = lambda *s: torch.rand(*s, generator=g)                                                # noqa: E731
    ani = u(P, 1) * np.log(1e6) * (u(P, 1) < 0.7)                                             # 30 % near-isotropic
    base = -12.0 + u(P, 1) * (24.0 - ani)
    scaling = (base + ani * u(P, 3) + (u(P, 3) - 0.5) * 2e-3).clamp(-12.0, 12.0)
    scaling[8], scaling[nr + 8] = torch.tensor([-12.0, -12.0, -11.999]), torch.tensor([12.0, 12.0 - float(np.log(1e6)), 7.0])
    q = torch.randn(P, 4, generator=g)
    q = q / q.norm(dim=1, keepdim=True) * 10 ** (u(P, 1) * 6 - 3)
    idx = torch.arange(P)
    for k in range(4):                                                     # identity, then the three 180-degree rotations
        rows = idx % 16 == k
        q[rows] = torch.eye(4)[k] * q[rows].norm(dim=1, keepdim=True)
    noise = noise.clone()
    zero_noise = idx[idx % 16 == 5]
    noise[:, zero_noise] = 0.0
    four = idx[idx % 16 == 6]
    noise[0, four], noise[1, four] = 4.0, -4.0
    dyadic = idx[(idx % 16 == 7) & (idx >= nr)]                             # identity quaternion, scaling 0, dyadic noise and xyz
    q[dyadic] = torch.tensor([1.0, 0.0, 0.0, 0.0])
    scaling[dyadic] = 0.0
    noise[0, dyadic], noise[1, dyadic] = torch.tensor([0.5, -2.0, 0.25]), torch.tensor([-0.125, 1.0, 3.0])
    t["bg_xyz"][dyadic - nr] = torch.round(t["bg_xyz"][dyadic - nr] * 8) / 8
    t["_scaling"], t["bg_scaling"] = scaling[:nr].clone(), scaling[nr:].clone()
    t["_rotation"], t["bg_rotation"] = q[:nr].clone(), q[nr:].clone()
    iso = idx[(scaling.max(dim=1).values - scaling.min(dim=1).values) < 3e-3]
    return t, states, noise, {"zero_noise": zero_noise.numpy(), "dyadic": dyadic.numpy(), "isotropic": iso.numpy()}


B_EXTENT, B_SEED = 1e-4, 3                         # dense_scale = fl32(1e-6) < exp(-12)
B_ARGS = (P_MAX_GRAD, P_MIN_OPACITY, B_EXTENT, None)


def section_patterns():
    """Part D: {name: (fates, nr, max_screen_size)}.  A workgroup is 256 consecutive sources, a wave 64."""
    W, G = 64, 256
    pat = {}
    pat["a_keeps_in_group0"] = (["keep"] * G + ["prune"] * (2 * G + 44), 0, 20)
    for which in ("first", "last"):
        f = ["prune"] * (3 * G + 5)
        for s in range(0, len(f), G):
            i = s if which == "first" else min(s + G, len(f)) - 1
            f[i] = "clone"                                                  # survives on either set: a clone row (and the kept original)
        pat[f"b_only_{which}_of_each_group"] = (f, 300, 20)
    waves = ["clone", "split", "keep", "prune", "split", "clone", "prune", "clone", "split"]
    pat["c_wave_clones_then_wave_splits"] = ([w for w in waves for _ in range(W)], 200, 20)
    pat["d_group_clone_group_split"] = (["clone"] * G + ["split"] * G + ["clone"] * G + ["split"] * 3, 0, 20)
    pat["d_group_split_group_clone_ray"] = (["split"] * G + ["clone"] * G, 128, None)
    for P in (257, 513):
        pat[f"f_last_of_{P}"] = (["prune"] * (P - 1) + ["keep"], 100, 20)
    big = 65537
    for name, groups in (("group0", (0,)), ("group256", (256,)), ("both", (0, 256))):
        f = ["prune"] * big
        for gi in groups:
            for i in range(gi * G, min((gi + 1) * G, big)):
                f[i] = ("keep", "clone", "split")[i % 3]
        if 0 in groups:
            f[5] = "split"
        pat[f"g_65537_{name}"] = (f, 40 if 0 in groups else 0, 20)
    h = (["split_gone", "keep", "split_gone", "clone"] * 80)[:300]
    pat["h_children_pruned"] = (h, 130, 20)
    pat["h_new_set_empty"] = ((["split_gone"] * 70) + (["split_gone", "prune"] * 50), 70, 20)
    return pat


def boundary_pattern(nr, first, second, seed=0):
    """Part D (e): nr + 70 sources of seeded fates with the pair (last ray-bound, first background) given (first, second)."""
    gen = np.random.default_rng(1000 * nr + seed)
    fates = [FATE_NAMES[k] for k in gen.integers(0, len(FATE_NAMES), nr + 70)]
    fates[nr - 1], fates[nr] = first, second
    return fates


# part E: the planted raw opacities of the reset
RESET_SIZES = ((1, 0), (0, 1), (63, 1), (64, 64), (255, 2), (256, 1), (257, 256))
LOGIT01 = float(np.log(0.01 / 0.99))


def reset_values(n, seed):
    """n raw opacities: the planted values first (as many as fit), then a grid dense around logit(0.01) and through the band where
    fp32 sigmoid is subnormal.  The class of the fp32 result changes at x = -88.72 alone (expf(-x) overflows below it: -inf): the
    overflow band's values stay 6 away from it, the subnormal band's lowest, -88.5, 0.22 (a factor 1.25 in expf's argument)."""
    planted = [float("-inf"), -100.0, -95.0, -88.5, -88.25, -88.0, -87.75, -87.5, -87.4, -20.0, -0.0, 5.0, 100.0, float("inf"),
               float("nan"), LOGIT01, float(np.nextafter(np.float32(LOGIT01), np.float32(0))),
               float(np.nextafter(np.float32(LOGIT01), np.float32(-10)))]
    gen = np.random.default_rng(seed)
    grid = np.concatenate([LOGIT01 + np.linspace(-0.05, 0.05, 41), np.linspace(-88.5, -87.4, 23), gen.normal(0.0, 3.0, 64),
                           LOGIT01 + gen.normal(0.0, 1e-3, 64)])
    vals = np.concatenate([np.array(planted), grid]).astype(np.float32)
    if n <= len(planted):
        start = (seed * 5) % len(planted)
        return np.roll(vals[:len(planted)], -start)[:n].copy()
    return np.resize(vals, n).copy()


# part A: exact ties.  Only values every expf gives exactly are planted: exp(0) = 1, exp(-inf) = 0, sigmoid(0) = 0.5.
NINF = float("-inf")
SCALINGS_ONE = ((0.0, 0.0, 0.0), (0.0, -1.0, NINF), (NINF, 0.0, -1.0), (-1.0, NINF, 0.0))      # smax = 1.0 in three orders
SMALL = (-5.0, -5.5, -6.0)                                                                      # far below dense_scale = 0.05
_COUNTS = {"ray": {"none": (0, 0), "clone": (1, 0), "split": (0, 2), "pruned": (0, 0)},
           "bg": {"none": (1, 0), "clone": (2, 0), "split": (0, 2), "pruned": (0, 0)}}


def tie_scenes():
    """{name: scene} of part A.  A scene: tensors, states, noise, nr, percent_dense, args = (max_grad, min_opacity, extent,
    max_screen_size) for the binding, thr = the fp32 thresholds (max_grad, min_opacity, dense_scale, big_scale or None) the binding
    is MEANT to pass, rows = [(side, hand-made decision)] per source, expect = the (plain, children) counts of that table, classes =
    {edge class: sources}."""
    scenes = {}

    def add(name, rows, percent_dense, args, thr):
        """rows: (side, hot, overrides, decision), ray-bound rows first."""
        rows = sorted(rows, key=lambda r: r[0] != "ray")
        nr = sum(r[0] == "ray" for r in rows)
        fates = ["clone" if r[1] else "keep" for r in rows]
        t, states, noise = plant(fates, nr, 40 + len(scenes), {i: r[2] for i, r in enumerate(rows)})
        classes = {}
        for i, r in enumerate(rows):
            classes.setdefault(f"{r[0]} {r[3]}", []).append(i)
        scenes[name] = dict(tensors=t, states=states, noise=noise, nr=nr, percent_dense=percent_dense, args=args, thr=thr,
                            rows=[(r[0], r[3]) for r in rows], classes=classes,
                            expect=(np.array([_COUNTS[r[0]][r[3]][0] for r in rows]), np.array([_COUNTS[r[0]][r[3]][1] for r in rows])))

    one = {"prev": prev32(1.0), "tie": np.float32(1.0), "next": next32(1.0)}
    mg, mo = np.float32(P_MAX_GRAD), np.float32(P_MIN_OPACITY)
    for k, v in one.items():                       # dense_scale: percent_dense = 1, extent the float itself
        rows = [(side, hot, {"scaling": sc, "opacity": 0.0}, ("split" if k == "prev" else "clone") if hot else "none")
                for side in ("ray", "bg") for sc in SCALINGS_ONE for hot in (True, False)]
        add(f"dense_{k}", rows, 1.0, (float(mg), float(mo), float(v), None), (mg, mo, v, None))
    for k, v in one.items():                       # big_scale = fl32(0.2 * extent) on cold opaque rows of smax = 1.0
        for mss in (20, None):
            rows = [(side, False, {"scaling": sc, "opacity": 3.0}, "pruned" if (side == "bg" and k == "prev" and mss) else "none")
                    for side in ("ray", "bg") for sc in SCALINGS_ONE]
            extent = 5.0 * float(v)
            add(f"big_{k}_mss{mss}", rows, P_PERCENT, (float(mg), float(mo), extent, mss),
                (mg, mo, np.float32(P_PERCENT * extent), v if mss else None))
    half = {"prev": prev32(0.5), "tie": np.float32(0.5), "next": next32(0.5)}
    for k, v in half.items():                      # min_opacity on rows of raw opacity 0: the original, its clone, its children
        gone = k == "next"
        rows = [("bg", False, {"opacity": 0.0, "scaling": SMALL}, "pruned" if gone else "none"),
                ("bg", True, {"opacity": 0.0, "scaling": SMALL}, "pruned" if gone else "clone"),
                ("ray", True, {"opacity": 0.0, "scaling": SMALL}, "pruned" if gone else "clone"),
                ("ray", True, {"opacity": 0.0, "scaling": SCALINGS_ONE[1]}, "pruned" if gone else "split"),
                ("bg", True, {"opacity": 0.0, "scaling": SCALINGS_ONE[2]}, "pruned" if gone else "split"),
                ("ray", False, {"opacity": 0.0, "scaling": SMALL}, "none")]
        add(f"opacity_{k}", rows, P_PERCENT, (float(mg), float(v), P_EXTENT, None), (mg, v, np.float32(P_PERCENT * P_EXTENT), None))
    inf, m = float("inf"), float(mg)
    grads = {"prev": (float(prev32(mg)), 1.0, "none", "none"), "tie": (m, 1.0, "clone", "split"),
             "next": (float(next32(mg)), 1.0, "clone", "split"), "minus": (-m, 1.0, "clone", "none"),
             "minus_inf": (-inf, 1.0, "clone", "none"), "plus_inf": (inf, 1.0, "clone", "split"),
             "inf_by_inf": (inf, inf, "none", "none"), "zero_by_zero": (0.0, 0.0, "none", "none"),
             "x_by_minus_zero": (1.0, -0.0, "clone", "none")}
    rows = []
    for _k, (accum, denom, small, big) in grads.items():
        for side in ("ray", "bg"):
            rows.append((side, False, {"accum": accum, "denom": denom, "scaling": SMALL, "opacity": 1.0}, small))
            rows.append((side, False, {"accum": accum, "denom": denom, "scaling": SCALINGS_ONE[0], "opacity": 1.0}, big))
    add("grad", rows, P_PERCENT, (m, float(mo), P_EXTENT, None), (mg, mo, np.float32(P_PERCENT * P_EXTENT), None))
    scenes["grad"]["grads"] = {k: v[:2] for k, v in grads.items()}
    return scenes


def _bits(a):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def assert_copied(got: StandIn, before: StandIn, truth, what, skip_sources=()):
    """Everything of `got` that is a copy or a single IEEE operation against `before` and the truth's sections, BIT for bit (a NaN
    keeps its bits): the structure, every copied attribute of every new row, xyz and scaling of kept originals and clones, the
    moments (gathered for kept originals, +0 for new rows, +0 for the whole ray "scaling" group), the ray-bound tensors (untouched;
    a split source's raw scaling / 1.6), the statistics (zero, nr + rows long).  skip_sources: new rows and ray scaling rows of these
    sources are left out.  Returns the bool mask of the child rows."""
    nr, origin = truth["nr"], truth["origin"]
    K, C, S = len(truth["keep"]), len(truth["clones"]), len(truth["parents"])
    rows = K + C + 2 * S
    assert got._zval.shape[0] == nr and got.bg_xyz.shape[0] == rows, (what, "rows", got.bg_xyz.shape[0], "expected", rows)
    assert np.array_equal(origins(before, got).numpy(), origin), (what, "source of the new rows")
    live = ~np.isin(origin, np.asarray(list(skip_sources), dtype=np.int64))
    child = np.arange(rows) >= K + C
    both = lambda r, b: torch.cat([getattr(before, r).detach(), getattr(before, b).detach()]).cpu()      # noqa: E731
    for r, b in (("_features_dc", "bg_features_dc"), ("_features_rest", "bg_features_rest"), ("_opacity", "bg_opacity"),
                 ("_rotation", "bg_rotation")):
        assert np.array_equal(_bits(getattr(got, b))[live], _bits(both(r, b))[origin][live]), (what, b, "copied rows")
    plain = live & ~child
    assert np.array_equal(_bits(got.bg_scaling)[plain], _bits(both("_scaling", "bg_scaling"))[origin][plain]), (what, "bg_scaling")
    assert np.array_equal(_bits(got.bg_xyz)[plain], _bits(truth["ref32"]["xyz"])[origin][plain]), (what, "bg_xyz of originals and clones")
    for a, n, _tail, _lr in BG:
        sg, sb = got.group_state(n), before.group_state(n)
        assert (sg is None) == (sb is None), (what, n, "optimizer state present")
        if sb is None:
            continue
        assert float(sg["step"]) == float(sb["step"]), (what, n, "step")
        for k in ("exp_avg", "exp_avg_sq"):
            assert sg[k].shape == getattr(got, a).shape, (what, n, k, sg[k].shape)
            want = np.zeros(_bits(sg[k]).shape, dtype=np.uint32)
            want[:K] = _bits(sb[k])[truth["keep"] - nr]
            assert np.array_equal(_bits(sg[k])[live], want[live]), (what, n, k)
    for a, n, _tail, _lr in RAY:
        sg, sb = got.group_state(n), before.group_state(n)
        assert (sg is None) == (sb is None), (what, n, "optimizer state present")
        keep_rows = ~np.isin(np.arange(nr), np.asarray(list(skip_sources), dtype=np.int64))
        if a == "_scaling":
            want = _bits(before._scaling).copy()
            hit = truth["split"][:nr]
            want[hit] = _bits(truth["ref32"]["ray_scaling"])[hit]
            assert np.array_equal(_bits(got._scaling)[keep_rows], want[keep_rows]), (what, "ray-bound raw scaling")
        else:
            assert np.array_equal(_bits(getattr(got, a)), _bits(getattr(before, a))), (what, a, "ray-bound tensor changed")
        if sb is not None:
            for k in ("exp_avg", "exp_avg_sq"):
                want = np.zeros_like(_bits(sb[k])) if a == "_scaling" else _bits(sb[k])
                assert np.array_equal(_bits(sg[k]), want), (what, n, k)
    for a, tail in STATS:
        x = getattr(got, a)
        assert tuple(x.shape) == (nr + rows,) + tail and not _bits(x).any(), (what, a, "zero and nr + rows long")
    return child

"""The reference's densify_and_prune and reset_opacity as plain torch, a stand-in model class with the reference model's attribute
names, and the cases of tests/golden/ref_densify.npz.

`densify_and_prune` restates GaussianModel.densify_and_prune (scene/gaussian_model.py:758-930) and `reset_opacity` :644-651 in this
project's words, taking the split's unit normal samples explicitly (noise[copy, source]); tests/test_densify_cpu.py holds both to the
arrays the reference's own code produced.  tools/densify_timing.py times the restatement as the torch leg."""
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

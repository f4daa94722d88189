"""scgaussian_amd.optim on the GPU: ArenaAdam against torch.optim.Adam (default implementation, run on copies), the SH-tail skip,
captured steps, and the densification statistics against the reference's own numbers."""
import copy
import importlib.util
import os

import numpy as np
import pytest
import torch

import parity_utils as pu
from scgaussian_amd import optim as O
from scgaussian_amd import synthetic as syn

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"

# the reference's two optimizers (scene/gaussian_model.py:496-512, arguments/__init__.py defaults, spatial_lr_scale 1)
RAY = [("zval", "zval", 1.6e-4), ("features_dc", "f_dc", 2.5e-3), ("features_rest", "f_rest", 2.5e-3 / 20),
       ("opacity", "opacity", 5e-2), ("scaling", "scaling", 5e-3), ("rotation", "rotation", 1e-3)]
BG = [("bg_xyz", "bg_xyz", 1.6e-4), ("bg_features_dc", "bg_f_dc", 2.5e-3), ("bg_features_rest", "bg_f_rest", 2.5e-3 / 20),
      ("bg_opacity", "bg_opacity", 5e-2), ("bg_scaling", "bg_scaling", 5e-3), ("bg_rotation", "bg_rotation", 1e-3)]


def _tensors(P=3001, seed=0):
    """The raw model's twelve tensors (odd counts: odd numel in several segments)."""
    sc = syn.make_scene(P, 64, 48, seed=seed)
    m = syn.make_raw_model(sc)
    return {a: getattr(m, a).detach().clone().to(DEV) for a, _, _ in RAY + BG}


class Model:
    """Just enough of the reference's GaussianModel for its optimizer surgery: leaf tensors + two optimizers."""

    def __init__(self, tensors, cls, with_bg=True):
        self.t = {k: torch.nn.Parameter(v.clone()) for k, v in tensors.items()}
        mk = lambda spec: [{"params": [self.t[a]], "lr": lr, "name": n} for a, n, lr in spec]  # noqa: E731
        self.optimizer = cls(mk(RAY), lr=0.0, eps=1e-15)
        self.optimizer_bg = cls(mk(BG), lr=0.0, eps=1e-15) if with_bg else None

    def opts(self):
        return [o for o in (self.optimizer, self.optimizer_bg) if o is not None]

    def set_grads(self, grads):
        for k, p in self.t.items():
            p.grad = None if grads.get(k) is None else grads[k].clone()

    def step(self, it):
        # the position lr schedule (update_learning_rate: zval and bg_xyz follow an exponential decay)
        for o in self.opts():
            for g in o.param_groups:
                if g["name"] in ("zval", "bg_xyz"):
                    g["lr"] = 1.6e-4 * (0.99 ** it)
            o.step()

    # ---- the reference's state surgery, restated (gaussian_model.py:517-530, 758-840) ----
    def _swap(self, opt, name, new_t, moments):
        g = next(g for g in opt.param_groups if g["name"] == name)
        old = g["params"][0]
        st = opt.state.get(old, None)
        new_p = torch.nn.Parameter(new_t)
        if st:
            st["exp_avg"], st["exp_avg_sq"] = moments(st["exp_avg"]), moments(st["exp_avg_sq"])
            del opt.state[old]
            opt.state[new_p] = st
        g["params"][0] = new_p
        return new_p

    def prune(self, keep_ray, keep_bg):
        for o, spec, keep in ((self.optimizer, RAY, keep_ray), (self.optimizer_bg, BG, keep_bg)):
            for a, n, _ in spec:
                self.t[a] = self._swap(o, n, self.t[a][keep].detach(), lambda m, k=keep: m[k])

    def cat(self, ext):
        for o, spec in ((self.optimizer, RAY), (self.optimizer_bg, BG)):
            for a, n, _ in spec:
                e = ext[a]
                self.t[a] = self._swap(o, n, torch.cat([self.t[a].detach(), e]),
                                       lambda m, e=e: torch.cat([m, torch.zeros_like(e)]))

    def replace(self, attr, name, value):
        o = self.optimizer if not attr.startswith("bg_") else self.optimizer_bg
        self.t[attr] = self._swap(o, name, value, torch.zeros_like)


def _grads(tensors, gen, rest_cols=45, drop=()):
    out = {}
    for k, v in tensors.items():
        g = torch.randn(v.shape, generator=gen, device=DEV) * 1e-2
        if k.endswith("features_rest"):
            flat = g.view(g.shape[0], -1)
            flat[:, rest_cols:] = 0
        out[k] = None if k in drop else g
    return out


def _assert_parity(a: Model, b: Model, what=""):
    for oa, ob in zip(a.opts(), b.opts()):
        for ga, gb in zip(oa.param_groups, ob.param_groups):
            pa, pb = ga["params"][0], gb["params"][0]
            lr = ga["lr"]
            bound = 1e-6 * pb.abs() + 1e-5 * lr
            assert bool(((pa - pb).abs() <= bound).all()), (what, ga["name"], float((pa - pb).abs().max()))
            sa, sb = oa.state.get(pa), ob.state.get(pb)
            assert bool(sa) == bool(sb), (what, ga["name"])
            if not sa:
                continue
            for key in ("exp_avg", "exp_avg_sq"):
                ma, mb = sa[key], sb[key]
                scale = float(mb.abs().max()) if mb.numel() else 0.0
                assert float((ma - mb).abs().max()) <= 1e-5 * scale, (what, ga["name"], key)
            assert float(sa["step"]) == float(sb["step"]), (what, ga["name"])
            assert sa["step"].is_cuda


@pytest.mark.parametrize("with_bg", [True, False])
def test_adam_parity_twelve_groups(with_bg):
    base = _tensors()
    a, b = Model(base, O.ArenaAdam, with_bg), Model(base, torch.optim.Adam, with_bg)
    gen = torch.Generator(device=DEV).manual_seed(7)
    for it in range(1, 101):
        drop = ("rotation",) if it % 7 == 3 else ()                      # a step without that parameter's gradient
        g = _grads(base, gen, drop=drop)
        a.set_grads(g)
        b.set_grads(g)
        a.step(it)
        b.step(it)
        if it in (1, 10, 100):
            torch.cuda.synchronize()
            _assert_parity(a, b, f"step {it}")
    assert all(o.fallback_steps == 0 for o in a.opts())


def test_adam_parity_unaligned_and_odd_segments():
    gen = torch.Generator(device=DEV).manual_seed(3)
    bufs = [torch.randn(n + 1, device=DEV, generator=gen) for n in (1001, 4099, 45 * 37)]
    shapes = [(1001,), (4099,), (37, 15, 3)]
    pa = [torch.nn.Parameter(b[1:].view(s)) for b, s in zip(bufs, shapes)]     # data_ptr 4 bytes past a 16-byte boundary
    pb = [torch.nn.Parameter(b[1:].view(s).clone()) for b, s in zip(bufs, shapes)]
    assert all(p.data_ptr() % 16 == 4 for p in pa)
    oa = O.ArenaAdam([{"params": [p], "lr": 1e-3 * (i + 1)} for i, p in enumerate(pa)], eps=1e-15)
    ob = torch.optim.Adam([{"params": [p], "lr": 1e-3 * (i + 1)} for i, p in enumerate(pb)], eps=1e-15)
    for _ in range(10):
        for x, y in zip(pa, pb):
            gb = torch.randn(x.numel() + 1, device=DEV, generator=gen)
            x.grad = gb[1:].view(x.shape)                                          # unaligned gradient too
            y.grad = x.grad.clone()
        oa.step()
        ob.step()
    torch.cuda.synchronize()
    assert oa.fallback_steps == 0
    for i, (x, y) in enumerate(zip(pa, pb)):
        assert bool(((x - y).abs() <= 1e-6 * y.abs() + 1e-5 * 1e-3 * (i + 1)).all())
        for key in ("exp_avg", "exp_avg_sq"):
            ref = ob.state[y][key]
            assert float((oa.state[x][key] - ref).abs().max()) <= 1e-5 * float(ref.abs().max())


def test_sh_tail_skip_is_exact_and_follows_the_degree():
    base = _tensors()
    a, b = Model(base, O.ArenaAdam), Model(base, torch.optim.Adam)
    gen = torch.Generator(device=DEV).manual_seed(11)
    rest = ("features_rest", "bg_features_rest")
    it = 0
    for _ in range(50):                                                  # SH degree 0: features_rest gets zero gradients
        it += 1
        g = _grads(base, gen, rest_cols=0)
        a.set_grads(g)
        b.set_grads(g)
        a.step(it)
        b.step(it)
    torch.cuda.synchronize()
    for k in rest:
        pa, pb = a.t[k], b.t[k]
        oa = a.optimizer if k == "features_rest" else a.optimizer_bg
        ob = b.optimizer if k == "features_rest" else b.optimizer_bg
        assert torch.equal(pa, base[k]) and torch.equal(pa, pb)          # bitwise untouched, bitwise torch's
        assert torch.equal(oa.state[pa]["exp_avg"], ob.state[pb]["exp_avg"])
        assert torch.equal(oa.state[pa]["exp_avg_sq"], ob.state[pb]["exp_avg_sq"])
        assert not bool(oa.state[pa]["exp_avg"].any())
        assert oa.live_columns()[pa] == 0
    _assert_parity(a, b, "degree 0")
    for _ in range(10):                                                  # degree 1: columns < 9 of each row
        it += 1
        g = _grads(base, gen, rest_cols=9)
        a.set_grads(g)
        b.set_grads(g)
        a.step(it)
        b.step(it)
    torch.cuda.synchronize()
    _assert_parity(a, b, "degree 1")
    assert a.optimizer.live_columns()[a.t["features_rest"]] == 9
    assert a.optimizer_bg.live_columns()[a.t["bg_features_rest"]] == 9
    # densification's surgery: prune, cat, reset of the opacities (new moments: the next step re-derives the watermark)
    nr, nb = base["zval"].shape[0], base["bg_xyz"].shape[0]
    keep_r = torch.arange(nr, device=DEV) % 5 != 2
    keep_b = torch.arange(nb, device=DEV) % 3 != 0
    for m in (a, b):
        m.prune(keep_r, keep_b)
    ext_src = _tensors(P=501, seed=4)
    for m in (a, b):
        m.cat({k: v.clone() for k, v in ext_src.items()})
        m.replace("opacity", "opacity", torch.full_like(m.t["opacity"], -2.0))
    shapes = {k: v.shape for k, v in a.t.items()}
    for _ in range(3):
        it += 1
        g = _grads({k: torch.empty(s, device=DEV) for k, s in shapes.items()}, gen, rest_cols=9)
        a.set_grads(g)
        b.set_grads(g)
        a.step(it)
        b.step(it)
    torch.cuda.synchronize()
    _assert_parity(a, b, "after prune + cat + replace")
    assert a.optimizer.live_columns()[a.t["features_rest"]] == 9
    assert a.optimizer_bg.live_columns()[a.t["bg_features_rest"]] == 9
    # a torch Adam checkpoint loaded into ArenaAdam
    for oa, ob in zip(a.opts(), b.opts()):
        oa.load_state_dict(copy.deepcopy(ob.state_dict()))
    for _ in range(5):
        it += 1
        g = _grads({k: torch.empty(s, device=DEV) for k, s in shapes.items()}, gen, rest_cols=9)
        a.set_grads(g)
        b.set_grads(g)
        a.step(it)
        b.step(it)
    torch.cuda.synchronize()
    _assert_parity(a, b, "after load_state_dict")
    assert a.optimizer.live_columns()[a.t["features_rest"]] == 9


def test_captured_step_equals_eager_bitwise():
    base = _tensors()
    a, b = Model(base, O.ArenaAdam), Model(base, O.ArenaAdam)
    gen = torch.Generator(device=DEV).manual_seed(5)
    seq = [_grads(base, gen, rest_cols=9) for _ in range(22)]
    for m in (a, b):                                                     # eager steps: state, watermarks
        for it in range(2):
            m.set_grads(seq[it])
            m.step(it)
    a.set_grads(seq[1])                                                  # the static gradients the graph reads
    static = {k: p.grad for k, p in a.t.items()}
    for o in a.opts():
        o.sync_hyperparameters()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for o in a.opts():
            o.step()
    for r in range(20):
        g = seq[2 + r]
        for k, t in static.items():
            t.copy_(g[k])
        if r == 7:
            for m in (a, b):
                for o in m.opts():
                    o.param_groups[1]["lr"] *= 0.5                       # features_dc / bg_features_dc
            for o in a.opts():
                o.sync_hyperparameters()
        graph.replay()
        b.set_grads(g)
        for o in b.opts():
            o.step()
    torch.cuda.synchronize()
    for oa, ob in zip(a.opts(), b.opts()):
        for ga, gb in zip(oa.param_groups, ob.param_groups):
            pa, pb = ga["params"][0], gb["params"][0]
            assert torch.equal(pa, pb), ga["name"]
            for key in ("exp_avg", "exp_avg_sq", "step"):
                assert torch.equal(oa.state[pa][key], ob.state[pb][key]), (ga["name"], key)
    assert float(a.optimizer.state[a.t["zval"]]["step"]) == 22
    assert a.optimizer.live_columns()[a.t["features_rest"]] == 9
    del graph


def test_captured_training_step_with_arena_adam_and_densification_stats():
    spec = importlib.util.spec_from_file_location("fit_captured", os.path.join(ROOT, "examples", "fit_captured.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    h, _ = mod.fit(iters=150, P=4000, W=192, H=144, captured=True, verbose=False, arena_adam=True)
    assert h[-1][2] > h[0][2] + 3.0, h                                   # the bar of the captured fit with torch's Adam
    max_r, acc, den = mod.fit.densification
    assert float(den.max()) >= 150 // 3 and bool((acc >= 0).all()) and float(acc.max()) > 0
    assert bool(((den > 0).squeeze(1) == (max_r > 0)).all())


def test_densification_stats_match_the_reference():
    ref = np.load(os.path.join(ROOT, "tests", "golden", "ref_model.npz"))
    g2d = torch.from_numpy(ref["render_plain_grad_viewspace"]).to(DEV)
    radii = torch.from_numpy(ref["render_plain_radii"]).to(DEV)
    P = radii.numel()
    acc, den = torch.zeros(P, 1, device=DEV), torch.zeros(P, 1, device=DEV)
    gen = torch.Generator(device=DEV).manual_seed(2)
    max_r = (torch.rand(P, generator=gen, device=DEV) * 20).floor()
    want_r = max_r.clone()
    vis = radii > 0
    want_r[vis] = torch.max(want_r[vis], radii[vis])
    O.densification_stats(max_r, acc, den, g2d, radii)
    torch.cuda.synchronize()
    pu.assert_close(acc, ref["densify_accum"], "densify accum")
    assert np.array_equal(den.cpu().numpy(), ref["densify_denom"])
    assert torch.equal(max_r, want_r)
    # a second view accumulates; a strided gradient (the (P, 3) slot's first two columns) reads the same numbers
    O.densification_stats(max_r, acc, den, g2d[:, :2], radii)
    torch.cuda.synchronize()
    assert np.array_equal(den.cpu().numpy(), 2 * ref["densify_denom"])
    pu.assert_close(acc, 2 * ref["densify_accum"], "densify accum x2")


# Densification statistics at the edges.  Reference: the reference's three statements (train.py:191-192, gaussian_model.py:932-934)
#     max_radii2D[vis] = max(max_radii2D[vis], radii[vis]);  accum[vis] += norm(grad[vis, :2], dim=-1, keepdim=True);  denom[vis] += 1
# with vis = radii > 0, evaluated in fp64 on the CPU and rounded to fp32.
#   P        1, 255, 256, 257 (around the 256-thread workgroup), 100 003
#   radii    positive, 0 and negative
#   layout   (P,2), (P,3), a [:, :2] view of (P,4): row strides 2, 3, 4
#   poison   NaN / Inf gradients in rows with radii <= 0 must not reach accum
STATS_P = [1, 255, 256, 257, 100003]
STATS_LAYOUTS = ["p2", "p3", "p4_view"]


def _stats_inputs(P, layout, seed):
    g = torch.Generator().manual_seed(seed)
    radii = torch.randint(-3, 40, (P,), generator=g, dtype=torch.int32)
    if P >= 3:
        radii[0], radii[1], radii[-1] = 0, -1, 17                 # all three kinds present, the last row visible
    else:
        radii[:] = 5
    cols = {"p2": 2, "p3": 3, "p4_view": 4}[layout]
    grad = torch.randn(P, cols, generator=g) * 1e-3
    hidden = radii <= 0
    poison = torch.tensor([float("nan"), float("inf"), -float("inf")])
    grad[hidden] = poison[torch.randint(0, 3, (int(hidden.sum()), cols), generator=g)]
    acc = torch.rand(P, 1, generator=g) * 1e-2
    den = torch.randint(0, 30, (P, 1), generator=g).float()
    max_r = (torch.rand(P, generator=g) * 30).floor()
    return radii, grad, acc, den, max_r


def _stats_reference(radii, grad, acc, den, max_r):
    vis = radii > 0
    acc64, den64, max64 = acc.double().clone(), den.double().clone(), max_r.double().clone()
    max64[vis] = torch.max(max64[vis], radii[vis].double())
    acc64[vis] += torch.norm(grad.double()[vis, :2], dim=-1, keepdim=True)
    den64[vis] += 1
    return acc64.float(), den64.float(), max64.float()


def _stats_run(radii, grad, acc, den, max_r, layout, no_grad=False, side_stream=False):
    gd = grad.to(DEV)
    gd = gd[:, :2] if layout == "p4_view" else gd
    assert gd.stride(0) == {"p2": 2, "p3": 3, "p4_view": 4}[layout]
    a, d, m, r = acc.to(DEV), den.to(DEV), max_r.to(DEV), radii.to(DEV)
    torch.cuda.synchronize()
    if side_stream:
        st = torch.cuda.Stream()
        with torch.cuda.stream(st):
            O.densification_stats(m, a, d, gd, r)
        st.synchronize()
    elif no_grad:
        with torch.no_grad():
            O.densification_stats(m, a, d, gd, r)
    else:
        O.densification_stats(m, a, d, gd, r)
    torch.cuda.synchronize()
    return a.cpu(), d.cpu(), m.cpu()


@pytest.mark.parametrize("layout", STATS_LAYOUTS)
@pytest.mark.parametrize("P", STATS_P)
def test_densification_stats_edges_against_fp64(P, layout):
    inp = _stats_inputs(P, layout, seed=P + len(layout))
    radii = inp[0]
    want_a, want_d, want_m = _stats_reference(*inp)
    a, d, m = _stats_run(*inp, layout)
    assert torch.isfinite(a).all()                                # no poison from an invisible row
    pu.assert_close(a, want_a, f"densify accum P={P} {layout}")
    assert torch.equal(d, want_d) and torch.equal(m, want_m)
    hidden = radii <= 0                                           # invisible rows are untouched, to the bit
    assert torch.equal(a[hidden], inp[2][hidden]) and torch.equal(d[hidden], inp[3][hidden]) and torch.equal(m[hidden], inp[4][hidden])
    if P >= 3:
        assert bool(hidden.any()) and bool((radii < 0).any()) and bool((radii == 0).any())
    # inside torch.no_grad() and on a side stream: the same numbers
    for kw in (dict(no_grad=True), dict(side_stream=True)):
        a2, d2, m2 = _stats_run(*inp, layout, **kw)
        assert torch.equal(a2, a) and torch.equal(d2, d) and torch.equal(m2, m), kw

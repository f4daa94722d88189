"""densify.densify_and_prune / reset_opacity (csrc/densify.hip) on the GPU: against the arrays recorded from the reference's own
Python (tests/golden/ref_densify.npz), against the plain-torch restatement (tests/densify_refs.py, run on the CPU) at the sizes where
the three kernels take another path, the hand-over to the next optimizer step, and determinism."""
import math

import pytest
import torch

import densify_refs as D
import parity_utils as pu
from scgaussian_amd import _lib, densify, optim as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
FX = D.fixture()
MAX_GRAD, MIN_OPACITY, EXTENT = 4e-4, 0.005, 5.0
RAY_ATTRS = [r[0] for r in D.RAY] + [f[0] for f in D.FIXED]
OPTIMIZERS = {"torch": torch.optim.Adam, "arena": O.ArenaAdam}


# ---- against the reference's own results -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", list(OPTIMIZERS))
@pytest.mark.parametrize("tag", D.CASES)
def test_fixture_densify_and_prune(tag, kind):
    before = D.load_case(FX, tag, "in")
    got = D.load_case(FX, tag, "in", DEV, OPTIMIZERS[kind])
    kept = {a: getattr(got, a) for a in RAY_ATTRS}
    densify.densify_and_prune(got, *D.case_args(FX, tag), noise=torch.from_numpy(FX[f"{tag}_noise"]).to(DEV))
    for a, t in kept.items():
        assert getattr(got, a) is t, (a, "ray-bound tensors keep their identity")
    for a, n, _t, _lr in D.BG:
        p = getattr(got, a)
        grp = next(g for g in got.optimizer_bg.param_groups if g["name"] == n)
        assert grp["params"][0] is p and isinstance(p, torch.nn.Parameter) and p.requires_grad and p.is_contiguous()
        assert len(got.optimizer_bg.state) == (6 if before.group_state(n) is not None else 0)
    D.assert_same_model(got, D.load_case(FX, tag, "out"), before, f"{tag} {kind}")


@pytest.mark.parametrize("kind", list(OPTIMIZERS))
def test_fixture_reset_opacity(kind):
    before = D.load_case(FX, "reset", "in")
    got = D.load_case(FX, "reset", "in", DEV, OPTIMIZERS[kind])
    kept = (got._opacity, got.bg_opacity)
    densify.install(got)
    got.reset_opacity()
    assert got._opacity is kept[0] and got.bg_opacity is kept[1]
    D.assert_same_model(got, D.load_case(FX, "reset", "out"), before, f"reset {kind}", reset=True)


# ---- against the restatement ---------------------------------------------------------------------------------------------------
def make_inputs(nr, nb, seed, mode="mixed"):
    """Tensors of a model of nr + nb Gaussians (CPU).  No row sits within 1e-3 relative of a threshold behind an exp (the CPU's and
    the GPU's exp may differ by an ulp; which side of a threshold a row is on must not depend on that)."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)                                             # noqa: E731
    P = nr + nb
    centre = {"mixed": -3.0, "ws_row": -3.0, "none": -3.0, "prune_all": -3.0, "clone": -4.5, "split": -1.5}[mode]
    spread = 0.6 if centre == -3.0 else 0.2

    def one_set(n):
        s = dict(features_dc=torch.rand(n, 1, 3, generator=g) * 3 - 1.5, features_rest=r(n, 15, 3) * 0.15, opacity=r(n, 1) * 2,
                 scaling=r(n, 3) * spread + centre, rotation=r(n, 4))
        if mode == "mixed" and n:
            big = torch.rand(n, generator=g) < 0.06                       # beyond 0.2 * extent; some with children that are not
            s["scaling"][big, 0] = torch.where(torch.rand(int(big.sum()), generator=g) < 0.5, 0.3, 0.7)
            s["opacity"][torch.rand(n, generator=g) < 0.06] = -6.5        # below min_opacity
        return s
    ray, bg = one_set(nr), one_set(nb)
    d = r(nr, 3)
    t = {"_zval": torch.rand(nr, 1, generator=g) * 6 + 3, "_rayo": r(nr, 3) * 0.1, "_rayd": d / d.norm(dim=1, keepdim=True).clamp_min(1e-6),
         "bg_xyz": r(nb, 3) * 3}
    t.update({"_" + k: v for k, v in ray.items()})
    t.update({"bg_" + k: v for k, v in bg.items()})
    if mode == "prune_all":
        t["bg_opacity"][:] = -7.0
    if mode == "ws_row":                                                  # a cold row only the world-size term can remove
        t["bg_scaling"][1] = torch.tensor([0.3, -1.0, -2.0])
        t["bg_opacity"][1] = 2.0
    for k in ("_scaling", "bg_scaling"):                                  # keep clear of dense_scale, big_scale and 1.6 * big_scale
        s = torch.exp(t[k].double()).max(dim=1).values
        near = sum(((s / thr - 1).abs() < 1e-3) for thr in (0.01 * EXTENT, 0.2 * EXTENT, 0.32 * EXTENT)) > 0
        t[k][near] += 0.01
    for k in ("_opacity", "bg_opacity"):
        near = (t[k] - math.log(MIN_OPACITY / (1 - MIN_OPACITY))).abs() < 0.01
        t[k][near] -= 0.05
    denom = torch.randint(1, 6, (P, 1), generator=g).float()
    heat = {"mixed": torch.rand(P, 1, generator=g) * 2, "ws_row": torch.rand(P, 1, generator=g) * 2, "none": torch.zeros(P, 1),
            "prune_all": torch.zeros(P, 1), "clone": torch.full((P, 1), 1.75), "split": torch.full((P, 1), 1.75)}[mode]
    accum = denom * heat * MAX_GRAD
    if mode == "ws_row":
        accum[nr + 1] = 0.0
    if mode == "mixed" and P > 8:
        denom[P // 3], accum[P // 3] = 0.0, 0.0                           # NaN -> 0
        denom[P // 2], accum[P // 2] = 0.0, 1.0                           # inf: selected
        denom[P // 5], accum[P // 5] = 2.0, 2 * torch.tensor(MAX_GRAD)    # == max_grad bit for bit: selected
    t.update(xyz_gradient_accum=accum, denom=denom, max_radii2D=torch.full((P,), 1e9))      # huge: must remove nothing
    states = {}
    for a, n, _tail, _lr in D.RAY + D.BG:
        if t[a].shape[0]:
            states[n] = (3.0, r(*t[a].shape) * 1e-3, torch.rand(t[a].shape, generator=g) * 1e-6)
    return t, states, torch.randn(2, P, 3, generator=g)


def build(t, states, device, optimizer_cls):
    m = D.StandIn(t, 0.01, optimizer_cls, device)
    for n, (step, exp_avg, exp_avg_sq) in states.items():
        m.set_state(n, step, exp_avg, exp_avg_sq)
    return m


_REF = {}


def reference(key, mss=20):
    """(inputs, states, noise, model before, model after the restatement on the CPU, its info), computed once per case."""
    if (key, mss) not in _REF:
        t, states, noise = make_inputs(*key)
        after = build(t, states, "cpu", torch.optim.Adam)
        info = D.densify_and_prune(after, MAX_GRAD, MIN_OPACITY, EXTENT, mss, noise)
        _REF[(key, mss)] = (t, states, noise, build(t, states, "cpu", torch.optim.Adam), after, info)
    return _REF[(key, mss)]


def run_gpu(key, mss=20, kind="arena", with_state=True):
    t, states, noise, before, want, info = reference(key, mss)
    got = build(t, states if with_state else {}, DEV, OPTIMIZERS[kind])
    kept = {a: getattr(got, a) for a in RAY_ATTRS}
    densify.install(got)
    got.densify_and_prune(MAX_GRAD, MIN_OPACITY, EXTENT, mss, noise=noise.to(DEV))
    for a, x in kept.items():
        assert getattr(got, a) is x, a
    return got, want, before, info


# P = 1, 63, 64, 65 (a wavefront), 255, 256, 257 (a workgroup), 65 537 (one more source than one round of the scan workgroup covers:
# 256 workgroups of 256 sources)
SIZES = [(1, 0), (0, 1), (31, 32), (32, 32), (33, 32), (128, 127), (128, 128), (129, 128), (32769, 32768)]


@pytest.mark.parametrize("nr,nb", SIZES)
def test_sizes_against_the_restatement(nr, nb):
    got, want, before, info = run_gpu((nr, nb, 100 + nr, "mixed"), kind="arena" if nr % 2 else "torch")
    D.assert_same_model(got, want, before, f"P={nr}+{nb}")
    if nr + nb > 60:
        assert min(info["sections"]) > 0, info["sections"]              # every section is exercised


@pytest.mark.parametrize("nr,nb,mode", [(0, 300, "mixed"), (300, 0, "mixed"), (150, 150, "none"), (150, 150, "clone"),
                                        (150, 150, "split"), (150, 150, "prune_all"), (0, 70, "prune_all")])
def test_rule_edges_against_the_restatement(nr, nb, mode):
    got, want, before, info = run_gpu((nr, nb, 7, mode))
    D.assert_same_model(got, want, before, f"{mode} {nr}+{nb}")
    kept, clones, children = info["sections"]
    P = nr + nb
    expected = {"none": (None, 0, 0), "clone": (None, P, 0), "split": (0, 0, P), "prune_all": (0, 0, 0)}.get(mode)
    if expected:
        assert (clones, children) == expected[1:] and (expected[0] is None or kept == expected[0]), info["sections"]
    if mode == "prune_all":
        assert got.bg_xyz.shape == (0, 3) and got.xyz_gradient_accum.shape == (nr, 1)
    if mode == "split":                                                  # every ray-bound raw log-scale row was divided
        assert torch.equal(got._scaling.detach().cpu(), before._scaling.detach() / torch.tensor(1.6))


def test_groups_without_optimizer_state():
    got, want, before, _ = run_gpu((100, 90, 5, "mixed"), kind="torch", with_state=False)
    assert not got.optimizer_bg.state and not got.optimizer.state
    for a, _n, _t, _lr in D.RAY + D.BG:
        w, g = getattr(want, a).detach(), getattr(got, a).detach().cpu()
        assert g.shape == w.shape and (torch.equal(g, w) or a in ("bg_xyz", "bg_scaling")), a
    pu.assert_close(got.bg_xyz, want.bg_xyz, "bg_xyz without state")


def test_world_size_term_only_with_max_screen_size():
    key = (40, 50, 9, "ws_row")
    sizes = {}
    for mss in (None, 20):
        got, want, before, _ = run_gpu(key, mss)
        D.assert_same_model(got, want, before, f"max_screen_size {mss}")
        sizes[mss] = D.origins(before, got).tolist()
    planted = 40 + 1
    assert planted in sizes[None] and planted not in sizes[20]
    assert float(before.max_radii2D.min()) > 1.5 * 20                    # and max_radii2D removed nothing in either


def test_binding_refusals():
    t, states, noise = make_inputs(20, 10, 1)
    cases = {"non-fp32": ("bg_scaling", lambda x: x.double()), "non-contiguous": ("_rotation", lambda x: x.t().contiguous().t()),
             "cpu": ("bg_xyz", lambda x: x.cpu())}
    for what, (attr, spoil) in cases.items():
        m = build(t, {}, DEV, torch.optim.Adam)
        setattr(m, attr, spoil(getattr(m, attr).detach()))
        with pytest.raises(_lib.ScgError):
            densify.densify_and_prune(m, MAX_GRAD, MIN_OPACITY, EXTENT, 20, noise=noise.to(DEV))
    m = build(t, states, DEV, torch.optim.Adam)
    with pytest.raises(_lib.ScgError, match="max_grad"):
        densify.densify_and_prune(m, 0.0, MIN_OPACITY, EXTENT, 20)
    with pytest.raises(_lib.ScgError, match="noise"):
        densify.densify_and_prune(m, MAX_GRAD, MIN_OPACITY, EXTENT, 20, noise=noise.to(DEV)[:, :-1])
    m.optimizer_bg.param_groups[0]["params"].append(torch.nn.Parameter(torch.zeros(3, device=DEV)))
    with pytest.raises(_lib.ScgError, match="one per group"):
        densify.densify_and_prune(m, MAX_GRAD, MIN_OPACITY, EXTENT, 20, noise=noise.to(DEV))
    assert m.bg_xyz.shape[0] == 10


def test_default_noise_and_model_cache_release():
    t, states, _ = make_inputs(64, 64, 3, "split")
    t["_opacity"][:], t["bg_opacity"][:] = 1.0, 1.0                      # nothing below min_opacity: every source has two children
    m = build(t, states, DEV, O.ArenaAdam)
    m._scg_model_args = ("stale",)
    torch.manual_seed(5)
    densify.densify_and_prune(m, MAX_GRAD, MIN_OPACITY, EXTENT, None)
    assert "_scg_model_args" not in vars(m) and m.bg_xyz.shape[0] == 2 * 128
    first = m.bg_xyz.detach().clone()
    m = build(t, states, DEV, O.ArenaAdam)
    torch.manual_seed(5)
    densify.densify_and_prune(m, MAX_GRAD, MIN_OPACITY, EXTENT, None)
    assert torch.equal(m.bg_xyz.detach(), first) and bool(torch.isfinite(first).all())
    assert not torch.equal(first[:128], first[128:])                     # the two copies drew different samples


# ---- hand-over to the next step ------------------------------------------------------------------------------------------------
def test_next_arena_adam_step_equals_torch_adam_on_the_restatement():
    key = (120, 100, 21, "mixed")
    t, states, noise = make_inputs(*key)
    got = build(t, states, DEV, O.ArenaAdam)
    gen = torch.Generator().manual_seed(1)

    def grads(model, low_columns_only):
        out = {}
        for a, _n, _tail, _lr in D.RAY + D.BG:
            g = torch.randn(getattr(model, a).shape, generator=gen) * 1e-3
            if low_columns_only and a.endswith("features_rest"):
                g.reshape(g.shape[0], 45)[:, 9:] = 0
            out[a] = g
        return out

    def step(model, gr):
        for a in gr:
            getattr(model, a).grad = gr[a].to(getattr(model, a).device)
        model.optimizer.step()
        model.optimizer_bg.step()

    # a step before the call leaves ArenaAdam with a features_rest watermark (moments live in every column here: 45)
    ref = build(t, states, "cpu", torch.optim.Adam)
    g0 = grads(got, True)
    step(got, g0)
    step(ref, g0)
    for m in (got, ref):                                                  # the same statistics on both sides after that step
        m.xyz_gradient_accum, m.denom = m.xyz_gradient_accum.clone(), m.denom.clone()
    before = build({a: getattr(ref, a).detach() for a in t}, {}, "cpu", torch.optim.Adam)
    for a, n, _tail, _lr in D.RAY + D.BG:                                 # the GPU's step is the state both calls start from
        st = got.group_state(n)
        getattr(ref, a).data.copy_(getattr(got, a).detach().cpu())
        getattr(before, a).data.copy_(getattr(got, a).detach().cpu())
        ref.group_state(n)["exp_avg"].copy_(st["exp_avg"].cpu())
        ref.group_state(n)["exp_avg_sq"].copy_(st["exp_avg_sq"].cpu())
    info = D.densify_and_prune(ref, MAX_GRAD, MIN_OPACITY, EXTENT, 20, noise)
    densify.densify_and_prune(got, MAX_GRAD, MIN_OPACITY, EXTENT, 20, noise=noise.to(DEV))
    D.assert_same_model(got, ref, before, "before the next step")
    assert min(info["sections"]) > 0

    # the next step: torch.optim.Adam on the restatement's result, on the device
    want = build({a: getattr(ref, a).detach() for a in t}, {}, DEV, torch.optim.Adam)
    for a, n, _tail, _lr in D.RAY + D.BG:
        st = ref.group_state(n)
        want.set_state(n, float(st["step"]), st["exp_avg"], st["exp_avg_sq"])
    g1 = grads(got, False)
    step(got, g1)
    step(want, g1)
    dev = got.optimizer_bg._dev[torch.cuda.current_device()]
    (arr, slots, _gis), = dev.tables.values()                             # the cached tables of the old tensors were dropped
    rest = [k for k, (p, _st, row_len) in enumerate(slots) if row_len > 0]
    assert len(rest) == 1 and slots[rest[0]][0] is got.bg_features_rest
    assert arr[rest[0]].flags == _lib.ADAM_FORCE_FULL, "the features_rest watermark was not forced after the densification"
    assert got.optimizer_bg.fallback_steps == 0 and got.optimizer.fallback_steps == 0
    child = torch.zeros(ref.bg_xyz.shape[0], dtype=torch.bool)
    child[ref.bg_xyz.shape[0] - 2 * info["sections"][2]:] = True
    for a, n, _tail, lr in D.RAY + D.BG:
        pa, pb = getattr(got, a).detach(), getattr(want, a).detach()
        assert pa.shape == pb.shape, a
        rows = ~child.to(DEV) if a in ("bg_xyz", "bg_scaling") else slice(None)
        bound = 1e-6 * pb.abs() + 1e-5 * lr                               # the Adam parity bound of tests/test_gpu_optim.py
        assert bool(((pa - pb).abs() <= bound)[rows].all()), (a, float((pa - pb).abs().max()))
        if a in ("bg_xyz", "bg_scaling"):
            pu.assert_close(pa[child], pb[child], f"{a} of the children after the step")
        sa, sb = got.group_state(n), want.group_state(n)
        assert float(sa["step"]) == float(sb["step"]) == 5.0
        for k in ("exp_avg", "exp_avg_sq"):
            assert float((sa[k] - sb[k]).abs().max()) <= 1e-5 * float(sb[k].abs().max()), (a, k)


# ---- determinism -----------------------------------------------------------------------------------------------------------------
def test_two_calls_give_identical_bits():
    t, states, noise = make_inputs(700, 600, 33)
    runs = []
    for _ in range(2):
        m = build(t, states, DEV, O.ArenaAdam)
        densify.densify_and_prune(m, MAX_GRAD, MIN_OPACITY, EXTENT, 20, noise=noise.to(DEV))
        densify.reset_opacity(m)
        runs.append(m)
    a, b = runs
    for attr, n, _tail, _lr in D.RAY + D.BG:
        assert torch.equal(getattr(a, attr).detach(), getattr(b, attr).detach()), attr
        for k in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(a.group_state(n)[k], b.group_state(n)[k]), (attr, k)
    for attr, _tail in D.STATS:
        assert torch.equal(getattr(a, attr), getattr(b, attr)) and not bool(getattr(a, attr).any())
    assert not bool(a.group_state("opacity")["exp_avg"].any()) and not bool(a.group_state("bg_opacity")["exp_avg_sq"].any())

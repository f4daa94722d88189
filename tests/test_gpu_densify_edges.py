"""densify.densify_and_prune / reset_opacity (csrc/densify.hip) alone at their threshold, value and section edges, against the
header's rule in fp64 (tests/densify_refs.py: densify_truth, reset_truth).

A  exact ties and their one-ulp neighbours: hand-made tables, the fp64 truth and the kernel agree everywhere, nothing excluded
B  computed rows (child xyz, child scaling, the divided ray-bound raw scaling) through compare_rows: the class of every element is
   the fp32 restatement's, finite elements lie within max(4 e_ref, 1 fp32 ulp of the row's largest term) of fp64
C  non-finite and extreme rows between finite neighbours, and their isolation: a benign row of the same fate in their place leaves
   every other output bit bit-identical
D  section patterns: origins, copies and moments torch.equal to the restatement
E  reset_opacity alone
The conditions on the inputs (bit patterns of the thresholds, no source within 64 e_ref of a threshold, every edge class present)
are held by tests/test_densify_edges_cpu.py; here a source may be left out of nothing: tests A, C and D assert that their near set
at 16 e_ref is empty and compare everything.  Every comparison prints the kernel's deviation beside e_ref (pytest -s);
profiles/densify_edges_gpu_tests.txt holds one such output."""
import numpy as np
import pytest
import torch

import densify_refs as D
from scgaussian_amd import densify, optim as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
OPTIMIZERS = {"torch": torch.optim.Adam, "arena": O.ArenaAdam}
RAY_ATTRS = [r[0] for r in D.RAY] + [f[0] for f in D.FIXED]
TIES = D.tie_scenes()
PATTERNS = D.section_patterns()
P_ARGS = (D.P_MAX_GRAD, D.P_MIN_OPACITY, D.P_EXTENT)


def kind_of(k):
    """Half the cases on ArenaAdam, half on torch.optim.Adam."""
    return "arena" if k % 2 else "torch"


def run(t, states, noise, args, kind, percent_dense=D.P_PERCENT):
    """(model before on the CPU, model after the kernels, fp64 truth) of one call with the thresholds the binding rounds to fp32."""
    max_grad, min_opacity, extent, mss = args
    truth = D.densify_truth(t, *D.thresholds32(percent_dense, extent, mss, max_grad, min_opacity), noise)
    before = D.make_model(t, states, percent_dense=percent_dense)
    got = D.make_model(t, states, DEV, OPTIMIZERS[kind], percent_dense)
    kept = {a: getattr(got, a) for a in RAY_ATTRS}
    densify.install(got)
    got.densify_and_prune(max_grad, min_opacity, extent, mss, noise=noise.to(DEV))
    for a, x in kept.items():
        assert getattr(got, a) is x, (a, "ray-bound tensors keep their identity")
    return before, got, truth


# ---- A: exact ties ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,name", list(enumerate(TIES)))
def test_exact_ties_and_their_neighbours(k, name):
    sc = TIES[name]
    before, got, truth = run(sc["tensors"], sc["states"], sc["noise"], sc["args"], kind_of(k), sc["percent_dense"])
    table = sc["expect"]
    for what, (plain, children) in (("truth", D.counts_of(truth)), ("kernel", D.counts_in(before, got))):
        bad = np.nonzero((plain != table[0]) | (children != table[1]))[0]
        assert len(bad) == 0, (name, what, "differs from the table at sources", bad, [sc["rows"][i] for i in bad],
                               "kept or cloned", plain[bad], "children", children[bad], "table", table[0][bad], table[1][bad])
    child = D.assert_copied(got, before, truth, name)
    # the computed rows of these scenes hold exact values and infinities: their class and value are the restatement's
    rows = truth["origin"][child]
    if len(rows):
        copy = (np.arange(child.sum()) >= child.sum() // 2).astype(int)
        D.compare_rows(got.bg_xyz.detach().cpu().numpy()[child], truth["child_xyz"][copy, rows], truth["ref32"]["child_xyz"][copy, rows],
                       truth["child_term"][copy, rows], f"{name} child xyz")
        D.compare_rows(got.bg_scaling.detach().cpu().numpy()[child], truth["child_scaling"][rows], truth["ref32"]["child_scaling"][rows],
                       truth["scaling_term"][rows], f"{name} child scaling")


# ---- B: computed rows against fp64 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", list(OPTIMIZERS))
def test_computed_rows_against_fp64(kind):
    t, states, noise, rows = D.split_scene(D.B_SEED)
    before, got, truth = run(t, states, noise, D.B_ARGS, kind)
    P, nr = truth["g"].shape[0], truth["nr"]
    near = D.near_threshold(truth, D.NEAR)
    print("split scene: near set", len(near), "of", P, "e_ref of g / smax / child smax / o", truth["e_ref"])
    assert len(near) <= 0.01 * P
    child = D.assert_copied(got, before, truth, "split scene", skip_sources=near)
    assert child.all() and got.bg_xyz.shape[0] == 2 * P
    far = ~np.isin(np.arange(P), near)                                     # (the near set is empty on the CPUs this was written on)
    xyz = got.bg_xyz.detach().cpu().numpy().reshape(2, P, 3)
    scaling = got.bg_scaling.detach().cpu().numpy().reshape(2, P, 3)
    iso = far & np.isin(np.arange(P), rows["isotropic"])
    small = far & (truth["scaling"].max(axis=1) < -6.0)
    assert iso.sum() > 100 and small.sum() > 50
    for c in (0, 1):
        for what, sel in (("", far), (", near-isotropic sources", iso), (", small sources", small)):
            D.compare_rows(xyz[c][sel], truth["child_xyz"][c][sel], truth["ref32"]["child_xyz"][c][sel], truth["child_term"][c][sel],
                           f"child xyz of copy {c}{what}")
    for what, sel in (("", far), (", small sources", small)):
        D.compare_rows(scaling[0][sel], truth["child_scaling"][sel], truth["ref32"]["child_scaling"][sel], truth["scaling_term"][sel],
                       f"child scaling{what}")
    D.compare_rows(got._scaling.detach().cpu().numpy()[far[:nr]], truth["ray_scaling"][far[:nr]], truth["ref32"]["ray_scaling"][far[:nr]],
                   np.abs(truth["scaling"][:nr]).max(axis=1)[far[:nr]], "divided ray-bound raw scaling")
    # zero noise: both children at the parent's xyz; identity quaternion, scaling 0, dyadic noise: noise + xyz; bit for bit
    z, d = rows["zero_noise"], rows["dyadic"]
    parent = truth["ref32"]["xyz"]
    assert np.array_equal(xyz[0][z], parent[z]) and np.array_equal(xyz[1][z], parent[z]), "zero noise moved a child"
    assert np.array_equal(xyz[:, d], noise.numpy()[:, d] + parent[d][None]), "identity rotation, unit scale: child xyz != noise + xyz"
    # the two children of one parent share every attribute but xyz
    for a in ("bg_features_dc", "bg_features_rest", "bg_opacity", "bg_scaling", "bg_rotation"):
        x = D._bits(getattr(got, a)).reshape(2, P, -1)
        assert np.array_equal(x[0], x[1]), (a, "differs between the two children")
    assert not np.array_equal(xyz[0], xyz[1])


# ---- C: non-finite and extreme rows ----------------------------------------------------------------------------------------------
def test_nonfinite_rows_and_their_isolation():
    t, states, noise, planted = D.nonfinite_scene()
    args = P_ARGS + (20,)
    before, got, truth = run(t, states, noise, args, "arena")
    assert len(D.near_threshold(truth, D.NEAR)) == 0
    # structure and every copied row (the planted NaN bits included) bit for bit
    child = D.assert_copied(got, before, truth, "non-finite scene")
    S = len(truth["parents"])
    rows = truth["origin"][child]
    copy = (np.arange(2 * S) >= S).astype(int)
    xyz, scaling = got.bg_xyz.detach().cpu().numpy()[child], got.bg_scaling.detach().cpu().numpy()[child]
    is_planted = np.isin(rows, list(planted.values()))
    assert is_planted.sum() >= 2 * 10 and (~is_planted).sum() > 20
    for what, sel in (("planted", is_planted), ("finite neighbours", ~is_planted)):
        D.compare_rows(xyz[sel], truth["child_xyz"][copy, rows][sel], truth["ref32"]["child_xyz"][copy, rows][sel],
                       truth["child_term"][copy, rows][sel], f"non-finite scene child xyz, {what}")
        D.compare_rows(scaling[sel], truth["child_scaling"][rows][sel], truth["ref32"]["child_scaling"][rows][sel],
                       truth["scaling_term"][rows][sel], f"non-finite scene child scaling, {what}")
    nr = truth["nr"]
    hit = truth["split"][:nr]
    D.compare_rows(got._scaling.detach().cpu().numpy()[hit], truth["ray_scaling"][hit], truth["ref32"]["ray_scaling"][hit],
                   what="non-finite scene divided ray-bound raw scaling")
    # the same against the restatement's structure
    after = D.make_model(t, states)
    info = D.densify_and_prune(after, *args, noise)
    assert np.array_equal(info["origin"].numpy(), truth["origin"]) and info["sections"] == (len(truth["keep"]), len(truth["clones"]), S)
    assert got.bg_xyz.shape[0] == after.bg_xyz.shape[0]
    # isolation: a benign row of the same fate in place of every planted one; every other output row and moment bit-identical
    t2, s2, n2 = D.benign_twin(truth, planted)
    before2, got2, truth2 = run(t2, s2, n2, args, "arena")
    assert np.array_equal(truth2["origin"], truth["origin"]) and np.array_equal(truth2["split"], truth["split"])
    D.assert_copied(got2, before2, truth2, "benign twin")
    others = ~np.isin(truth["origin"], list(planted.values()))
    for a, n, _tail, _lr in D.BG:
        assert np.array_equal(D._bits(getattr(got, a))[others], D._bits(getattr(got2, a))[others]), (a, "a neighbour of a planted row changed")
        for key in ("exp_avg", "exp_avg_sq"):
            assert np.array_equal(D._bits(got.group_state(n)[key])[others], D._bits(got2.group_state(n)[key])[others]), (n, key)
    ray_others = ~np.isin(np.arange(nr), list(planted.values()))
    assert np.array_equal(D._bits(got._scaling)[ray_others], D._bits(got2._scaling)[ray_others])
    assert bool(torch.isfinite(got2.bg_xyz).all()) and bool(torch.isfinite(got2.bg_scaling).all())


# ---- D: section patterns ---------------------------------------------------------------------------------------------------------
def check_pattern(fates, nr, mss, seed, kind, what):
    t, states, noise = D.plant(fates, nr, seed, state_nan=True)
    args = P_ARGS + (mss,)
    before, got, truth = run(t, states, noise, args, kind)
    assert len(D.near_threshold(truth, D.NEAR)) == 0, what
    want = D.make_model(t, states)
    info = D.densify_and_prune(want, *args, noise)
    assert np.array_equal(info["origin"].numpy(), truth["origin"]), what
    D.assert_same_model(got, want, before, what)                          # origins, copies and moments torch.equal, children close
    D.assert_copied(got, before, truth, what)                             # and bit for bit, the +0 moments and statistics included
    rows = nr + len(truth["origin"])
    for a, tail in D.STATS:
        x = getattr(got, a)
        assert tuple(x.shape) == (rows,) + tail and not bool(x.any()), (what, a)
    if nr:
        st = got.group_state("scaling")
        assert bool(before.group_state("scaling")["exp_avg"].isnan().any())
        assert not bool(st["exp_avg"].any()) and not bool(st["exp_avg_sq"].any()), (what, "ray scaling moments")
    return truth, got


@pytest.mark.parametrize("k,name", list(enumerate(PATTERNS)))
def test_section_patterns(k, name):
    fates, nr, mss = PATTERNS[name]
    truth, got = check_pattern(fates, nr, mss, 7, kind_of(k), name)
    if name == "h_new_set_empty":
        assert got.bg_xyz.shape == (0, 3) and got.xyz_gradient_accum.shape == (nr, 1)
        assert torch.equal(got._scaling.detach().cpu(), D.make_model(*D.plant(fates, nr, 7)[:2])._scaling.detach() / torch.tensor(1.6))


@pytest.mark.parametrize("k,nr", list(enumerate([1, 63, 64, 65, 300])))
def test_set_boundary_with_every_fate_pair(k, nr):
    pairs = [(a, b) for a in D.FATE_NAMES for b in D.FATE_NAMES]
    for j, (first, second) in enumerate(pairs):
        check_pattern(D.boundary_pattern(nr, first, second), nr, 20, 100 + j, kind_of(k + j), f"nr={nr} {first}/{second}")


# ---- E: reset_opacity alone ------------------------------------------------------------------------------------------------------
def reset_case(nr, nb, ray_state, bg_state, kind):
    x = {"_opacity": D.reset_values(nr, 2 * nr + 1), "bg_opacity": D.reset_values(nb, 2 * nb)}
    t, states, _noise = D.plant(["keep"] * (nr + nb), nr, 5)
    t["_opacity"], t["bg_opacity"] = torch.from_numpy(x["_opacity"])[:, None], torch.from_numpy(x["bg_opacity"])[:, None]
    use = {}
    for n, on in (("opacity", ray_state and nr), ("bg_opacity", bg_state and nb)):
        if on:
            m, v = states[n][1].clone(), states[n][2].clone()
            m[0::3], v[0::2] = float("nan"), float("inf")
            m[1::3] = float("-inf")
            use[n] = (3.0, m, v)
    got = D.make_model(t, use, DEV, OPTIMIZERS[kind])
    kept = (got._opacity, got.bg_opacity)
    densify.install(got)
    got.reset_opacity()
    assert got._opacity is kept[0] and got.bg_opacity is kept[1], "both tensors keep their identity"
    what = f"reset {nr}+{nb} {kind} state {bool(ray_state)}/{bool(bg_state)}"
    out = np.concatenate([got._opacity.detach().cpu().numpy()[:, 0], got.bg_opacity.detach().cpu().numpy()[:, 0]])
    xs = np.concatenate([x["_opacity"], x["bg_opacity"]])
    for n in ("opacity", "bg_opacity"):
        st = got.group_state(n) if (n == "opacity" and nr) or (n == "bg_opacity" and nb) else None
        assert (st is not None) == (n in use), (what, n, "optimizer state present")
        if st is not None:
            for key in ("exp_avg", "exp_avg_sq"):
                assert st[key].shape == getattr(got, "_opacity" if n == "opacity" else "bg_opacity").shape
                assert not D._bits(st[key]).any(), (what, n, key, "not +0 after the reset")
    return xs, out, what


_CAPPED = []


def capped_bits():
    """The bits the kernel gives x = +inf: one source, one launch, once."""
    if not _CAPPED:
        t, _states, _noise = D.plant(["keep"], 1, 5)
        t["_opacity"] = torch.tensor([[float("inf")]])
        m = D.make_model(t, {}, DEV)
        densify.install(m)
        m.reset_opacity()
        _CAPPED.append(int(D._bits(m._opacity)[0, 0]))
    return _CAPPED[0]


@pytest.mark.parametrize("k,size", list(enumerate(D.RESET_SIZES)))
def test_reset_opacity_alone(k, size):
    nr, nb = size
    xs, out, what = reset_case(nr, nb, True, True, kind_of(k))
    r64, r32 = D.reset_truth(xs), D.reset_ref32(xs)
    # every x whose sigmoid is clearly above 0.01 (by 100 ulps of 0.01 and more) yields ONE bit pattern, that of x = +inf
    above = xs > D.LOGIT01 + 1e-4
    top = D.reset_ref32(np.float32([np.inf]))
    if above.any():
        pattern = set(D._bits(out[above]).tolist())
        assert pattern == {capped_bits()}, (what, "results above the cap are not the one of x = +inf", sorted(pattern), capped_bits())
        D.compare_rows(out[above][:1, None], D.reset_truth(np.float32([np.inf]))[:, None], top[:, None], what=f"{what}: the capped value")
    with np.errstate(over="ignore"):
        s32 = np.float32(1) / (np.float32(1) + np.exp(-xs))
    sub = (s32 < np.finfo(np.float32).tiny) & ~above
    for name, sel in (("at and below the cap", ~above & ~sub), ("subnormal sigmoid and below", sub)):
        if sel.any():
            D.compare_rows(out[sel][:, None], r64[sel][:, None], r32[sel][:, None], what=f"{what}: {name}")


@pytest.mark.parametrize("nr,nb,ray_state,bg_state,kind", [(70, 60, False, False, "torch"), (70, 60, True, False, "arena"),
                                                          (70, 60, False, True, "torch"), (130, 0, True, False, "arena"),
                                                          (130, 0, False, False, "torch")])
def test_reset_opacity_with_missing_state(nr, nb, ray_state, bg_state, kind):
    xs, out, what = reset_case(nr, nb, ray_state, bg_state, kind)
    D.compare_rows(out[:, None], D.reset_truth(xs)[:, None], D.reset_ref32(xs)[:, None], what=what)

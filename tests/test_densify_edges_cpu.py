"""The conditions on the inputs of tests/test_gpu_densify_edges.py, checked on the reference side alone (tests/densify_refs.py):
the planted thresholds are the intended fp32 bit patterns, no source of a pattern scene sits within 64 e_ref of a threshold (four
times the GPU test's margin of 16: another CPU's fp32 run has another e_ref), the fp32 restatement and the fp64 truth take the same
decisions, every edge class is there, and reset_truth agrees with the restatement and the recorded fixture."""
import numpy as np
import pytest

import densify_refs as D

FX = D.fixture()
TIES = D.tie_scenes()
PATTERNS = D.section_patterns()


def truth_of(t, noise, args, percent_dense=D.P_PERCENT):
    max_grad, min_opacity, extent, mss = args
    return D.densify_truth(t, *D.thresholds32(percent_dense, extent, mss, max_grad, min_opacity), noise)


def restatement(t, states, noise, args, percent_dense=D.P_PERCENT):
    before, after = D.make_model(t, states, percent_dense=percent_dense), D.make_model(t, states, percent_dense=percent_dense)
    info = D.densify_and_prune(after, *args, noise)
    return before, after, info


def assert_clear(truth, what):
    near = D.near_threshold(truth, D.NEAR_CPU)
    assert len(near) == 0, (what, "sources within 64 e_ref of a threshold", near[:8], truth["e_ref"])
    assert truth["agree"], (what, "the fp32 restatement and the fp64 truth decide differently")


# ---- part A ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(TIES))
def test_tie_scenes_pass_the_intended_bit_patterns_and_hold_their_rows(name):
    sc = TIES[name]
    max_grad, min_opacity, extent, mss = sc["args"]
    got = D.thresholds32(sc["percent_dense"], extent, mss, max_grad, min_opacity)
    for g, w in zip(got, sc["thr"]):
        assert (g is None) == (w is None) and (g is None or (g.dtype == np.float32 and g.tobytes() == np.float32(w).tobytes())), (g, w)
    one, half = np.float32(1.0), np.float32(0.5)
    kind, k = name.split("_")[0], name.split("_")[1] if "_" in name else ""
    edge = {"prev": lambda x: np.nextafter(x, np.float32(-np.inf)), "tie": lambda x: x, "next": lambda x: np.nextafter(x, np.float32(np.inf))}
    if kind == "dense":
        assert got[2] == edge[k](one) and (got[2] < one, got[2] == one, got[2] > one) == (k == "prev", k == "tie", k == "next")
    if kind == "big":
        assert (got[3] is None) == name.endswith("None") and (got[3] is None or got[3] == edge[k](one))
        assert np.float32(0.2 * extent) == edge[k](one)
    if kind == "opacity":
        assert got[1] == edge[k](half)
    truth = truth_of(sc["tensors"], sc["noise"], sc["args"], sc["percent_dense"])
    # the planted quantities are exact in every arithmetic: the fp32 run and the fp64 run hold the same numbers
    assert truth["agree"]
    if kind == "grad":
        mg = np.float32(max_grad)
        with np.errstate(divide="ignore", invalid="ignore"):
            vals = {k: np.float32(a) / np.float32(d) for k, (a, d) in sc["grads"].items()}
        assert vals["prev"] == np.nextafter(mg, np.float32(0)) and vals["tie"] == mg and vals["next"] == np.nextafter(mg, np.float32(1))
        assert vals["minus"] == -mg and vals["minus_inf"] == -np.inf and vals["plus_inf"] == np.inf and vals["x_by_minus_zero"] == -np.inf
        assert np.isnan(vals["inf_by_inf"]) and np.isnan(vals["zero_by_zero"])
        assert np.array_equal(truth["g"], truth["ref32"]["g"].astype(np.float64))
    else:
        q, value = {"dense": ("smax", 1.0), "big": ("smax", 1.0), "opacity": ("o", 0.5)}[kind]
        assert (truth[q] == value).all() and (truth["ref32"][q] == np.float32(value)).all(), q
    # the hand-made table and the fp64 truth agree, and so does the restatement
    plain, children = D.counts_of(truth)
    assert np.array_equal(plain, sc["expect"][0]) and np.array_equal(children, sc["expect"][1]), (name, plain, children, sc["expect"])
    before, after, _info = restatement(sc["tensors"], sc["states"], sc["noise"], sc["args"], sc["percent_dense"])
    p2, c2 = D.counts_in(before, after)
    assert np.array_equal(p2, plain) and np.array_equal(c2, children), (name, "restatement", p2, c2)
    for cls, rows in sc["classes"].items():
        assert len(rows) > 0, cls
    wanted = {"dense": {"ray split", "bg split", "ray none", "bg none"} if k == "prev" else {"ray clone", "bg clone", "ray none", "bg none"},
              "big": {"bg pruned", "ray none"} if (k == "prev" and not name.endswith("None")) else {"bg none", "ray none"},
              "opacity": {"bg pruned", "ray pruned", "ray none"} if k == "next" else {"bg none", "bg clone", "ray clone", "ray split",
                                                                                     "bg split", "ray none"},
              "grad": {"ray none", "ray clone", "ray split", "bg none", "bg clone", "bg split"}}[kind]
    assert set(sc["classes"]) == wanted, (name, set(sc["classes"]))


def test_tie_scenes_cover_every_planted_threshold():
    assert {n.split("_mss")[0] for n in TIES} == {f"{q}_{k}" for q in ("dense", "big", "opacity") for k in ("prev", "tie", "next")} | {"grad"}
    assert len(TIES["grad"]["grads"]) == 9 and len(TIES["grad"]["rows"]) == 36


# ---- part B ------------------------------------------------------------------------------------------------------------------
def test_split_scene_is_what_it_claims():
    t, states, noise, rows = D.split_scene(D.B_SEED)
    truth = truth_of(t, noise, D.B_ARGS)
    P = truth["g"].shape[0]
    assert P == 3 * 256 + 1 and truth["split"].all() and not truth["child_gone"].any() and truth["agree"]
    near = D.near_threshold(truth, D.NEAR_CPU)
    print("split scene: near set", len(near), "of", P, "e_ref", truth["e_ref"])
    assert len(near) <= 0.01 * P
    s = truth["scaling"]
    assert s.min() == -12.0 and s.max() == 12.0 and (s.max(axis=1) - s.min(axis=1)).max() > np.log(1e5)
    q = np.concatenate([np.asarray(t["_rotation"]), np.asarray(t["bg_rotation"])]).astype(np.float64)
    norm = np.sqrt((q * q).sum(axis=1))
    assert norm.min() < 1e-2 and norm.max() > 1e2 and norm.min() >= 0.9e-3 and norm.max() <= 1.1e3
    for k in range(4):                                                     # identity and the three 180-degree rotations
        assert ((q != 0).sum(axis=1) == 1)[np.nonzero(q[:, k])[0]].sum() >= 40
    u = np.asarray(noise)
    assert len(rows["zero_noise"]) >= 40 and not u[:, rows["zero_noise"]].any()
    assert (np.abs(u) == 4.0).all(axis=2).any() and len(rows["dyadic"]) >= 20 and len(rows["isotropic"]) >= 100
    assert (rows["zero_noise"] < 300).any() and (rows["zero_noise"] >= 300).any()
    # dyadic rows: noise + xyz is exact in fp32, and the fp64 truth says so
    d = rows["dyadic"]
    want = u[:, d].astype(np.float64) + truth["xyz"][d][None]
    assert np.array_equal(truth["child_xyz"][:, d], want) and np.array_equal(want.astype(np.float32).astype(np.float64), want)
    before, after, info = restatement(t, states, noise, D.B_ARGS)
    assert info["sections"] == (0, 0, P) and np.array_equal(info["origin"].numpy(), truth["origin"])
    # the restatement's children are the fp32 run of the truth's expressions, bit for bit: e_ref is the restatement's own
    assert np.array_equal(D._bits(after.bg_xyz), D._bits(truth["ref32"]["child_xyz"].reshape(-1, 3)))
    assert np.array_equal(D._bits(after.bg_scaling), D._bits(np.concatenate([truth["ref32"]["child_scaling"]] * 2)))


# ---- part C ------------------------------------------------------------------------------------------------------------------
def test_nonfinite_scene_is_clear_and_holds_every_planted_row():
    t, states, noise, planted = D.nonfinite_scene()
    args = (D.P_MAX_GRAD, D.P_MIN_OPACITY, D.P_EXTENT, 20)
    truth = truth_of(t, noise, args)
    assert_clear(truth, "non-finite scene")
    assert len(planted) == 4 * len(D.C_ROWS) and len(set(planted.values())) == len(planted)
    nr = truth["nr"]
    for (name, side, heat), i in planted.items():
        assert (i < nr) == (side == "ray") and (abs(truth["g"][i]) >= D.P_MAX_GRAD) == (heat == "hot"), (name, side, heat)
        sc = truth["scaling"][i]
        if name.startswith("scaling_nan"):
            k = int(name[-1])
            assert np.isnan(sc[k]) and np.isfinite(np.delete(sc, k)).all() and np.isnan(truth["smax"][i])
            assert not truth["clone"][i] and not truth["split"][i]         # a NaN selects nothing
        if name == "scaling_pinf":
            assert truth["smax"][i] == np.inf and truth["split"][i] == (heat == "hot") and truth["gone"][i] and truth["child_gone"][i]
        if name == "scaling_ninf":
            assert truth["smax"][i] == 0.0 and truth["clone"][i] == (heat == "hot")
        if name.startswith("opacity"):
            want = {"opacity_nan": np.nan, "opacity_pinf": 1.0, "opacity_ninf": 0.0}.get(name)
            assert (want is None and 0 < truth["o"][i] < 1e-40 and truth["ref32"]["o"][i] == 0) or \
                np.array_equal(truth["o"][i], want, equal_nan=True)
            assert truth["gone"][i] == (name in ("opacity_ninf", "opacity_m100"))
        if name.startswith(("quat", "noise")):
            assert truth["split"][i] == (heat == "hot") and not truth["child_gone"][i]
            cls = D._class(truth["ref32"]["child_xyz"][:, i])
            if name in ("quat_zero", "quat_1e-30", "quat_nan"):
                assert (cls == 3).all()                                     # 0 / 0 in fp32: the whole rotation is NaN
            if name == "quat_1e-30":
                assert np.isfinite(truth["child_xyz"][:, i]).all()          # fp64 has the range: the class is the fp32 run's
            if name == "noise_nan":
                assert (cls == 3).all()
            if name == "noise_inf":
                assert set(cls.reshape(-1)) <= {1, 2} and {1, 2} <= set(cls.reshape(-1))
    before, after, info = restatement(t, states, noise, args)
    assert np.array_equal(info["origin"].numpy(), truth["origin"]) and min(info["sections"]) > 0
    # the twin: same fates, nothing planted, every other source bit-identical
    t2, _s2, n2 = D.benign_twin(truth, planted)
    twin = truth_of(t2, n2, args)
    assert_clear(twin, "benign twin")
    assert np.array_equal(twin["split"], truth["split"]) and np.array_equal(twin["origin"], truth["origin"])   # the same fates
    others = ~np.isin(np.arange(D.C_P), list(planted.values()))
    for a in t:
        x, y = D._bits(t[a]), D._bits(t2[a])
        if x.shape[0] == D.C_P:
            assert np.array_equal(x[others], y[others]), a
    assert np.isfinite(np.concatenate([np.asarray(v, dtype=np.float64).reshape(-1) for v in t2.values()])).all()


# ---- part D ------------------------------------------------------------------------------------------------------------------
def check_pattern(fates, nr, mss, seed, what):
    t, states, noise = D.plant(fates, nr, seed, state_nan=True)
    args = (D.P_MAX_GRAD, D.P_MIN_OPACITY, D.P_EXTENT, mss)
    truth = truth_of(t, noise, args)
    assert_clear(truth, what)
    got = np.array([D.fate_of(truth, i) for i in range(len(fates))])
    want = np.array(fates)
    if not mss:
        want[want == "split_gone"] = "split"
    assert np.array_equal(got, want), (what, "a planted fate was lost", np.nonzero(got != want)[0][:8])
    return truth


@pytest.mark.parametrize("name", list(PATTERNS))
def test_section_patterns_are_clear_and_hold_their_fates(name):
    fates, nr, mss = PATTERNS[name]
    truth = check_pattern(fates, nr, mss, 7, name)
    P, G, W = len(fates), 256, 64
    keep, clones, parents = truth["keep"], truth["clones"], truth["parents"]
    survivors = np.unique(np.concatenate([keep, clones, parents]))
    if name.startswith("a_"):
        assert len(keep) == 256 and keep.max() == 255 and len(clones) == 0 and len(parents) == 0 and P > 2 * G
    if name.startswith("b_"):
        first = name == "b_only_first_of_each_group"
        want = [s if first else min(s + G, P) - 1 for s in range(0, P, G)]
        assert list(survivors) == want and len(want) == 4 and (np.array(want) < nr).any() and (np.array(want) >= nr).any()
    if name.startswith("c_"):
        w = [set(np.array(fates)[k * W:(k + 1) * W]) for k in range(P // W)]
        assert any(w[k] == {"clone"} and w[k + 1] == {"split"} for k in range(len(w) - 1))
        assert any(w[k] == {"split"} and w[k + 1] == {"clone"} for k in range(len(w) - 1))
        assert nr % W != 0                                                  # and the set boundary inside a wave
    if name == "d_group_clone_group_split":
        assert nr == 0 and np.array_equal(keep[:G], np.arange(G)) and np.array_equal(clones[:G], np.arange(G))
        assert np.array_equal(parents[:G], np.arange(G, 2 * G))
    if name.startswith("f_"):
        assert list(survivors) == [P - 1] and P % G == 1 and list(keep) == [P - 1]
    if name.startswith("g_"):
        groups = set(survivors // G)
        assert P == 65537 and groups == {"g_65537_group0": {0}, "g_65537_group256": {256}, "g_65537_both": {0, 256}}[name]
        assert P - 1 in survivors or 256 not in groups
    if name == "h_children_pruned":
        assert truth["split"].sum() > 0 and len(parents) == 0 and truth["split"][:nr].any() and truth["split"][nr:].any()
        assert len(keep) > 0 and len(clones) > 0
    if name == "h_new_set_empty":
        assert nr > 0 and len(truth["origin"]) == 0 and truth["split"][:nr].all()


@pytest.mark.parametrize("nr", [1, 63, 64, 65, 300])
def test_boundary_patterns_are_clear_and_hold_their_fates(nr):
    for k, (first, second) in enumerate((a, b) for a in D.FATE_NAMES for b in D.FATE_NAMES):
        check_pattern(D.boundary_pattern(nr, first, second), nr, 20, 100 + k, f"nr={nr} {first}/{second}")


def test_restatement_and_truth_agree_on_every_origin_of_a_mixed_pattern():
    fates, nr, mss = PATTERNS["c_wave_clones_then_wave_splits"]
    t, states, noise = D.plant(fates, nr, 7, state_nan=True)
    before, after, info = restatement(t, states, noise, (D.P_MAX_GRAD, D.P_MIN_OPACITY, D.P_EXTENT, mss))
    truth = truth_of(t, noise, (D.P_MAX_GRAD, D.P_MIN_OPACITY, D.P_EXTENT, mss))
    assert np.array_equal(info["origin"].numpy(), truth["origin"])
    child = D.assert_copied(after, before, truth, "restatement")          # the bitwise helper holds the restatement itself
    assert child.sum() == 2 * len(truth["parents"])


# ---- part E ------------------------------------------------------------------------------------------------------------------
def test_reset_truth_against_the_restatement_and_the_fixture():
    before, after = D.load_case(FX, "reset", "in"), D.load_case(FX, "reset", "out")
    for attr in ("_opacity", "bg_opacity"):
        x = getattr(before, attr).detach().numpy()
        D.compare_rows(getattr(after, attr).detach().numpy(), D.reset_truth(x), D.reset_ref32(x), what=f"fixture {attr}")
    m = D.load_case(FX, "reset", "in")
    D.reset_opacity(m)
    assert np.array_equal(D._bits(m._opacity), D._bits(D.reset_ref32(before._opacity.detach().numpy())))


@pytest.mark.parametrize("nr,nb", D.RESET_SIZES)
def test_reset_values_hold_their_classes(nr, nb):
    x = np.concatenate([D.reset_values(nr, 2 * nr + 1), D.reset_values(nb, 2 * nb)])
    r32, r64 = D.reset_ref32(x), D.reset_truth(x)
    with np.errstate(over="ignore"):
        s32 = (np.float32(1) / (np.float32(1) + np.exp(-x.astype(np.float32)))).astype(np.float32)
    if nr + nb >= 64:
        sub = (s32 > 0) & (s32 < np.finfo(np.float32).tiny)
        assert sub.sum() >= 6 and np.isfinite(r32[sub]).all() and (x[sub] >= -88.5).all() and (x[sub] <= -87.4).all()
        over = np.isin(x, np.float32([-100.0, -95.0]))
        assert over.any() and (r32[over] == -np.inf).all() and np.isfinite(r64[over]).all()
        assert np.isnan(r32[np.isnan(x)]).all() and np.isnan(x).any() and (r32[x == -np.inf] == -np.inf).all() and (x == -np.inf).any()
        above = x > D.LOGIT01 + 1e-4
        assert above.sum() >= 5 and len(set(D._bits(r32[above]).tolist())) == 1 and (x == np.inf).any()
        assert np.isin(np.float32([-20.0, 5.0, 100.0]), x).all() and (np.signbit(x) & (x == 0)).any()
        near = np.abs(x - D.LOGIT01) < 0.06
        assert near.sum() >= 40
    # the class of the fp32 restatement never hangs on an ulp of expf: no finite x within 0.2 of -88.72, where expf(-x) overflows
    assert (np.abs(x[np.isfinite(x)] + 88.7228) > 0.2).all()
    assert np.array_equal(np.isnan(r32), np.isnan(r64)) and ((r32 == -np.inf) >= (r64 == -np.inf)).all()


def test_compare_rows_tells_class_and_value_apart():
    a = np.array([[1.0, 2.0, 4.0], [1e-6, 2e-6, np.inf], [np.nan, 1.0, -np.inf]])
    b = a.astype(np.float32)
    D.compare_rows(b, a, b, what="same")
    for bad in (np.nan, np.inf, -np.inf):
        g = b.copy()
        g[0, 1] = bad
        with pytest.raises(AssertionError, match="class"):
            D.compare_rows(g, a, b, what="class")
    g = b.copy()
    g[2, 0] = 1.0                                                         # finite where the restatement has a NaN
    with pytest.raises(AssertionError, match="class"):
        D.compare_rows(g, a, b, what="class")
    g = b.copy()
    g[1, 0] = np.float32(1e-6) * np.float32(1 + 1e-5)                     # 40 ulp of the small row's largest term, far below one of 4.0
    with pytest.raises(AssertionError, match="deviation"):
        D.compare_rows(g, a, b, what="value")
    g[1, 0] = np.nextafter(b[1, 0], np.float32(1))                        # one ulp of the element: within one ulp of the row's term
    D.compare_rows(g, a, b, what="one ulp")

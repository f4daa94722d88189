"""tests/model_refs.py is right, and its bar has teeth, without a GPU: the fp64 composition against autograd through the reference
getters and the oracle, the closed form of the activations' derivatives against the vector-Jacobian product, four wrong closed
forms each caught by loss_refs.held_to on the class built for it, the admission of every value member, and what the layouts
of tests/test_gpu_model_kernel_edges.py cover."""
import numpy as np
import pytest
import torch

import geometry_refs as GR
import loss_refs as LR
import model_refs as MR

F32, F64 = torch.float32, torch.float64
DEG = 2
NR = 170


@pytest.fixture(scope="module")
def pl():
    return MR.pool()


def _class_errors(pl, placement, name, got, labels):
    """{label: (err, e32)} of `got` (all members of the pool in `placement`) for one output."""
    ref = MR.reference(DEG)[placement]
    e = MR.gaussian_error(got, ref["g64"][name], ref["scale"][name])
    return {c: (float(e[torch.from_numpy(labels == c)].max()), float(ref["e32"][name][torch.from_numpy(labels == c)].max()))
            for c in sorted(set(labels))}


def test_fp64_composition_equals_autograd_through_the_getters_and_the_oracle(pl):
    """The pool as one model, every class in either set (NR of its members ray-bound): the oracle's preprocess under autograd
    through the fp32 getters is held to the fp64 composition with e32 taken from the composition at fp32 alone."""
    NP = len(pl)
    idx = torch.tensor(MR.interleaved(pl, MR.CLASSES), dtype=torch.long)
    model = pl.model(idx, NR)
    raw = GR.make_records(NP, seed=5)
    names = MR.raw_names(model)
    g0 = MR.model_backward(model, pl.cam, DEG, pl.mod, raw, F64)
    rowmax = lambda t: t.reshape(t.shape[0], -1).abs().max(1, keepdim=True).values          # noqa: E731
    both = {r: torch.cat([rowmax(g0[r]), rowmax(g0[b])]) for r, b in zip(MR.RAW_RAY, MR.RAW_BG)}
    rec, _ = GR.normalise_records(raw, both, MR.RAW_RAY)
    g64 = MR.model_backward(model, pl.cam, DEG, pl.mod, rec, F64)
    g32 = MR.model_backward(model, pl.cam, DEG, pl.mod, rec, F32)
    o32 = MR.model_backward(model, pl.cam, DEG, pl.mod, rec, F32, stage="oracle")
    assert torch.equal(g64["decisions"][0], o32["decisions"][0]) and torch.equal(g64["decisions"][0], g32["decisions"][0])
    labels = np.array(pl.labels(idx))
    iso = pl.iso()[idx]
    for n in names + ("means2D",):
        sl = slice(NR, NP) if n.startswith("bg_") else slice(0, NR) if n != "means2D" else slice(0, NP)
        scale = torch.where(iso[sl], g64["rot_scale"][sl], g64[n].abs().max(1).values) if n.endswith("rotation") else \
            g64["zval_scale"] if n == "zval" else None
        want = g64[n]
        got_o, got_r = (o32[n], g32[n])
        if n == "means2D":
            want, got_o, got_r = want[sl], got_o[sl], got_r[sl]
        e, e32 = MR.gaussian_error(got_o, want, scale), MR.gaussian_error(got_r, want, scale)
        for c in sorted(set(labels[sl])):
            if c.endswith(":sat") and n.endswith("opacity"):
                continue                                       # (fp64 sees a gradient where fp32 has none: both fp32 runs give exactly 0)
            m = torch.from_numpy(labels[sl] == c)
            LR.held_to(f"model refs oracle chain {c} {n}", float(e[m].max()), float(e32[m].max()), LR.GRAD_FLOOR, elements=int(m.sum()))
    for n in names:                                            # saturated logits: exactly 0 through both fp32 chains
        if n.endswith("opacity"):
            sl = slice(NR, NP) if n.startswith("bg_") else slice(0, NR)
            sat = torch.from_numpy(np.char.find(labels[sl], ":sat") >= 0)
            assert int(sat.sum()) > 0 and float(o32[n][sat].abs().max()) == 0.0 and float(g32[n][sat].abs().max()) == 0.0


def test_closed_form_of_the_activation_derivatives_equals_the_vjp(pl):
    N = len(pl)
    for n_ray in (N, 0, 100):
        model = pl.model(torch.arange(N), n_ray)
        g_act, _ = MR.stage_backward(model, pl.cam, DEG, pl.mod, MR.reference(DEG)["ray"]["rec"], F64)
        a, b = MR.autograd_vjp(model, g_act, F64), MR.explicit_vjp(model, g_act, F64)
        assert set(a) == set(b) == set(MR.raw_names(model))
        for n in a:
            assert bool(torch.isfinite(a[n]).all()), n
            s = a[n].abs().reshape(a[n].shape[0], -1).max(1).values.clamp_min(1e-300)
            if n.endswith("rotation"):                         # (isotropic members: relative to the terms that cancel)
                q = getattr(model, n).double()
                sl = slice(n_ray, N) if n.startswith("bg_") else slice(0, n_ray)
                s = torch.maximum(s, g_act["rotations"][sl].abs().max(1).values / q.norm(dim=1).clamp_min(MR.NORM_EPS))
            assert float(((a[n] - b[n]).abs().reshape(a[n].shape[0], -1).max(1).values / s).max()) < 1e-12, n


@pytest.mark.parametrize("wrong,cls,out", [("no_projection", "value_quat", "rotation"), ("o_for_o1mo", "value_logit", "opacity"),
                                           ("rayo_for_rayd", "value_ray", "zval"), ("clamp_ignored", "value_quat", "rotation")])
def test_a_wrong_activation_derivative_breaks_the_bar_on_the_class_built_for_it(pl, wrong, cls, out):
    N = len(pl)
    labels = np.array(pl.labels(torch.arange(N)))
    model = pl.model(torch.arange(N), N)
    ref = MR.reference(DEG)["ray"]
    g_act, _ = MR.stage_backward(model, pl.cam, DEG, pl.mod, ref["rec"], F64)
    right = _class_errors(pl, "ray", out, MR.explicit_vjp(model, g_act, F64)[out], labels)[cls]
    bad = _class_errors(pl, "ray", out, MR.explicit_vjp(model, g_act, F64, wrong=wrong)[out], labels)[cls]
    LR.held_to(f"model refs closed form {cls} {out}", right[0], right[1], LR.GRAD_FLOOR)
    print(f"wrong {wrong}: {cls} {out} err {bad[0]:.3e} e32 {bad[1]:.3e}")
    assert bad[0] > 100 * max(LR.FACTOR * bad[1], LR.GRAD_FLOOR), (wrong, bad)      # not a near miss
    with pytest.raises(AssertionError):
        LR.held_to(f"model refs WRONG {wrong} {cls} {out}", bad[0], bad[1], LR.GRAD_FLOOR)
    if wrong == "clamp_ignored":                               # the members the variant is about: |q| < 1e-12 and q != 0
        q = pl.t["rotation"].double().norm(dim=1)
        m = (q < MR.NORM_EPS) & (q > 0) & torch.from_numpy(labels == cls)
        assert int(m.sum()) >= 4
        others = torch.from_numpy(labels == cls) & ~m
        e = MR.gaussian_error(MR.explicit_vjp(model, g_act, F64, wrong=wrong)[out], ref["g64"][out], ref["scale"][out])
        assert float(e[m].min()) > 1e-4 and float(e[others].max()) < 1e-12


def test_every_value_member_is_admitted_and_carries_its_edge(pl):
    N = len(pl)
    ok = MR.admitted(pl.model(torch.arange(N), N), pl.cam, pl.mod)
    ok0 = MR.admitted(pl.model(torch.arange(N), 0), pl.cam, pl.mod)
    for c in MR.VALUE_CLASSES:
        m = pl.members(c)
        assert len(m) == GR.PER_CLASS and bool(ok[m].all()) and bool(ok0[m].all()), c
        assert bool((MR.reference(DEG)["ray"]["radii"][m] > 0).all()), c
    assert bool(ok[: len(GR.CLASSES) * GR.PER_CLASS].all())     # the planted members through the raw model, too
    t = pl.t
    lg = t["opacity"][pl.members("value_logit")].reshape(-1)
    assert float(lg.min()) == -200.0 and float(lg.max()) == 30.0 and bool((lg == 0).any())
    assert not bool(((lg > 6) & (lg < 30)).any()) and float(lg[lg > -200].min()) == -5.0
    o = torch.sigmoid(lg)
    assert bool((o[lg == 30] == 1).all()) and bool((o[lg == -200] == 0).all()) and int(((o > 0) & (o < 1)).sum()) == 12
    s = t["scaling"][pl.members("value_scale")]
    spread = s.max(1).values - s.min(1).values
    assert int((spread == 0).sum()) == 8 and int((spread == 10).sum()) == 8
    labels = pl.labels(pl.members("value_scale"))
    assert sorted(set(labels)) == ["value_scale:disc", "value_scale:iso"] and labels.count("value_scale:disc") == 8
    assert not bool(pl.disc()[: len(GR.CLASSES) * GR.PER_CLASS].any())       # no planted member is one
    q = t["rotation"][pl.members("value_quat")].double()
    norms = q.norm(dim=1)
    for want in (1e-3, 1e3, 1e-6, 1e-13, 5e-13, 1e-11):
        assert int(((norms / want - 1).abs() < 1e-5).sum()) == 2, want
    assert int((norms == 0).sum()) == 2 and int((q[:, 0] < -0.2).sum()) >= 2
    r = pl.members("value_ray")
    dn = t["rayd"][r].double().norm(dim=1)
    assert int(((dn - 0.5).abs() < 1e-6).sum()) == 4 and int(((dn - 2).abs() < 1e-6).sum()) == 4
    assert int((t["zval"][r] < 0).sum()) == 4 and int((t["zval"][r] == 0).sum()) == 4
    assert bool((t["rayo"][r].abs().max(1).values > 0).all())
    z0 = r[(t["zval"][r] == 0).reshape(-1)]
    assert torch.equal(t["rayo"][z0], t["xyz"][z0])


def test_the_layouts_put_every_member_in_either_set_and_a_culled_one_at_every_edge(pl):
    culled = set(i for c in GR.CULLED for i in pl.members(c).tolist())
    seen = {"ray": set(), "bg": set()}
    for P, sizes in MR.SIZES.items():
        assert {0, 1, 59, 60, 61, 63, 64, 65, 119, 120, P - 1, P} <= set(sizes) and (121 in sizes) == (P > 121)
        for n_ray in sizes:
            idx = MR.scene_layout(pl, P, n_ray, MR.case_start(P, n_ray)).tolist()
            assert len(idx) == P
            seen["ray"].update(idx[:n_ray])
            seen["bg"].update(idx[n_ray:])
            for part in (idx[:n_ray], idx[n_ray:]):
                edges = {0, len(part) - 1} | {b for k in range(1, len(part) // 60 + 1) for b in (60 * k - 1, 60 * k)}
                assert all(part[e] in culled for e in edges if 0 <= e < len(part)), (P, n_ray)
    value = set(i for c in MR.VALUE_CLASSES for i in pl.members(c).tolist())
    assert value <= seen["ray"] and value <= seen["bg"]
    idx = MR.scene_layout(pl, 181, 61, MR.case_start(181, 61), bg_all_culled_first=True).tolist()
    assert all(i in culled for i in idx[61:121]) and not all(i in culled for i in idx[121:])
    # the sizes put 45 n and 3 n on every remainder mod 4 at a set's end
    ends = {n for P, sizes in MR.SIZES.items() for k in sizes for n in (k, P - k) if n}
    assert {(45 * n) % 4 for n in ends} == {0, 1, 2, 3} and {(3 * n) % 4 for n in ends} == {0, 1, 2, 3}


def test_the_words_the_tail_rule_may_write():
    for n in (1, 59, 60, 61, 121):
        assert bool(MR.rest_words_the_tail_rule_may_write(n, 3).all())                # degree 3: every word is active
        for deg in (1, 2):
            may = MR.rest_words_the_tail_rule_may_write(n, deg)
            active = 3 * ((deg + 1) ** 2 - 1)
            assert bool(may[:, :active].all())                                         # every word that can be non-zero is stored
            assert bool((~may[:, active:]).any())                                      # ... and some tail words are left alone
    may = MR.rest_words_the_tail_rule_may_write(1, 1)                                  # one record, a partial workgroup: 11 float4 + 1 word
    assert may[0].tolist() == [True] * 12 + [False] * 32 + [True]
    may = MR.rest_words_the_tail_rule_may_write(2, 1)                                  # 22 float4 + 2 words; float4 11 = words 44 | 45 46 47
    assert may[0].tolist() == [True] * 12 + [False] * 32 + [True] and may[1].tolist() == [True] * 11 + [False] * 32 + [True] * 2

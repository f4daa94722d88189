"""tests/optim_refs.py earns its place, without a GPU: the numpy restatement of csrc/adam_math.h against torch.optim.Adam and
against the same step in double, the mutants it must tell apart, and the premises of the frames and of the two coefficients that
tests/test_gpu_optim_edges.py relies on."""
import itertools

import numpy as np
import pytest
import torch

import loss_refs
import optim_refs as OR


def _torch_adam(seg, steps):
    """torch.optim.Adam (CPU, default implementation) from seg's state over its first `steps` gradients: (p, m, v)."""
    p = torch.nn.Parameter(torch.from_numpy(seg.p.copy()))
    opt = torch.optim.Adam([p], lr=seg.lr, betas=(seg.b1, seg.b2), eps=seg.eps)
    opt.state[p] = dict(step=torch.tensor(float(seg.step)), exp_avg=torch.from_numpy(seg.m.copy()),
                        exp_avg_sq=torch.from_numpy(seg.v.copy()))
    for k in range(steps):
        p.grad = torch.from_numpy(seg.g[k].copy())
        opt.step()
    st = opt.state[p]
    assert float(st["step"]) == float(seg.step) + steps
    return p.detach().numpy(), st["exp_avg"].numpy(), st["exp_avg_sq"].numpy()


def test_restatement_against_torch_adam_over_30_steps():
    """At the bound tests/test_gpu_optim.py holds the kernel to: 1e-6 |p| + 1e-5 lr, moments at 1e-5 of their maximum.  The count
    of elements whose bits differ from torch's is printed: torch's bits are not the contract (its CPU lerp is fused)."""
    seg = OR.plain_seg(4099, seed=1, launches=30)
    seg.m[:], seg.v[:] = 0, 0
    want = OR.ref_launches([seg], 30)[-1][0]
    p, m, v = _torch_adam(seg, 30)
    print("bits differing from torch CPU after 30 steps (of 4099): m %d v %d p %d"
          % (OR.differing(want.m, m), OR.differing(want.v, v), OR.differing(want.p, p)))
    assert bool((np.abs(want.p - p) <= 1e-6 * np.abs(p) + 1e-5 * seg.lr).all())
    for a, b in ((want.m, m), (want.v, v)):
        assert float(np.abs(a - b).max()) <= 1e-5 * float(np.abs(b).max())


@pytest.mark.parametrize("step", OR.STEPS_IN + (OR.STEP_LATE,))
def test_restatement_against_fp64_step(step):
    """One step from the same fp32 state.  e32 is the error of an independent fp32 evaluation (torch's CPU Adam); margin and floor
    are loss_refs.held_to's (4 * e32, GRAD_FLOOR of the largest value)."""
    seg = OR.plain_seg(4099, seed=2 + int(step), launches=1, step=step, lr=OR.LRS[int(step) % 6])
    r64 = OR.adam_step_f64(seg.p, seg.m, seg.v, seg.g[0], seg.step, seg.lr, seg.b1, seg.b2, seg.eps)
    got = OR.adam_step_ref(seg.p, seg.m, seg.v, seg.g[0], seg.step, seg.lr, seg.b1, seg.b2, seg.eps)
    t32 = _torch_adam(seg, 1)
    for name, g, r, t in zip("pmv", got, r64, t32):
        floor = loss_refs.GRAD_FLOOR * float(np.abs(r).max())
        loss_refs.held_to(f"adam restatement step {step:g} {name}", float(np.abs(g - r).max()), float(np.abs(t - r).max()),
                          floor, r.size)


def _edge_frames():
    """Every frame of tests/test_gpu_optim_edges.py that is a Seg: (name, [Seg], launches)."""
    out = []
    for off in OR.PLAIN_OFFSETS:
        out += [(s.name, [s], 3) for s in OR.plain_frames(off)]
    out += [(s.name, [s], 2) for s in OR.arith_frames()]
    for rows in OR.ROW_COUNTS:
        out += [(s.name, [s], 4) for s in OR.row_frames(rows)]
    out += [(s.name, [s], 4) for s in OR.row_frames(92, off=(4, 4, 4, 4))]
    out += [(s.name, [s], 4) for s in OR.other_row_frames()]
    out += [(s.name, [s], 3) for s, _w in OR.moving_frames().values()]
    out.append(("sixteen segments", OR.sixteen_frame(), 3))
    return out


def _differs(a, b):
    for la, lb in zip(a, b):
        for x, y in zip(la, lb):
            if not (OR.same_bits(x.p, y.p) and OR.same_bits(x.m, y.m) and OR.same_bits(x.v, y.v) and x.live == y.live):
                return True
    return False


def test_every_mutant_is_exposed_and_every_frame_exposes_one():
    """The proof that a bit-level comparison on these frames fails on a subtly wrong kernel.  Prints, per mutant, the first frame on
    which it changes a bit of p, m, v or the watermark (and on how many frames it does)."""
    frames = _edge_frames()
    hits = {mu: [] for mu in OR.MUTANTS + OR.LIVE_MUTANTS}
    blind = []
    for name, segs, k in frames:
        want = OR.ref_launches(segs, k)
        seen = False
        for mu in hits:
            if mu in OR.LIVE_MUTANTS and not any(s.row_len for s in segs):
                continue
            if _differs(OR.ref_launches(segs, k, mutant=mu), want):
                hits[mu].append(name)
                seen = True
        if not seen:
            blind.append(name)
    for mu, names in hits.items():
        print(f"MUTANT {mu}: exposed by {len(names)} of {len(frames)} frames, first: {names[0] if names else None}")
    assert not [mu for mu, names in hits.items() if not names], hits
    assert not blind, blind
    # what each part of the GPU suite is there for
    arith = {s.name for s in OR.arith_frames()}
    for mu in ("eps_omitted", "eps_under_root", "eps_before_div", "denormals_flushed"):
        assert arith & set(hits[mu]), mu
    for mu in ("bc2_not_rooted", "step_not_incremented"):                      # bias corrections that are 1 to a few digits
        assert [n for n in hits[mu] if n.startswith("arith") and "step=199" in n], mu


def test_coefficient_premise():
    """The host's double pow (the restatement) and the device's may differ in the last places: moving either result by up to 2 ulp
    must leave bc2s and nss unchanged as fp32, for every (b1, b2, lr, step) a GPU test uses, and for the reference's six learning
    rates at steps 1..199."""
    nudges = [n for n in itertools.product(range(-2, 3), repeat=2) if n != (0, 0)]
    steps = sorted({s + k for s in OR.STEPS_IN + (OR.STEP_LATE,) for k in range(OR.STEPS_AHEAD)})
    cases = [(b, lr, s) for b in OR.BETAS for lr in OR.LRS for s in steps]
    cases += [((0.9, 0.999), lr, s) for lr in OR.LRS_REFERENCE for s in range(0, 199)]
    sensitive = []
    for (b1, b2), lr, s in cases:
        base = OR.bias_coefs(s, lr, b1, b2)
        assert np.isfinite(base[0]) and np.isfinite(base[1]) and base[0] > 0 and base[1] < 0
        if any(OR.bits(np.array(OR.bias_coefs(s, lr, b1, b2, nudge=n)))[i] != OR.bits(np.array(base))[i]
               for n in nudges for i in (0, 1)):
            sensitive.append((b1, b2, lr, s))
    print(f"coefficient premise: {len(sensitive)} of {len(cases)} sensitive")
    assert not sensitive, sensitive


def test_frame_premises_watermark():
    """Row frames with a watermark inside the row and rows enough for every column phase: a float4 group has columns on both sides
    of `live`, a group wraps a row end; multi-workgroup frames have a row across element 4096."""
    checked = 0
    for rows in OR.ROW_COUNTS:
        for s in OR.row_frames(rows):
            pr = OR.row_premises(s.numel, s.row_len, s.w)
            assert OR.live_after(s.m, s.v, s.row_len) == s.w, s.name
            assert all(not g[(np.arange(s.numel) % s.row_len) >= s.w].any() for g in s.g), s.name
            if s.w >= 2 and rows >= 8:
                assert (np.abs(s.m[s.m != 0]) < OR.TINY).any() and (np.abs(s.m) >= OR.TINY).any(), s.name   # denormal and normal
            if s.w:                                                     # the watermark rests on denormals that stay denormal
                st = OR.ref_launches([s], 4)
                want = [x[0].live for x in st]
                flushed = [x[0].live for x in OR.ref_launches([s], 4, mutant="denormals_flushed")]
                assert want == [s.w] * 4 and flushed == [s.w - 1] * 2 + [s.w] * 2, (s.name, want, flushed)
                edge = (np.arange(s.numel) % s.row_len) == s.w - 1          # launch 3: the last live column decays, its gradient zero
                assert not s.g[3][edge].any() and (np.abs(st[2][0].m[edge]) >= OR.TINY).all()
                assert (OR.bits(st[3][0].m[edge]) != OR.bits(st[2][0].m[edge])).all(), s.name
            if rows >= 4 and 0 < s.w < s.row_len:
                assert pr["straddles_live"] and pr["wraps_row"], (s.name, pr)
                checked += 1
            assert pr["row_crosses_chunk"] == (rows >= 92), (s.name, pr)
    assert checked == 3 * 7
    for s in OR.other_row_frames():
        pr = OR.row_premises(s.numel, s.row_len, s.w)
        assert OR.live_after(s.m, s.v, s.row_len) == s.w, s.name
        assert s.numel > OR.CHUNK and pr["row_crosses_chunk"] == (OR.CHUNK % s.row_len != 0), (s.name, pr)
        if s.row_len % 4:
            assert pr["wraps_row"], s.name
        if 0 < s.w < s.row_len and s.row_len not in (4,):
            assert pr["straddles_live"], (s.name, pr)
    assert 4097 > OR.CHUNK and 1 < 4 and 3 < 4 and 48 % 4 == 0 and 4 % 4 == 0          # longer than a chunk, shorter than a group, multiples
    # the sixteen-segment frame's row segments and the moving frames
    rowsegs = [s for s in OR.sixteen_frame() if s.row_len]
    assert len({s.row_len for s in rowsegs}) == 2 and len({s.w for s in rowsegs}) == 2
    for s in rowsegs:
        pr = OR.row_premises(s.numel, s.row_len, s.w)
        assert pr["straddles_live"] and pr["row_crosses_chunk"], (s.name, pr)


def test_frame_premises_moving():
    fr = OR.moving_frames()
    for name, (s, want) in fr.items():
        st = OR.ref_launches([s], 3)
        assert [x[0].live for x in st][:2] == [OR.MOVE_W, want], (name, [x[0].live for x in st])
    # -0.0 beyond the watermark: the restatement's bits are those of +0.0 gradients, p included
    s, _ = fr["minus_zero_beyond"]
    assert np.signbit(s.g[1][s.g[1] == 0]).any()
    plus = OR.row_seg(OR.MOVE_ROWS, 45, OR.MOVE_W, seed=4242, launches=3)
    a, b = OR.ref_launches([s], 3)[-1][0], OR.ref_launches([plus], 3)[-1][0]
    assert OR.same_bits(a.p, b.p) and OR.same_bits(a.m, b.m) and OR.same_bits(a.v, b.v)
    # NaN moments count as non-zero
    s, _ = fr["nan_and_inf_beyond"]
    after = OR.ref_launches([s], 2)[-1][0]
    assert np.isnan(after.m[50 * 45 + 20]) and np.isinf(after.v[91 * 45 + 30]) and after.m[91 * 45 + 30] == -np.inf


def test_frame_premises_poison_and_denormals():
    """The arithmetic frames contain what they claim."""
    w2 = np.float32(1.0 - 0.999)
    for s in OR.arith_frames():
        assert s.numel == OR.CHUNK + 5
        g, m, v = s.g[0], s.m, s.v
        for x in OR.G_VALUES:
            sel = np.isnan(g) if np.isnan(x) else (g == x) & (np.signbit(g) == np.signbit(x))
            for mv in OR.M_VALUES:
                for vv in OR.V_VALUES:
                    assert (sel & (OR.bits(m) == OR.bits(mv)) & (OR.bits(v) == OR.bits(vv))).any(), (s.name, x, mv, vv)
        with np.errstate(all="ignore"):
            gg = (w2 * g) * g
            assert ((gg == 0) & (g != 0)).any()                               # g*g underflows while g does not
            fin = np.isfinite(g)
            assert (np.isinf(g * g) & np.isfinite(gg) & fin).any()            # g*g alone overflows, (w2*g)*g does not: 3e19
            assert (np.isinf(gg) & fin).any()                                 # (w2*g)*g overflows: 1e21
            w1g = np.float32(0.1) * g
            assert ((w1g != 0) & (np.abs(w1g) < OR.TINY)).any()               # a denormal first moment from a normal-or-not g
        st = OR.ref_launches([s], 1)[0][0]
        assert ((st.v != 0) & (st.v < OR.TINY)).any() and ((st.m != 0) & (np.abs(st.m) < OR.TINY)).any()   # denormal v and m AFTER the step
        assert (OR.bits(s.p) == 0).any() and (OR.bits(s.p) == 0x80000000).any()                             # +0 and -0 parameters
    assert np.float32(1e-38) < OR.TINY and np.float32(1e-38) != 0

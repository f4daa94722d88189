"""scgaussian_amd.init_stage at its launch, flush, segment and rule edges.

Bars.  Against a record of the reference (tests/golden/ref_init_edges.npz) or the fp64 CPU loop of tests/init_refs.py:
err <= max(4 * e32, floor) (init_refs.held -> loss_refs.held_to), e32 = the reference's fp32 record (or the fp32 CPU loop) against
the fp64 one, floors as in tests/test_gpu_init_stage.py: 2e-5 * max(1, max|ref|) for values, 1e-4 * max|g| for the gradient.
Against torch.optim.Adam: parameters 1e-6 |p| + 1e-5 lr element-wise, moments 1e-5 of their maximum (test b there).  Everything
about launch lengths and the best-state rule is exact.

    (1) scenes C (unequal views) and D (42 small segments) against the reference's records
    (2) arenas of 2, 64, 126, 128 and 130 elements inside sentinel-filled buffers, against the fp64 loop
    (3) a pair with no match at all (M = 0), in the middle of the arena and at its end
    (4) run(n) == n x run(1) bitwise around the 64-row flush; 4 097 iterations in two launches; the step limit
    (5) the `<` of the best-state rule at a tie and one ulp either side, at iterations 0, 1 and 2
    (6) Adam at steps 2 000 and 4 096 against torch.optim.Adam
    (7) the loss term at hand-made values: sign(0), Z + 1e-8 == 0, a masked-out match with a non-finite term
"""
import numpy as np
import pytest
import torch

import init_refs as ir

pytestmark = pytest.mark.gpu
DEV = "cuda"
STATE = ("z", "exp_avg", "exp_avg_sq", "best_z", "min_loss")
SENTINEL = -777.25


@pytest.fixture(scope="module")
def fx():
    return ir.fixture()


@pytest.fixture(scope="module")
def fe():
    return ir.fixture_edges()


def _from(vg, **kw):
    from scgaussian_amd.init_stage import InitStage
    return InitStage.from_view_gs(vg, **kw)


def _stage(fixture, tag, **kw):
    vg = ir.load_scene(fixture, tag, device=DEV)
    return _from(vg, **kw), vg


def _state(st):
    return {name: getattr(st, name).clone() for name in STATE}


def _same_state(st, ref, what=""):
    for name in STATE:
        mine, other = getattr(st, name), (ref[name] if isinstance(ref, dict) else getattr(ref, name))
        assert torch.equal(mine, other), (what, name, int((mine != other).sum()))


def _row_sums(st):
    """loss_scale * (each row of partials() added up in double): the scalar of every iteration."""
    return st.loss_scale * st.partials().double().sum(dim=1).numpy()


# ------------------------------------------------------------------------------------------------- (1) the recorded edge scenes

@pytest.mark.parametrize("tag", ["C", "D"])
def test_1_edge_scenes_against_the_reference_records(fe, tag):
    rec = lambda what, got, key, grad=False: ir.held(f"{tag} {what}", got, fe[f"{tag}_f64_{key}"], fe[f"{tag}_f32_{key}"], grad)  # noqa: E731
    iters, halve_at = int(fe[f"{tag}_iters"]), tuple(int(h) for h in fe[f"{tag}_halve_at"])
    st, _ = _stage(fe, tag)
    assert st.N == int(fe[f"{tag}_counts"].sum()) and [m for *_x, m in st.segments] == list(fe[f"{tag}_counts"])
    loss_state, grad, partials = st.evaluate()
    rec("it0 scalar", np.array(st.loss_scale * float(partials.cpu().double().sum())), "it0_loss")
    rec("it0 loss_state", loss_state, "it0_loss_state")
    rec("it0 grad", grad, "it0_grad", grad=True)
    assert torch.equal(grad.cpu() == 0, torch.from_numpy(fe[f"{tag}_f64_it0_grad"] == 0))
    for n in (1, 2):
        st.run(1)
        for name, key in (("z", "z"), ("best_z", "best"), ("min_loss", "min")):
            rec(f"after {n} {key}", getattr(st, name), f"after{n}_{key}")
    st, _ = _stage(fe, tag)
    st.run_schedule(iters, halve_at=halve_at)
    assert st.iteration == iters == 12 and len(st._partials) == 1 + len(halve_at)
    for name, key in (("z", "z"), ("best_z", "best"), ("min_loss", "min")):
        rec(f"final {key}", getattr(st, name), f"final_{key}")
    rec("losses", st.losses(), "losses")
    rec("row sums", _row_sums(st), "losses")
    assert st.partials().shape == (12, (st.N + 63) // 64)


# ------------------------------------------------------------------------------------------------- (2) small and ragged arenas

def _cut_pair(fx, M, dtype, device):
    """Views 1 and 2 of scene A with M matches of their 257: the first M - 1 and the next one that is valid, so the arena's last
    element (which the tail lanes of the last wave repeat) has a weight.  The depths move as they do in scene A (Adam with
    eps = 1e-15 does not feel the weights' scale): the generator's distances to the sign steps carry over."""
    full = ir.load_scene(fx, "A", device=device, dtype=dtype)
    ab, ba = full["view1"]["match_infos"]["view2"], full["view2"]["match_infos"]["view1"]
    valid = ((ab["blender_mask"] * ba["blender_mask"]) > 0).cpu()
    last = next(i for i in range(M - 1, 257) if bool(valid[i]))
    idx = torch.tensor(list(range(M - 1)) + [last], device=device)
    vg = {k: {**{f: full[k][f] for f in ("width", "height", "intr", "w2c")}, "match_infos": {}} for k in ("view1", "view2")}
    for a, b, mi in (("view1", "view2", ab), ("view2", "view1", ba)):
        cut = {k: v.detach()[idx].clone() for k, v in mi.items()}
        cut["z_val"].requires_grad_(True)
        vg[a]["match_infos"][b] = cut
    return vg


def _cpu_loop(fx, M, dtype, iters):
    vg = _cut_pair(fx, M, dtype, "cpu")
    loss, state = ir.matchloss_from_base(vg)
    (5 * loss).backward()
    out = {"scalar": np.array(5 * float(loss.detach())), "loss_state": ir.flat(vg, state),
           "grad": ir.flat(vg, {a: {b: mi["z_val"].grad for b, mi in v["match_infos"].items()} for a, v in vg.items()})}
    vg = _cut_pair(fx, M, dtype, "cpu")
    run = ir.torch_init_loop(vg, iters)
    out.update(z=ir.flat(vg, ir.z_of(vg)), best_z=ir.flat(vg, run["best"]), min_loss=ir.flat(vg, run["min_loss"]),
               losses=np.array([float(v) for v in run["losses"]]))
    return out


@pytest.mark.parametrize("M", [1, 32, 63, 64, 65])
def test_2_small_and_ragged_arenas_inside_sentinel_buffers(fx, M):
    r64, r32 = _cpu_loop(fx, M, torch.float64, 3), _cpu_loop(fx, M, torch.float32, 3)
    st = _from(_cut_pair(fx, M, torch.float32, DEV))
    N, pad = 2 * M, 130
    assert st.N == N and float(st.wgt[N - 1]) > 0
    bufs = {}
    for name in STATE + ("loss_state", "grad"):
        bufs[name] = torch.full((N + pad,), SENTINEL, dtype=torch.float32, device=DEV)
        if name in STATE:
            bufs[name][:N] = getattr(st, name)
            setattr(st, name, bufs[name][:N])
    W = (N + 63) // 64
    partials = torch.full((2, W), SENTINEL, dtype=torch.float32, device=DEV)
    st._launch(st.z, 0, 0, 0.0, st.loss_scale, bufs["loss_state"][:N], bufs["grad"][:N], partials[:1])
    torch.cuda.synchronize()
    held = lambda what, got, key, grad=False: ir.held(f"M={M} {what}", got, r64[key], r32[key], grad)      # noqa: E731
    held("it0 scalar", np.array(st.loss_scale * float(partials[0].cpu().double().sum())), "scalar")
    held("it0 loss_state", bufs["loss_state"][:N], "loss_state")
    held("it0 grad", bufs["grad"][:N], "grad", grad=True)
    assert bool((partials[1] == SENTINEL).all())
    st.run(3)
    torch.cuda.synchronize()
    for name in ("z", "best_z", "min_loss"):
        held(f"after 3 {name}", getattr(st, name), name)
    held("losses", st.losses(), "losses")
    held("row sums", _row_sums(st), "losses")
    assert st.partials().shape == (3, W)
    for name, buf in bufs.items():
        assert bool((buf[N:] == SENTINEL).all()), (name, "written past the arena's end")
        assert bool((buf[:N] != SENTINEL).all()), name


# ------------------------------------------------------------------------------------------------- (3) a pair with M = 0

@pytest.mark.parametrize("where", ["middle", "last"])
def test_3_a_pair_with_zero_matches(fx, where):
    ref, _ = _stage(fx, "A")
    base = ir.load_scene(fx, "A", device=DEV)
    empty = lambda: {"uv": torch.zeros(0, 2, device=DEV), "rays_o": torch.zeros(0, 3, device=DEV),                # noqa: E731
                     "rays_d": torch.zeros(0, 3, device=DEV), "cam_rays_d": torch.zeros(0, 3, device=DEV),
                     "blender_mask": torch.zeros(0, device=DEV), "z_val": torch.zeros(0, 1, device=DEV)}
    view3 = {**{f: base["view0"][f] for f in ("width", "height", "intr", "w2c")}, "match_infos": {"view1": empty()}}
    order = ["view0", "view3", "view1", "view2"] if where == "middle" else ["view0", "view1", "view2", "view3"]
    vg = {k: (view3 if k == "view3" else base[k]) for k in order}
    vg["view1"]["match_infos"]["view3"] = empty()
    st = _from(vg)
    assert st.empty_pairs == ([("view3", "view1"), ("view1", "view3")] if where == "middle" else [("view1", "view3"), ("view3", "view1")])
    assert st.N == ref.N == 646 and len(st.segments) == 8 and [m for *_x, m in st.segments].count(0) == 2
    if where == "last":
        assert st.segments[-1] == ("view3", "view1", 646, 0)
    else:
        assert st.segments[2] == ("view3", "view1", 66, 0) and st.segments[3][2] == 66      # shares its offset with the next one
    ref.run(6)
    st.run(6)
    torch.cuda.synchronize()
    assert bool(torch.isnan(st.losses()).all()) and st.losses().shape == (6,) and bool(torch.isfinite(ref.losses()).all())
    at = {(a, b): (off, M) for a, b, off, M in ref.segments}
    for a, b, off, M in st.segments:
        if M == 0:
            continue
        roff, rM = at[a, b]
        assert rM == M
        for name in STATE:
            assert torch.equal(getattr(st, name)[off:off + M], getattr(ref, name)[roff:roff + M]), (a, b, name)
    assert torch.equal(st.partials(), ref.partials())


# ------------------------------------------------------------------------------------------------- (4) launch length

LENGTHS = (63, 64, 65, 127, 128, 129)


@pytest.fixture(scope="module")
def single_steps(fx):
    """Scene A through 129 launches of one iteration: the five state arrays after each length of interest, all partial sums and
    scalars; then 65 more single iterations from the state after 64 at half the learning rate."""
    st, _ = _stage(fx, "A")
    snaps = {}
    for k in range(1, 130):
        st.run(1)
        if k in LENGTHS:
            snaps[k] = _state(st)
    halved, _ = _stage(fx, "A")
    for name in STATE:
        getattr(halved, name).copy_(snaps[64][name])
    halved.iteration, halved.lr = 64, 0.25
    for _k in range(65):
        halved.run(1)
    torch.cuda.synchronize()
    assert st.partials().shape == (129, 11)
    return dict(snaps=snaps, partials=st.partials(), losses=st.losses(), halved=_state(halved), halved_partials=halved.partials())


@pytest.mark.parametrize("n", LENGTHS)
def test_4a_one_launch_of_n_equals_n_launches_of_one(fx, single_steps, n):
    st, _ = _stage(fx, "A")
    st.run(n)
    torch.cuda.synchronize()
    assert st.iteration == n and len(st._partials) == 1
    _same_state(st, single_steps["snaps"][n], n)
    assert st.partials().shape == (n, 11) and torch.equal(st.partials(), single_steps["partials"][:n])
    assert torch.equal(st.losses(), single_steps["losses"][:n])


def test_4b_launches_that_start_off_the_tile_and_change_the_learning_rate(fx, single_steps):
    st, _ = _stage(fx, "A")                                                # first_iter = 5: rows are addressed by k, not by iteration
    st.run(5)
    st.run(124)
    torch.cuda.synchronize()
    _same_state(st, single_steps["snaps"][129], "5 + 124")
    assert torch.equal(st.partials(), single_steps["partials"]) and torch.equal(st.losses(), single_steps["losses"])
    st, _ = _stage(fx, "A")                                                # the learning rate halved before iteration 64
    st.run_schedule(129, halve_at=(64,))
    torch.cuda.synchronize()
    assert st.lr == 0.25 and [p.shape[0] for p in st._partials] == [64, 65]
    _same_state(st, single_steps["halved"], "64 + 65 at half the rate")
    assert torch.equal(st.partials()[:64], single_steps["partials"][:64])
    assert torch.equal(st.partials()[64:], single_steps["halved_partials"])
    assert not torch.equal(st.z, single_steps["snaps"][129]["z"])         # the rate matters
    st, _ = _stage(fx, "A", record_losses=False)                          # the kernel without the partial sums
    st.run(129)
    torch.cuda.synchronize()
    _same_state(st, single_steps["snaps"][129], "record_losses=False")


@pytest.mark.parametrize("n", [64, 65])
def test_4c_a_launch_writes_its_n_rows_of_partial_sums_and_no_other(fx, single_steps, n):
    st, _ = _stage(fx, "A")
    partials = torch.full((n + 1, 11), float("nan"), dtype=torch.float32, device=DEV)
    st._launch(st.z, 0, n, st.lr, st.loss_scale, None, None, partials)
    torch.cuda.synchronize()
    assert not bool(torch.isnan(partials[:n]).any()) and bool(torch.isnan(partials[n]).all())
    assert torch.equal(partials[:n].cpu(), single_steps["partials"][:n])


def test_4d_4097_iterations_are_two_launches(fe):
    from scgaussian_amd import init_stage as IS
    assert IS.MAX_STEPS == 4096
    st, _ = _stage(fe, "D")
    st.run(4097)
    one, _ = _stage(fe, "D")
    for _k in range(4097):
        one.run(1)
    torch.cuda.synchronize()
    assert st.iteration == one.iteration == 4097 and [tuple(p.shape) for p in st._partials] == [(4096, 2), (1, 2)]
    _same_state(st, one, "4097")
    single = torch.cat(one._partials).cpu()
    assert single.shape == (4097, 2) and torch.equal(st.partials(), single)
    one._partials = [torch.cat(one._partials)]
    assert torch.equal(st.losses(), one.losses()) and bool(torch.isfinite(st.losses()).all())


def test_4e_a_launch_past_the_step_limit_is_refused(fe):
    from scgaussian_amd._lib import ScgError
    st, _ = _stage(fe, "D")
    st.run(2)
    torch.cuda.synchronize()
    before = _state(st)
    with pytest.raises(ScgError, match="n_steps"):
        st._launch(st.z, st.iteration, 4097, st.lr, st.loss_scale, None, None, None)
    torch.cuda.synchronize()
    _same_state(st, before, "refused launch")
    assert st.iteration == 2


def test_4f_what_the_partial_sums_held_before_a_launch_changes_no_bit(fx):
    """InitStage takes its partial sums, and evaluate() its loss_state and gradient, from torch.empty: under the two fills of
    tests/guarded_alloc.py those buffers start as NaN and as 0.0115.  One stage per path of the kernel — the evaluation alone
    (n_steps = 0), a launch across the 64-row flush with the loss rows recorded, one that ends off the tile, and the same launches
    without a partials buffer — must leave the same bits in the state, in every row of partial sums and in evaluate()'s outputs as
    with buffers that start from whatever the allocator held."""
    import guarded_alloc as G

    def path(record):
        st, _ = _stage(fx, "A", record_losses=record)
        first = [t.clone() for t in st.evaluate()]
        st.run(65)
        st.lr *= 0.5
        st.run(3)
        torch.cuda.synchronize()
        out = dict(_state(st), it0_loss_state=first[0], it0_grad=first[1], it0_partials=first[2])
        if record:
            out.update(partials=st.partials(), losses=st.losses())
        return {k: v.cpu() for k, v in out.items()}

    for record in (True, False):
        runs = {}
        for fill in (G.FILL_A, G.FILL_B):
            with G.guarded(fill) as reg:
                runs[fill] = path(record)
                assert any(a.module == "scgaussian_amd.init_stage" for a in reg.allocations)      # the stage's own torch.empty calls
            assert reg.check() == []
        plain = path(record)
        for k in plain:
            assert G.same_bits(runs[G.FILL_A][k], runs[G.FILL_B][k]) and G.same_bits(runs[G.FILL_A][k], plain[k]), (record, k)
        assert not record or (plain["partials"].shape == (68, 11) and bool(torch.isfinite(plain["partials"]).all()))


# ------------------------------------------------------------------------------------------------- (5) the best-state rule

@pytest.mark.parametrize("iteration", [0, 1, 2])
def test_5_best_state_rule_at_a_tie_and_one_ulp_either_side(fx, iteration):
    probe, _ = _stage(fx, "A")
    ml = probe.evaluate()[0]
    finite = torch.isfinite(ml)
    assert int(finite.sum()) == probe.N                                   # scene A has no non-finite term at its start
    down, up = torch.full_like(ml, float("-inf")), torch.full_like(ml, float("inf"))
    presets = {"tie": ml.clone(), "below": torch.nextafter(ml, down), "above": torch.nextafter(ml, up)}
    assert bool((presets["below"] < ml).all()) and bool((presets["above"] > ml).all())
    if iteration == 2:
        presets["nan"] = torch.full_like(ml, float("nan"))
    for kind, preset in presets.items():
        st, _ = _stage(fx, "A")
        st.iteration = iteration
        st.best_z.fill_(SENTINEL)
        st.min_loss.copy_(preset)
        z0 = st.z.clone()
        st.run(1)
        torch.cuda.synchronize()
        assert bool((st.z != z0)[st.wgt > 0].all())                       # the step itself was taken
        if iteration == 0:                                                # min_loss and best_z are not read
            assert torch.equal(st.best_z, st.z) and torch.equal(st.min_loss, ml), kind
            continue
        kept = kind == "below"                                            # min_loss < ml: the old state stays
        assert torch.equal(st.min_loss, preset if kept else ml), (iteration, kind)
        want = torch.full_like(z0, SENTINEL) if (kept or iteration == 1) else z0
        assert torch.equal(st.best_z, want), (iteration, kind, int((st.best_z != want).sum()))


# ------------------------------------------------------------------------------------------------- (6) Adam far from step 1

def _adam_step(z, grad, m, v, step):
    p = torch.nn.Parameter(z.clone())
    opt = torch.optim.Adam([p], lr=0.5, eps=1e-15)
    opt.state[p] = {"step": torch.tensor(float(step)), "exp_avg": m.clone(), "exp_avg_sq": v.clone()}
    p.grad = grad.clone()
    opt.step()
    assert float(opt.state[p]["step"]) == step + 1
    return p.detach(), opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"]


def _held_to_adam(st, ref, what):
    p, m, v = ref
    bound = 1e-6 * p.abs() + 1e-5 * 0.5
    assert bool(((st.z - p).abs() <= bound).all()), (what, float((st.z - p).abs().max()))
    for mine, other, key in ((st.exp_avg, m, "exp_avg"), (st.exp_avg_sq, v, "exp_avg_sq")):
        assert float((mine - other).abs().max()) <= 1e-5 * float(other.abs().max()), (what, key)


@pytest.mark.parametrize("iteration", [1999, 4095])
def test_6a_one_step_at_a_late_iteration_is_torch_adam(fx, iteration):
    st, _ = _stage(fx, "A")
    st.run(3)                                                              # moments of a short earlier run
    st.iteration = iteration
    _, grad, _ = st.evaluate()
    z0, m0, v0 = st.z.clone(), st.exp_avg.clone(), st.exp_avg_sq.clone()
    ref = _adam_step(z0, grad, m0, v0, iteration)
    st.run(1)
    torch.cuda.synchronize()
    assert st.iteration == iteration + 1 and bool((st.z != z0).any())
    _held_to_adam(st, ref, iteration)
    # the bias corrections matter at this bar: the step count the moments' own age would give (4) is far outside it
    early = _adam_step(z0, grad, m0, v0, 3)[0]
    assert float((early - ref[0]).abs().max()) > 100 * (1e-6 * float(ref[0].abs().max()) + 1e-5 * 0.5)


def test_6b_the_last_entry_of_the_coefficient_table(fx):
    """Iteration 4095 reached INSIDE run(4096): entry 4095 of the table in LDS.  The state before it is that of run(4095), which
    test 4 holds bitwise to the same iterations of the longer launch."""
    head, _ = _stage(fx, "A", record_losses=False)
    head.run(4095)
    _, grad, _ = head.evaluate()
    ref = _adam_step(head.z, grad, head.exp_avg, head.exp_avg_sq, 4095)
    st, _ = _stage(fx, "A", record_losses=False)
    st.run(4096)
    torch.cuda.synchronize()
    assert st.iteration == 4096
    _held_to_adam(st, ref, "entry 4095")
    head.run(1)                                                            # and the split 4095 + 1 is the same launch, bitwise
    torch.cuda.synchronize()
    _same_state(st, head, "4095 + 1")


# ------------------------------------------------------------------------------------------------- (7) hand-made values

F_, CX, CY, WIDTH, HEIGHT = 8.0, 4.0, 2.0, 128, 64          # powers of two: every product below is exact in fp32
Z_NEG = -float(np.float32(1e-8))                           # Z + 1e-8f == 0 in fp32


def _hand_scene(dtype, device, with_masked=True):
    """Two views with identity w2c and K = [[f,0,cx],[0,f,cy],[0,0,1]]; rays along +z from integer origins.  Segment
    view0 -> view1, match by match (projected pixel (px, py), target (u, v)):
        0  o = (1, 2, 0), z = 4: (6, 6) against (6, 3)   px == u, py != v: the y part of the gradient only
        1  the same against (6, 6)                        both equal: term and gradient exactly 0
        2  o = (1, 2, -4), z = 4: Z == 0, valid          inv = 1 / 1e-8f
        3  o = (3, 1, 0), z = 2: (16, 6) against (9, 11) an ordinary match (four valid matches: weight 1/4)
        4  o = (1, 2, 0), z = -1e-8f: Z + 1e-8f == 0     masked out; its term is not finite
    view1 -> view0 holds ordinary matches."""
    t = lambda rows: torch.tensor(rows, dtype=torch.float64).to(dtype).to(device)          # noqa: E731
    n = 5 if with_masked else 4
    K = t([[F_, 0, CX], [0, F_, CY], [0, 0, 1]])
    eye = torch.eye(4, dtype=dtype, device=device)
    d = t([[0, 0, 1]] * n)
    ab = dict(uv=t([[1, 1]] * n), rays_o=t([[1, 2, 0], [1, 2, 0], [1, 2, -4], [3, 1, 0], [1, 2, 0]][:n]), rays_d=d, cam_rays_d=d,
              blender_mask=t([1, 1, 1, 1, 0][:n]), z_val=t([[4], [4], [4], [2], [Z_NEG]][:n]).requires_grad_(True))
    ba = dict(uv=t([[6, 3], [6, 6], [5, 7], [9, 11], [2, 2]][:n]), rays_o=t([[2, 1, 0], [1, 1, 0], [0, 3, 0], [2, 2, 0], [1, 0, 0]][:n]),
              rays_d=d, cam_rays_d=d, blender_mask=t([1] * n), z_val=t([[2], [4], [8], [2], [4]][:n]).requires_grad_(True))
    return {"view0": {"width": WIDTH, "height": HEIGHT, "intr": K, "w2c": eye, "match_infos": {"view1": ab}},
            "view1": {"width": WIDTH, "height": HEIGHT, "intr": K, "w2c": eye, "match_infos": {"view0": ba}}}


def _hand_reference(dtype):
    vg = _hand_scene(dtype, "cpu")
    loss, state = ir.matchloss_from_base(vg)
    (5 * loss).backward()
    return ir.flat(vg, state), ir.flat(vg, {a: {b: mi["z_val"].grad for b, mi in v["match_infos"].items()} for a, v in vg.items()})


def test_7_the_term_at_hand_made_values():
    ml64, g64 = _hand_reference(torch.float64)
    ml32, g32 = _hand_reference(torch.float32)
    st = _from(_hand_scene(torch.float32, DEV))
    assert st.N == 10 and st.empty_pairs == [] and torch.equal(st.wgt.cpu(), torch.tensor([.25, .25, .25, .25, 0] * 2))
    loss_state, grad, partials = st.evaluate()
    ml, g = loss_state.cpu(), grad.cpu()
    ok = torch.ones(10, dtype=torch.bool)
    ok[4] = False                                                         # the masked-out match: below
    for what, got, r64, r32 in (("term", ml, ml64, ml32), ("gradient", g, g64, g32)):
        err, e32 = (got.double() - r64).abs(), (r32.double() - r64).abs()
        bar = torch.maximum(4 * e32, 2e-5 * r64.abs().clamp_min(1.0))
        print(f"CENSUS init hand-made {what}: worst err / bar {float((err / bar)[ok].max()):.3e}, e32 {e32[ok].tolist()}")
        assert bool((err <= bar)[ok].all()), (what, err.tolist(), bar.tolist())
    # 0: ex == 0 contributes nothing, although d px / d z = (4 - 6) / 4 is not zero: 5 * 1/4 * ((2 - 6) / 4) * (0.5 / 64)
    assert float(ml[0]) == 3 * 0.5 / HEIGHT and float(g[0]) == 5 * 0.25 * -1.0 * 0.5 / HEIGHT
    # 1: both equal
    assert float(ml[1]) == 0.0 and float(g[1]) == 0.0
    # 2: Z == 0: X = 8, Y = 16 over 1e-8f, large but relative to its own size (held above); the gradient is finite
    assert float(ml64[2]) > 1e6 and abs(float(g64[2])) > 1e13 and bool(torch.isfinite(ml[2])) and bool(torch.isfinite(g[2]))
    # 4: masked out
    assert float(g[4]) == 0.0 and not bool(torch.isfinite(ml32[4])) and not bool(torch.isfinite(ml[4]))
    assert bool(torch.isnan(ml[4])) == bool(torch.isnan(ml32[4]))
    without = _from(_hand_scene(torch.float32, DEV, with_masked=False))
    _, _, partials_without = without.evaluate()
    assert partials.shape == (1,) and bool(torch.isfinite(partials).all()) and torch.equal(partials, partials_without)
    # a run over it: the non-finite term stays with its own match
    z0 = st.z.clone()
    st.run(2)
    torch.cuda.synchronize()
    assert float(st.z[4]) == float(z0[4]) and float(st.z[1]) == float(z0[1]) and bool(torch.isfinite(st.z).all())
    assert bool(torch.isfinite(st.partials()).all()) and bool(torch.isfinite(st.losses()).all())

"""scgaussian_amd.init_stage on the GPU against the records of the reference's own init stage (tests/golden/ref_init.npz).

Bars.  Against the fp64 record:  err <= max(4 * e32, floor)  (tests/loss_refs.py held_to), e32 = the reference's own fp32 record
against its fp64 one, err and e32 maxima over the array; floor = 2e-5 * max(1, max|ref|) for values (scalars, loss_state, z, best,
min_loss) and 1e-4 * max|g| for the gradient: the floors of tests/test_match_loss.py.  Against torch.optim.Adam: the bars
tests/test_gpu_optim.py holds ArenaAdam to (parameters 1e-6 |p| + 1e-5 lr element-wise, moments 1e-5 of their maximum).

    (a) evaluate mode at iteration 0                 (b) one run step against torch.optim.Adam fed the kernel's gradient
    (c) run(12) == 12 x run(1), bitwise              (d) the 40-iteration trajectory, and the states after 1 and 2 iterations
    (e) a pair without a valid match                 (f) match_loss_from_base + torch.optim.Adam in the reference's loop shape
    (g) a NaN depth
"""
import numpy as np
import pytest
import torch

import init_refs as ir
import loss_refs as lr

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def fx():
    return ir.fixture()


def _stage(fx, tag="A", **kw):
    from scgaussian_amd.init_stage import InitStage
    vg = ir.load_scene(fx, tag, device=DEV)
    return InitStage.from_view_gs(vg, **kw), vg


def _held(fx, what, got, key, grad=False):
    """max|got - fp64 record| <= max(4 * e32, floor)."""
    r64 = np.asarray(fx[f"A_f64_{key}"], dtype=np.float64)
    r32 = np.asarray(fx[f"A_f32_{key}"], dtype=np.float64)
    got = np.asarray(got.detach().cpu() if torch.is_tensor(got) else got, dtype=np.float64)
    assert got.shape == r64.shape, (what, got.shape, r64.shape)
    scale = float(np.abs(r64).max())
    floor = ir.GRAD_FLOOR * scale if grad else ir.FLOOR * max(1.0, scale)
    lr.held_to(f"init {what}", float(np.abs(got - r64).max()), float(np.abs(r32 - r64).max()), floor, r64.size)


def _adam_bound(p_ref, lr_):
    return 1e-6 * p_ref.abs() + 1e-5 * lr_


def test_a_evaluate_mode_against_the_reference_at_iteration_0(fx):
    st, _vg = _stage(fx)
    z0 = st.z.clone()
    loss_state, grad, partials = st.evaluate()
    torch.cuda.synchronize()
    assert torch.equal(st.z, z0) and not st.exp_avg.any() and not st.best_z.any() and st.iteration == 0     # no state changed
    scalar = st.loss_scale * float(partials.cpu().double().sum())
    _held(fx, "it0 scalar", np.array(scalar), "it0_loss")
    _held(fx, "it0 loss_state", loss_state, "it0_loss_state")
    _held(fx, "it0 grad", grad, "it0_grad", grad=True)
    assert torch.equal(grad.cpu() == 0, torch.from_numpy(fx["A_f64_it0_grad"] == 0))         # masked-out matches: exactly zero
    # the autograd form: 5 * matchloss, backward into the z_val leaves of view_gs
    from scgaussian_amd.init_stage import match_loss_from_base
    vg = ir.load_scene(fx, "A", device=DEV)
    loss, state = match_loss_from_base(vg, st)
    (5 * loss).backward()
    _held(fx, "it0 scalar (autograd)", np.array(5 * float(loss.detach())), "it0_loss")
    assert torch.equal(ir.flat(vg, state), loss_state)
    g = ir.flat(vg, {a: {b: vg[a]["match_infos"][b]["z_val"].grad for b in vg[a]["match_infos"]} for a in vg})
    assert torch.equal(g, grad)
    assert state["view0"]["view2"].shape == (65,) and vg["view0"]["match_infos"]["view2"]["z_val"].grad.shape == (65, 1)
    # ... and without a packed stage
    vg2 = ir.load_scene(fx, "A", device=DEV)
    loss2, _ = match_loss_from_base(vg2)
    assert float(loss2) == float(loss)


def test_b_one_run_step_is_torch_adam_on_the_kernels_own_gradient(fx):
    st, _vg = _stage(fx)
    _, grad, _ = st.evaluate()
    p = torch.nn.Parameter(st.z.clone())
    opt = torch.optim.Adam([p], lr=0.5, eps=1e-15)
    for step in range(3):                                                  # steps 1..3: the bias corrections move
        p.grad = grad.clone()
        opt.step()
        st.run(1)
        torch.cuda.synchronize()
        assert bool(((st.z - p.detach()).abs() <= _adam_bound(p.detach(), 0.5)).all()), (step, float((st.z - p.detach()).abs().max()))
        for mine, key in ((st.exp_avg, "exp_avg"), (st.exp_avg_sq, "exp_avg_sq")):
            ref = opt.state[p][key]
            assert float((mine - ref).abs().max()) <= 1e-5 * float(ref.abs().max()), (step, key)
        with torch.no_grad():                                              # the next step starts from the same point
            p.copy_(st.z)
            opt.state[p]["exp_avg"].copy_(st.exp_avg)
            opt.state[p]["exp_avg_sq"].copy_(st.exp_avg_sq)
        _, grad, _ = st.evaluate()
    assert st.iteration == 3


def test_c_one_launch_of_12_equals_12_launches_of_1_bitwise(fx):
    a, _ = _stage(fx)
    b, _ = _stage(fx)
    a.run(5)
    a.lr *= 0.5
    a.run(7)
    for k in range(12):
        if k == 5:
            b.lr *= 0.5
        b.run(1)
    torch.cuda.synchronize()
    for name in ("z", "exp_avg", "exp_avg_sq", "best_z", "min_loss"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    assert torch.equal(a.partials(), b.partials()) and a.partials().shape == (12, 11)
    assert torch.equal(a.losses(), b.losses()) and a.iteration == b.iteration == 12
    # without the partial sums: the same state
    c, _ = _stage(fx, record_losses=False)
    c.run(5)
    c.lr *= 0.5
    c.run(7)
    torch.cuda.synchronize()
    for name in ("z", "exp_avg", "exp_avg_sq", "best_z", "min_loss"):
        assert torch.equal(getattr(a, name), getattr(c, name)), name


def test_d_trajectory_against_the_reference_run(fx):
    st, vg = _stage(fx)
    st.run(1)
    torch.cuda.synchronize()
    for name, key in (("z", "z"), ("best_z", "best"), ("min_loss", "min")):
        _held(fx, f"after 1 {key}", getattr(st, name), f"after1_{key}")
    assert torch.equal(st.best_z, st.z)                                    # the aliasing quirk: best follows the first step
    z1 = st.z.clone()
    st.run(1)
    torch.cuda.synchronize()
    for name, key in (("z", "z"), ("best_z", "best"), ("min_loss", "min")):
        _held(fx, f"after 2 {key}", getattr(st, name), f"after2_{key}")
    assert torch.equal(st.best_z, z1)
    # a fresh stage through the whole schedule: 4 launches
    st, vg = _stage(fx)
    st.run_schedule(40, halve_at=(10, 20, 30))
    torch.cuda.synchronize()
    assert st.iteration == 40 and st.lr == 0.0625 and len(st._partials) == 4
    _held(fx, "losses", st.losses(), "losses")
    for name, key in (("z", "z"), ("best_z", "best"), ("min_loss", "min")):
        _held(fx, f"final {key}", getattr(st, name), f"final_{key}")
    assert bool((st.best_z != st.z).any())                                 # some match was better earlier than at the end
    best, mins = st.best_state_dict(), st.min_loss_state()
    assert best["view1"]["view2"].shape == (257, 1) and mins["view1"]["view2"].shape == (257,)
    st.load_best(vg)
    _held(fx, "loaded z", ir.flat(vg, {a: {b: vg[a]["match_infos"][b]["z_val"] for b in vg[a]["match_infos"]} for a in vg}),
          "loaded_z")


def test_e_a_pair_without_a_valid_match(fx):
    from scgaussian_amd.init_stage import InitStage, match_loss_from_base
    st, vg = _stage(fx, "B")
    z0 = st.z.clone()
    loss_state, grad, _ = st.evaluate()
    assert not grad.any() and bool(torch.isfinite(loss_state).all())
    np.testing.assert_allclose(loss_state.cpu().numpy(), fx["B_f64_it0_loss_state"], rtol=0, atol=ir.FLOOR * max(1.0, float(fx["B_f64_it0_loss_state"].max())))
    loss, _ = match_loss_from_base(vg, st)
    assert bool(torch.isnan(loss))
    st.run(3)
    torch.cuda.synchronize()
    assert torch.equal(st.z, z0) and bool(torch.isnan(st.losses()).all()) and st.losses().shape == (3,)
    assert torch.equal(st.z.cpu(), torch.from_numpy(fx["B_f32_final_z"]))
    assert torch.equal(st.min_loss, loss_state)                            # every iteration saw the same terms
    # the other pairs of a scene are unaffected: scene A with the masks of (view0, view2) zeroed, against scene A itself
    ref, _ = _stage(fx)
    vg = ir.load_scene(fx, "A", device=DEV)
    vg["view0"]["match_infos"]["view2"]["blender_mask"].zero_()
    cut = InitStage.from_view_gs(vg)
    assert cut.empty_pairs == [("view0", "view2"), ("view2", "view0")]
    ref.run(6)
    cut.run(6)
    torch.cuda.synchronize()
    assert bool(torch.isnan(cut.losses()).all()) and bool(torch.isfinite(ref.losses()).all())
    for a, b, off, M in cut.segments:
        for name in ("z", "exp_avg", "exp_avg_sq", "best_z", "min_loss"):
            mine, other = getattr(cut, name)[off:off + M], getattr(ref, name)[off:off + M]
            if (a, b) in cut.empty_pairs:
                if name == "z":
                    assert torch.equal(mine, torch.from_numpy(fx[f"A_in_{a[4:]}{b[4:]}_z_val"]).reshape(-1).to(DEV))
                elif name in ("exp_avg", "exp_avg_sq"):
                    assert not mine.any()
            else:
                assert torch.equal(mine, other), (a, b, name)


def test_f_match_loss_from_base_with_torch_adam_in_the_reference_loop(fx):
    from scgaussian_amd.init_stage import InitStage, match_loss_from_base
    st, _ = _stage(fx)
    st.run(5)
    st.lr *= 0.5
    st.run(7)
    vg = ir.load_scene(fx, "A", device=DEV)
    loop_stage = InitStage.from_view_gs(vg, record_losses=False)
    loop_stage.install(vg)                                                 # the z_val leaves are the arena's views
    out = ir.torch_init_loop(vg, 12, halve_at=(5,), loss_fn=lambda v: match_loss_from_base(v, loop_stage))
    torch.cuda.synchronize()
    z = loop_stage.z
    assert bool(((st.z - z).abs() <= _adam_bound(z, 0.5)).all()), float((st.z - z).abs().max())
    best, mins = ir.flat(vg, out["best"]), ir.flat(vg, out["min_loss"])
    assert bool(((st.best_z - best).abs() <= _adam_bound(best, 0.5)).all())
    assert bool(((st.min_loss - mins).abs() <= ir.FLOOR * mins.abs().clamp_min(1.0)).all())
    opt = out["optimizer"]
    m = torch.cat([opt.state[p]["exp_avg"].reshape(-1) for g in opt.param_groups for p in g["params"]])
    v = torch.cat([opt.state[p]["exp_avg_sq"].reshape(-1) for g in opt.param_groups for p in g["params"]])
    assert float((st.exp_avg - m).abs().max()) <= 1e-5 * float(m.abs().max())
    assert float((st.exp_avg_sq - v).abs().max()) <= 1e-5 * float(v.abs().max())
    losses = torch.stack(out["losses"]).cpu()
    assert float((st.losses() - losses).abs().max()) <= ir.FLOOR * max(1.0, float(losses.abs().max()))


def test_g_a_nan_depth_stays_with_its_own_match(fx):
    ref, _ = _stage(fx)
    st, _ = _stage(fx)
    hit = 389 + 70                                                         # a valid match of (view2, view1), second wave of the pair
    assert float(st.wgt[hit]) > 0
    ref.run(2)
    st.run(2)
    st.z[hit] = float("nan")
    ref.run(4)
    st.run(4)
    torch.cuda.synchronize()
    assert bool(torch.isnan(st.z[hit])) and bool(torch.isnan(st.min_loss[hit])) and bool(torch.isnan(st.best_z[hit]))
    keep = torch.ones(st.N, dtype=torch.bool, device=DEV)
    keep[hit] = False
    for name in ("z", "exp_avg", "exp_avg_sq", "best_z", "min_loss"):
        assert torch.equal(getattr(st, name)[keep], getattr(ref, name)[keep]), name
        assert bool(torch.isfinite(getattr(st, name)[keep]).all()), name

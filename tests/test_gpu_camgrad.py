"""The camera gradients on the GPU (libscg_camgrad.so, scgaussian_amd/camera_grad.py, pose.py).

1  the public routes: GaussianRasterizer, the K-view rasterizer and render.render on the model path return viewmatrix.grad,
   projmatrix.grad and campos.grad, and they are the CPU oracle's autograd gradients at the bar every parameter gradient is held to;
2  the kernel alone on planted records against the fp64 restatement of its rule (tests/camgrad_refs.py), within
   max(4 e_ref, 1 ulp of the sum's scale): e_ref is what the fp32 oracle's autograd, the first fp32 evaluation of the same rule,
   deviates from fp64 on the same case and output tensor (largest entry); the scale of an entry is the sum of the magnitudes of the
   terms that are added up to form it (camgrad_refs.camera_rule, per_gaussian="scale": per Gaussian, and for campos — a small
   remainder of larger products per Gaussian — of those products), one ulp of it (2^-23) what one rounding of such a sum may cost;
3  the translation identity, which needs no oracle: the sum over Gaussians of the existing backward's dL/dmeans3D is a contraction of
   the three camera gradients — it holds the chain restated in camgrad.hip to geometry_backward_one;
4  bit-exactness and robustness: two runs, fresh and reused partials, a side stream, a captured graph, no host read, and the
   default path's bits with and without the camera's requires_grad;
5  pose recovery: examples/fit_pose.py's loop driven by the oracle on the CPU and by the kernels.
"""
import functools
import types

import numpy as np
import pytest
import torch

import camgrad_refs as CR
import geometry_refs as G
import parity_utils as pu
from scgaussian_amd import camera_grad
from scgaussian_amd import model_path as mp
from scgaussian_amd import rasterizer as R
from scgaussian_amd import render as rmod
from scgaussian_amd import synthetic as syn

pytestmark = pytest.mark.gpu
DEV = "cuda"
W, H, P, DEG, BG = 64, 48, 600, 3, (0.1, 0.2, 0.3)
NAMES7 = ("means3D", "opacities", "shs", "colors_precomp", "scales", "rotations", "cov3D_precomp")
CAMS = ((-25.0, 12.0, 6.0), (8.0, -4.0, 7.0), (15.0, 6.0, 7.5))


@functools.lru_cache(maxsize=None)
def _scene():
    return syn.make_scene(P, W, H, seed=4, log_scale_mean=-3.0)


def _cam(k):
    return syn.orbit_camera(W, H, *CAMS[k])


def _upstream(k):
    return syn.make_upstream_grads(W, H, seed=60 + k)


@functools.lru_cache(maxsize=None)
def _oracle(k):
    """(35 camera gradients, records, radii) of view k of the small scene through the CPU oracle: computed once, never changed."""
    sc = _scene()
    return CR.oracle_rasterize_camera_grads(G.mode_inputs(sc, _cam(k), DEG, 1.0, "sh_sr"), _cam(k), DEG, 1.0, _upstream(k), BG)


def _with_leaves(cam, deg, bg, mod=1.0):
    st = pu.hip_settings(cam, deg, bg, mod)
    leaves = [t.detach().clone().requires_grad_(True) for t in (st.viewmatrix, st.projmatrix, st.campos)]
    return st._replace(viewmatrix=leaves[0], projmatrix=leaves[1], campos=leaves[2]), leaves


def _loss(out, k):
    c, _r, d, a = out
    u = [t.to(DEV) for t in _upstream(k)]
    return (c * u[0]).sum() + (d * u[1]).sum() + (a * u[2]).sum()


def _check(leaves, want35, what):
    for t, w, name in zip(leaves, CR.split(want35), ("viewmatrix", "projmatrix", "campos")):
        assert isinstance(t.grad, torch.Tensor), (what, name, "no gradient")
        assert t.grad.shape == t.shape and t.grad.dtype == t.dtype and t.grad.device == t.device
        print(what, name, "max|got - oracle| / max|oracle| =", pu.nrm_err(t.grad, torch.from_numpy(np.ascontiguousarray(w))))
        pu.assert_close(t.grad, torch.from_numpy(np.ascontiguousarray(w)).float(), (*what, name))
    got = torch.cat([t.grad.reshape(-1) for t in leaves]).cpu().numpy()
    assert not got[CR.DEAD].any(), (what, "a dead entry is not an exact zero")


def _gaussian_leaves(sc):
    return {n: getattr(sc, n).detach().to(DEV).requires_grad_(True) for n in ("means3D", "opacities", "shs", "scales", "rotations")}


# ---- 1: the public routes ----------------------------------------------------------------------------------------------------------
def test_rasterizer_returns_the_oracles_camera_gradients():
    want, _rec, radii = _oracle(0)
    st, leaves = _with_leaves(_cam(0), DEG, BG)
    g = _gaussian_leaves(_scene())
    out = R.GaussianRasterizer(st)(means2D=torch.zeros(P, 3, device=DEV, requires_grad=True), **g)
    assert torch.equal(out[1].cpu(), radii)
    _loss(out, 0).backward()
    torch.cuda.synchronize()
    _check(leaves, want, ("GaussianRasterizer",))
    assert all(t.grad is not None for t in g.values())
    # a second step of the same camera (the one-call path, its records a raw pointer into the workspace): the same gradients
    for t in leaves:
        t.grad = None
    _loss(R.GaussianRasterizer(st)(means2D=torch.zeros(P, 3, device=DEV, requires_grad=True), **g), 0).backward()
    _check(leaves, want, ("GaussianRasterizer", "second step"))


def test_views_rasterizer_returns_per_view_camera_gradients():
    pairs = [_with_leaves(_cam(k), DEG, BG) for k in range(3)]
    g = _gaussian_leaves(_scene())
    outs = R.GaussianRasterizerViews([st for st, _ in pairs])(means2D=torch.zeros(3, P, 3, device=DEV, requires_grad=True), **g)
    sum(_loss(o, k) for k, o in enumerate(outs)).backward()
    torch.cuda.synchronize()
    for k, (_st, leaves) in enumerate(pairs):
        _check(leaves, _oracle(k)[0], ("GaussianRasterizerViews", k))
    # a view that does not reach the loss gets no gradient; only campos of view 1 asked for: the other two stay None
    pairs = [_with_leaves(_cam(k), DEG, BG) for k in range(2)]
    st1 = pairs[1][0]._replace(viewmatrix=pairs[1][1][0].detach(), projmatrix=pairs[1][1][1].detach())
    outs = R.GaussianRasterizerViews([pairs[0][0], st1])(means2D=torch.zeros(2, P, 3, device=DEV, requires_grad=True), **g)
    _loss(outs[1], 1).backward()
    assert all(t.grad is None for t in pairs[0][1])
    pu.assert_close(pairs[1][1][2].grad, torch.from_numpy(_oracle(1)[0][32:].copy()).float(), ("views", "campos alone"))


def _raw_model(ray_fraction=0.6, n=None):
    """The raw model of the small scene, or of its first n Gaussians."""
    sc = _scene() if n is None else syn.Scene(*[t[:n].contiguous() for t in _scene()])
    model = syn.make_raw_model(sc, ray_fraction=ray_fraction, seed=7)
    model.active_sh_degree = DEG
    md = model.to(DEV)
    md.requires_grad_()
    md.active_sh_degree = DEG
    return model, md


def _activated_inputs(model, md):
    act = mp.activate(**mp.tensors_of(md))
    return dict(means3D=act[0].cpu(), opacities=act[1].cpu(), shs=model.get_features.detach(), scales=act[2].cpu(), rotations=act[3].cpu())


def _camera_object(cam, leaves):
    return types.SimpleNamespace(image_height=cam.image_height, image_width=cam.image_width, FoVx=cam.FoVx, FoVy=cam.FoVy,
                                 world_view_transform=leaves[0], full_proj_transform=leaves[1], camera_center=leaves[2])


def test_render_on_the_model_path_returns_the_oracles_camera_gradients():
    model, md = _raw_model()
    cam = _cam(0)
    want, _rec, radii = CR.oracle_rasterize_camera_grads(_activated_inputs(model, md), cam, DEG, 1.0, _upstream(0), BG)
    _st, leaves = _with_leaves(cam, DEG, BG)
    assert rmod.model_fast_path_available(md, rmod.PipelineParams())
    out = rmod.render(_camera_object(cam, leaves), md, rmod.PipelineParams(), torch.tensor(BG, device=DEV))
    assert torch.equal(out["radii"].cpu(), radii)
    _loss((out["render"], None, out["rendered_depth"], out["rendered_alpha"]), 0).backward()
    torch.cuda.synchronize()
    _check(leaves, want, ("render.render", "model path"))
    assert md.zval.grad is not None and md.bg_xyz.grad is not None


# ---- 2: the kernel alone -----------------------------------------------------------------------------------------------------------
def _seven(inputs):
    return tuple(None if inputs.get(n) is None else inputs[n].detach().to(DEV).contiguous() for n in NAMES7)


def _kernel(inputs, cam, deg, mod, records, radii, want_campos=True, seven=None, home=lambda x: x, **kw):
    """home: what every device tensor handed to the call goes through first (tests/test_gpu_guard_bands.py moves them into guarded
    buffers with it; here the identity)."""
    st = home(pu.hip_settings(cam, deg, (0.0, 0.0, 0.0), mod))
    out = camera_grad.camera_backward(st, home(_seven(inputs)) if seven is None else seven, home(radii.to(DEV).contiguous()),
                                      home(records.to(DEV).contiguous()), want_campos, **kw)
    torch.cuda.synchronize()
    assert [tuple(o.shape) for o in out] == [(4, 4), (4, 4), (3,)]
    return torch.cat([o.reshape(-1) for o in out]).cpu().double().numpy()


def _held(got, inputs, cam, deg, mod, records, radii, what, want_campos=True):
    """got against the fp64 restatement within max(4 e_ref, 1 ulp of the sum's scale) (the module's docstring)."""
    ref = CR.camera_rule(inputs, cam, deg, mod, records, radii, want_campos=want_campos)
    scale = np.abs(CR.camera_rule(inputs, cam, deg, mod, records, radii, want_campos=want_campos, per_gaussian="scale")).sum(0)
    o32, _pre = CR.oracle_preprocess_camera_grads({k: v for k, v in inputs.items() if v is not None}, cam, deg, mod, records)
    if not want_campos:
        o32[32:] = 0.0
    assert np.isfinite(got).all(), (what, got)
    for sl, name in ((slice(0, 16), "viewmatrix"), (slice(16, 32), "projmatrix"), (slice(32, 35), "campos")):
        e_ref = float(np.abs(o32[sl] - ref[sl]).max())
        e_got = np.abs(got[sl] - ref[sl])
        bound = np.maximum(4.0 * e_ref, 2.0 ** -23 * scale[sl])
        print(what, name, "e_ref", e_ref, "e_got", float(e_got.max()), "worst e_got / bound", float((e_got / np.maximum(bound, 1e-300)).max()))
        assert (e_got <= bound).all(), (what, name, e_ref, e_got, bound)
    assert not got[CR.DEAD].any(), what
    return ref


@functools.lru_cache(maxsize=None)
def _sized(n, deg=3, mode="sh_sr"):
    sc = syn.make_scene(2 * 256 + 1, W, H, seed=12, log_scale_mean=-3.0)
    sc = syn.Scene(*[t[:n].contiguous() for t in sc])
    cam = _cam(0)
    inputs = G.mode_inputs(sc, cam, deg, 1.0, mode)
    pre = G.oracle_preprocess({k: v for k, v in inputs.items()}, cam, deg, 1.0) if n else None
    radii = pre["radii"] if n else torch.zeros(0, dtype=torch.int32)
    return inputs, cam, G.make_records(n, 20 + n), radii


@pytest.mark.parametrize("n", (0, 1, 63, 64, 65, 255, 256, 257, 2 * 256 + 1))
def test_kernel_alone_at_the_sizes_where_its_paths_part(n):
    inputs, cam, records, radii = _sized(n)
    got = _kernel(inputs, cam, 3, 1.0, records, radii)
    if n == 0:
        assert not got.any()
        return
    assert n < 2 or 0 < int((radii > 0).sum()) < n
    _held(got, inputs, cam, 3, 1.0, records, radii, ("size", n))


@pytest.mark.parametrize("deg", (0, 1, 2, 3))
@pytest.mark.parametrize("mode", ("sh_sr", "col_sr", "sh_cov", "col_cov"))
def test_kernel_alone_at_every_degree_and_input_mode(deg, mode):
    inputs, cam, records, radii = _sized(257, deg, mode)
    got = _kernel(inputs, cam, deg, 1.0, records, radii)
    ref = _held(got, inputs, cam, deg, 1.0, records, radii, (mode, deg))
    assert bool(ref[32:].any()) == (mode.startswith("sh") and deg > 0) == bool(got[32:].any())
    # NO_CAMPOS: the same viewmatrix and projmatrix gradients bit for bit, campos exact zeros
    without = _kernel(inputs, cam, deg, 1.0, records, radii, want_campos=False)
    assert np.array_equal(without[:32], got[:32]) and not without[32:].any()
    _held(without, inputs, cam, deg, 1.0, records, radii, (mode, deg, "NO_CAMPOS"), want_campos=False)


@pytest.mark.parametrize("deg", (1, 2, 3))
def test_kernel_alone_with_both_sh_record_layouts(deg):
    inputs, cam, records, radii = _sized(257, deg)
    seven = list(_seven(inputs))
    aligned = _kernel(inputs, cam, deg, 1.0, records, radii, seven=tuple(seven))
    buf = torch.empty(257 * 48 + 4, device=DEV)
    shifted = buf[1: 1 + 257 * 48].view(257, 16, 3)                    # 4 bytes off a 16-byte boundary: the scalar record reads
    shifted.copy_(seven[2])
    assert seven[2].data_ptr() % 16 == 0 and shifted.data_ptr() % 16 == 4 and shifted.is_contiguous()
    seven[2] = shifted
    assert np.array_equal(_kernel(inputs, cam, deg, 1.0, records, radii, seven=tuple(seven)), aligned)
    # fewer coefficients than 16 per record (M = (deg + 1)^2: no 16-byte records at M = 4 x 3 floats? 48 bytes: still aligned)
    K = (deg + 1) ** 2
    short = {**inputs, "shs": inputs["shs"][:, :K].contiguous()}
    assert np.array_equal(_kernel(short, cam, deg, 1.0, records, radii), aligned)


@functools.lru_cache(maxsize=None)
def _planted():
    pl = G.planted()
    inputs = pl.inputs(3, "sh_sr")
    pre = G.oracle_preprocess({k: v for k, v in inputs.items()}, pl.cam, 3, pl.mod)
    return pl, pre["radii"], G.make_records(inputs["means3D"].shape[0], 5)


@pytest.mark.parametrize("cls", ("all", "clamp_x", "clamp_y", "clamp_xy", "edge_x_over", "edge_y_over", "sh_neg", "lowpass", "lam_floor",
                                 "near_over", "partial"))
def test_kernel_alone_on_the_planted_edges(cls):
    """The 1.3 tanfov clamp active in x only, in y only, in both (and one ulp beyond the limit); each colour channel clamped alone,
    in pairs and all three; the 2D covariance at its low-pass floor (det at its smallest); the first visible depth."""
    pl, radii, records = _planted()
    if cls != "all":
        m = pl.members(cls)
        pl, radii, records = pl.subset(m), radii[m], records[m]
        assert bool((radii > 0).all())
    inputs = pl.inputs(3, "sh_sr")
    got = _kernel(inputs, pl.cam, 3, pl.mod, records, radii)
    _held(got, inputs, pl.cam, 3, pl.mod, records, radii, ("planted", cls))


def test_kernel_alone_with_an_empty_workgroup_between_two_full_ones_and_with_everything_culled():
    sc = syn.make_scene(3 * 256, W, H, seed=13, log_scale_mean=-3.0)
    sc.means3D[256:512, 2] = -sc.means3D[256:512, 2]                   # the middle workgroup: behind the camera
    cam = syn.default_camera(W, H)
    inputs = G.mode_inputs(sc, cam, 3, 1.0, "sh_sr")
    radii = G.oracle_preprocess({k: v for k, v in inputs.items()}, cam, 3, 1.0)["radii"]
    assert not bool((radii[256:512] > 0).any()) and int((radii[:256] > 0).sum()) > 100 and int((radii[512:] > 0).sum()) > 100
    records = G.make_records(3 * 256, 31)
    got = _kernel(inputs, cam, 3, 1.0, records, radii)
    _held(got, inputs, cam, 3, 1.0, records, radii, ("empty workgroup",))
    zeros = _kernel(inputs, cam, 3, 1.0, records, torch.zeros_like(radii))
    assert not zeros.any() and not np.signbit(zeros).any()


@pytest.mark.parametrize("deg,ray_fraction", [(3, 0.6), (0, 0.6), (1, 1.0), (2, 0.0)])
def test_kernel_alone_on_the_model_path(deg, ray_fraction):
    n = 257
    sc = syn.Scene(*[t[:n].contiguous() for t in _scene()])
    model = syn.make_raw_model(sc, ray_fraction=ray_fraction, seed=9)
    md = model.to(DEV)
    t = mp.tensors_of(md)
    assert mp.supported(t)
    inputs = _activated_inputs(model, md)
    cam = _cam(1)
    radii = G.oracle_preprocess({k: v for k, v in inputs.items()}, cam, deg, 1.0)["radii"]
    records = G.make_records(n, 40 + deg)
    for want_campos in (True, False):
        got = _kernel(inputs, cam, deg, 1.0, records, radii, want_campos=want_campos, seven=mp._ModelArgs(t))
        _held(got, inputs, cam, deg, 1.0, records, radii, ("model", deg, ray_fraction, want_campos), want_campos=want_campos)


# ---- 3: the translation identity ---------------------------------------------------------------------------------------------------
def _translation(st, leaves):
    V, PM = (t.detach().double().cpu().reshape(4, 4) for t in leaves[:2])
    dV, dPM, dc = (t.grad.double().cpu().reshape(-1) for t in leaves)
    return V[:3, :3] @ dV[12:15] + PM[:3, [0, 1, 3]] @ dPM[[12, 13, 15]] - dc


@pytest.mark.parametrize("mode", ("sh_sr", "col_sr", "sh_cov", "col_cov"))
def test_translation_identity_ties_the_restated_chain_to_the_geometry_backward(mode):
    """Moving every Gaussian by e equals moving the camera by -e: sum_i dL/dmeans3D_i = V[j, 0:3] . dV[12:15] + PM[j, (0, 1, 3)] .
    dPM[(12, 13, 15)] - dcampos.  The left side comes from geometry_backward_one, the right side from camgrad.hip."""
    sc, cam = _scene(), _cam(2)
    st, leaves = _with_leaves(cam, DEG, BG, 0.9)
    g = {k: v.to(DEV).requires_grad_(True) for k, v in pu.run_oracle_inputs(sc, cam, DEG, 0.9, mode).items() if k != "means2D"}
    out = R.GaussianRasterizer(st)(means2D=torch.zeros(P, 3, device=DEV, requires_grad=True), **g)
    _loss(out, 2).backward()
    torch.cuda.synchronize()
    pu.assert_close(_translation(st, leaves), g["means3D"].grad.double().sum(0).cpu(), ("translation identity", mode))


def test_translation_identity_on_the_model_path():
    model, md = _raw_model(ray_fraction=0.0)                            # every Gaussian free: bg_xyz.grad IS dL/dmeans3D
    cam = _cam(1)
    st, leaves = _with_leaves(cam, DEG, BG)
    out = rmod.render(_camera_object(cam, leaves), md, rmod.PipelineParams(), torch.tensor(BG, device=DEV))
    _loss((out["render"], None, out["rendered_depth"], out["rendered_alpha"]), 1).backward()
    torch.cuda.synchronize()
    pu.assert_close(_translation(st, leaves), md.bg_xyz.grad.double().sum(0).cpu(), ("translation identity", "model"))


# ---- 4: robustness and bit-exactness -----------------------------------------------------------------------------------------------
def test_runs_are_bit_equal_with_fresh_and_reused_partials_on_a_side_stream_and_in_a_captured_graph():
    inputs, cam, records, radii = _sized(2 * 256 + 1)
    seven = _seven(inputs)
    first = _kernel(inputs, cam, 3, 1.0, records, radii, seven=seven)
    assert np.array_equal(_kernel(inputs, cam, 3, 1.0, records, radii, seven=seven), first)
    out = torch.full((35,), float("nan"), device=DEV)
    partials = torch.full((3 * 27,), float("nan"), device=DEV)          # fresh: never written
    assert np.array_equal(_kernel(inputs, cam, 3, 1.0, records, radii, seven=seven, out=out, partials=partials), first)
    assert bool(torch.isfinite(partials).all())
    other = G.make_records(2 * 256 + 1, 77)
    second = _kernel(inputs, cam, 3, 1.0, other, radii, seven=seven, out=out, partials=partials)      # reused: the first run's sums
    assert np.array_equal(second, _kernel(inputs, cam, 3, 1.0, other, radii, seven=seven)) and not np.array_equal(second, first)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        on_side = _kernel(inputs, cam, 3, 1.0, records, radii, seven=seven)
    torch.cuda.current_stream().wait_stream(side)
    assert np.array_equal(on_side, first)
    # a captured graph replayed on rewritten records
    st = pu.hip_settings(cam, 3, (0.0, 0.0, 0.0))
    rec_d, radii_d = records.to(DEV).contiguous(), radii.to(DEV)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        camera_grad.camera_backward(st, seven, radii_d, rec_d, out=out, partials=partials)
    rec_d.copy_(other.to(DEV))
    out.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().double().numpy(), second)


def test_the_camera_pass_reads_nothing_back(monkeypatch):
    st, leaves = _with_leaves(_cam(0), DEG, BG)
    g = _gaussian_leaves(_scene())

    def step():
        return _loss(R.GaussianRasterizer(st)(means2D=torch.zeros(P, 3, device=DEV, requires_grad=True), **g), 0)
    step().backward()                                                   # (the camera's first render: its key is read once)
    loss = step()
    torch.cuda.synchronize()
    reads = []
    for name in ("cpu", "item", "tolist", "numpy"):
        orig = getattr(torch.Tensor, name)
        monkeypatch.setattr(torch.Tensor, name, (lambda orig, name: lambda self, *a, **k: (reads.append(name) if self.is_cuda else None,
                                                                                         orig(self, *a, **k))[1])(orig, name))
    orig_to = torch.Tensor.to
    monkeypatch.setattr(torch.Tensor, "to", lambda self, *a, **k: (reads.append("to") if self.is_cuda and any(
        str(v) == "cpu" for v in list(a) + list(k.values()) if isinstance(v, (str, torch.device))) else None, orig_to(self, *a, **k))[1])
    orig_sync = torch.cuda.synchronize
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: (reads.append("synchronize"), orig_sync(*a, **k))[1])
    loss.backward()
    forward_reads = len(reads)
    step()                                                              # the forward of a camera that was seen: no read either
    monkeypatch.undo()
    assert reads == [] and forward_reads == 0, reads
    assert all(t.grad is not None for t in leaves)


def test_the_default_path_keeps_its_bits():
    """Outputs and Gaussian gradients with and without requires_grad on the camera: bit for bit (a scene whose gradient records
    receive one contribution each, so that the float atomics of the blend backward have no order)."""
    Wq, Hq, Pq = 64, 48, 40
    sc, cam = pu.one_quadrant_scene(Pq, Wq, Hq, seed=3), syn.default_camera(Wq, Hq)
    up = [t.to(DEV) for t in syn.make_upstream_grads(Wq, Hq, seed=5)]

    def run(camera_grads):
        st, leaves = _with_leaves(cam, 3, BG)
        if not camera_grads:
            st = st._replace(viewmatrix=leaves[0].detach(), projmatrix=leaves[1].detach(), campos=leaves[2].detach())
        g = _gaussian_leaves(sc)
        m2 = torch.zeros(Pq, 3, device=DEV, requires_grad=True)
        outs = []
        for _ in range(2):                                             # the staged path, then the one-call path
            for t in (*g.values(), m2):
                t.grad = None
            c, r, d, a = R.GaussianRasterizer(st)(means2D=m2, **g)
            ((c * up[0]).sum() + (d * up[1]).sum() + (a * up[2]).sum()).backward()
            outs.append([c.detach(), r, d.detach(), a.detach(), m2.grad.clone(), *[t.grad.clone() for t in g.values()]])
        torch.cuda.synchronize()
        return outs, leaves
    plain, leaves_plain = run(False)
    with_cam, leaves_cam = run(True)
    assert all(t.grad is None for t in leaves_plain) and all(t.grad is not None for t in leaves_cam)
    for a_step, b_step in zip(plain, with_cam):
        for a, b in zip(a_step, b_step):
            assert torch.equal(a, b)


# ---- 5: pose recovery --------------------------------------------------------------------------------------------------------------
def test_pose_recovery_follows_the_oracles_loop():
    """60 Adam steps on CameraPose.delta at 40 x 24 pixels, Gaussians fixed (examples/fit_pose.py): the oracle's loop ends below a
    tenth of the initial pose error (the premise: tests/test_camgrad_cpu.py checks it without a GPU), the kernels' loop within twice
    the oracle's final error — fp32 trajectories part."""
    fp = CR.fit_pose_module()
    e0, _h, e_oracle = fp.fit(rasterize=CR.rasterize_oracle, dev="cpu", verbose=False)
    e0_hip, _h, e_hip = fp.fit(dev=DEV, verbose=False)
    print("pose error: initial", e0, "oracle's loop", e_oracle, "kernels' loop", e_hip)
    assert abs(e0_hip - e0) < 1e-5 * e0 and e_oracle < 0.1 * e0        # (the same start, up to the two devices' fp32 sin and cos)
    assert e_hip <= 2.0 * e_oracle, (e_hip, e_oracle)

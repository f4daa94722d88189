"""The forward that never reads the host (rasterizer.NO_HOST_READ, ScgFrame.num_rendered_out) and the captured training step
built on it (graph_step.CapturedStep) — VERDICT r5 item 3; SURVEY §8b "or none, if the caller passes a capacity and the kernel
reports overflow".

Bar: a no-host-read / replayed forward equals the default one BIT FOR BIT (same kernels, same capacity class); gradients within
the noise of the blend backward's float atomics (two eager backwards differ by as much: measured against each other here);
an overflow (the scene grew past the frozen capacity) is detected at the NEXT render / replay and that one is complete again.
"""
import numpy as np
import pytest
import torch

import parity_utils as pu
from captured_refs import grad_noise_ok as _grad_noise_ok
from scgaussian_amd import graph_step as gs
from scgaussian_amd import rasterizer as R
from scgaussian_amd import render as rmod
from scgaussian_amd import synthetic as syn

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _leaves(sc):
    return [t.detach().clone().to(DEV).requires_grad_(True) for t in (sc.means3D, sc.shs, sc.opacities, sc.scales, sc.rotations)]


def _step(rast, leaves, ups):
    m, f, o, s, r = leaves
    c, radii, d, a = rast(means3D=m, means2D=torch.zeros_like(m, requires_grad=True), opacities=o, shs=f, scales=s, rotations=r)
    torch.autograd.backward([c, d, a], list(ups))
    return c, d, a, radii


def _eager(rast, leaves, ups):
    for p in leaves:
        p.grad = None
    out = _step(rast, leaves, ups)
    torch.cuda.synchronize()
    return [t.detach().clone() for t in out], [p.grad.detach().clone() for p in leaves]


def test_no_host_read_forward_is_the_default_forward_bit_for_bit():
    P, W, H = 30_000, 400, 304
    sc = syn.make_scene(P, W, H, seed=2).to(DEV)
    cam = syn.orbit_camera(W, H, 4.0, 2.0, 7.0)
    st = pu.hip_settings(cam, 3, (0.1, 0.2, 0.3))
    rast = R.GaussianRasterizer(st)
    args = dict(means3D=sc.means3D, means2D=torch.zeros_like(sc.means3D), opacities=sc.opacities, shs=sc.shs, scales=sc.scales,
                rotations=sc.rotations)
    with torch.no_grad():
        rast(**args)                                                     # staged: establishes the capacity
        want = [t.clone() for t in rast(**args)]                         # one-call path, host read
        ref = R.forward_fused(st, sc.means3D, sc.opacities, sc.shs, None, sc.scales, sc.rotations, None, False)
        Rn = ref[4]["num_rendered"]
        before = R.overflow_stats()
        with R.no_host_read():
            got = rast(**args)
            out = R.forward_fused(st, sc.means3D, sc.opacities, sc.shs, None, sc.scales, sc.rotations, None, False)
        assert out[4]["num_rendered"] is None and out[4]["count_word"] is not None
        torch.cuda.synchronize()
        assert out[4]["count_word"].value() == Rn                        # the binning stage's own count, in the pinned word
        for g, w in zip(got, want):
            assert torch.equal(g, w)
        after = R.settle_counts()
        assert after["renders"] == before["renders"] + 2 and after["settled"] == before["settled"] + 2
        assert after["overflows"] == before["overflows"]


def test_no_host_read_overflow_is_noticed_at_the_cameras_next_render():
    P, W, H = 20_000, 320, 240
    sc = syn.make_scene(P, W, H, seed=5).to(DEV)
    cam = syn.orbit_camera(W, H, -6.0, 1.0, 7.0)
    st = pu.hip_settings(cam, 2, (0.0, 0.0, 0.0))
    rast = R.GaussianRasterizer(st)
    scales = sc.scales.clone()

    def render():
        return rast(means3D=sc.means3D, means2D=torch.zeros_like(sc.means3D), opacities=sc.opacities, shs=sc.shs, scales=scales,
                    rotations=sc.rotations)
    with torch.no_grad():
        render()
        render()
        scales.mul_(5.0)                                                 # the scene grows: several times the instances
        before = R.settle_counts()
        with R.no_host_read():
            clipped = [t.clone() for t in render()]                      # launched with the old capacity
            torch.cuda.synchronize()
            again = [t.clone() for t in render()]                        # looks at the word first: room for the count now
            torch.cuda.synchronize()
        stats = R.settle_counts()
        assert stats["overflows"] == before["overflows"] + 1
        truth = render()                                                 # default mode (host read + retry): the complete result
        for g, w in zip(again, truth):
            assert torch.equal(g, w)
        assert not torch.equal(clipped[0], truth[0])                     # (the clipped render WAS incomplete: the test bites)
        assert torch.equal(clipped[1], truth[1])                         # radii come from the geometry stage: never clipped


def test_a_forward_the_library_rejects_gives_its_count_word_back():
    """scg_forward rejects sh_degree 4 on the host, before anything is launched: the count word the attempt took goes back to the
    pool (without the release in forward_fused's error path the free list stays one slot short)."""
    from scgaussian_amd import _counts, _lib
    P, W, H = 64, 32, 32
    sc = syn.make_scene(P, W, H, seed=1).to(DEV)
    st = pu.hip_settings(syn.default_camera(W, H), 3, (0.0, 0.0, 0.0))
    args = dict(means3D=sc.means3D, means2D=torch.zeros_like(sc.means3D), opacities=sc.opacities, shs=sc.shs, scales=sc.scales,
                rotations=sc.rotations)
    with torch.no_grad():
        R.GaussianRasterizer(st)(**args)                                 # a normal render: the camera's capacity is known
        torch.cuda.synchronize()
        before = R.settle_counts()
        _counts._count_pool()
        spec, ckey = R._spec_state(sc.means3D.device), (W, H, R._camera_key(st.viewmatrix))
        free = len(_counts._COUNT_FREE)
        with R.no_host_read():
            with pytest.raises(_lib.ScgError) as err:
                R.GaussianRasterizer(st._replace(sh_degree=4))(**args)
            assert "sh_degree 4 not in 0..3" in str(err.value)
            assert len(_counts._COUNT_FREE) == free
            assert ckey not in spec.pending
            R.GaussianRasterizer(st)(**args)
        torch.cuda.synchronize()
        after = R.settle_counts()
    assert after["settled"] == before["settled"] + 1 and after["overflows"] == before["overflows"]
    assert len(_counts._COUNT_FREE) == free


@pytest.mark.parametrize("workload", ["small", "S1"])
def test_captured_step_replays_the_eager_step(workload):
    P, W, H = (10_000, 256, 256) if workload == "S1" else (4_000, 160, 128)
    sc = syn.make_scene(P, W, H, seed=1)
    cam = syn.orbit_camera(W, H, 3.0, -2.0, 7.0)
    st = pu.hip_settings(cam, 3, (0.2, 0.2, 0.2))
    rast = R.GaussianRasterizer(st)
    leaves = _leaves(sc)
    ups = [t.to(DEV) for t in syn.make_upstream_grads(W, H, seed=4)]
    _eager(rast, leaves, ups)
    want_out, want_g = _eager(rast, leaves, ups)
    _, noise_g = _eager(rast, leaves, ups)                               # a second eager backward: the atomics' noise
    step = gs.CapturedStep(lambda: _step(rast, leaves, ups), params=leaves)
    for _ in range(3):
        out = step.replay()
    torch.cuda.synchronize()
    for g, w in zip(out, want_out):
        assert torch.equal(g, w)                                         # images and radii: bit for bit
    _grad_noise_ok([p.grad for p in leaves], want_g, noise_g)
    assert step.overflows == 0 and step.recaptures == 0 and len(step.words) == 1
    # the parameters move (an optimizer step in place): the replay follows them, like the eager step
    with torch.no_grad():
        leaves[0].add_(0.01 * torch.randn_like(leaves[0]))
        leaves[2].mul_(0.97)
    out = [t.clone() for t in step.replay()]
    got_g = [p.grad.clone() for p in leaves]
    torch.cuda.synchronize()
    saved = [p.grad for p in leaves]
    want_out, want_g = _eager(rast, leaves, ups)
    _, noise_g = _eager(rast, leaves, ups)
    for g, w in zip(out, want_out):
        assert torch.equal(g, w)
    _grad_noise_ok(got_g, want_g, noise_g)
    for p, g in zip(leaves, saved):
        p.grad = g
    step.close()


def test_captured_step_recovers_from_an_overflow_one_replay_late():
    P, W, H = 12_000, 256, 192
    sc = syn.make_scene(P, W, H, seed=7)
    cam = syn.orbit_camera(W, H, 0.0, 0.0, 7.0)
    st = pu.hip_settings(cam, 1, (0.0, 0.0, 0.0))
    rast = R.GaussianRasterizer(st)
    leaves = _leaves(sc)
    ups = [t.to(DEV) for t in syn.make_upstream_grads(W, H, seed=2)]
    step = gs.CapturedStep(lambda: _step(rast, leaves, ups), params=leaves)
    step.replay()
    torch.cuda.synchronize()
    cap0 = step.capacities[0]
    with torch.no_grad():
        leaves[3].mul_(5.0)                                              # scales x5: num_rendered far beyond capacity + 25 %
    step.replay()                                                        # clipped (nobody knows yet)
    torch.cuda.synchronize()
    assert step.overflows == 0
    out = [t.clone() for t in step.replay()]                             # sees the count, captures again, replays: complete
    got_g = [p.grad.clone() for p in leaves]
    torch.cuda.synchronize()
    assert step.overflows == 1 and step.recaptures == 1 and step.capacities[0] > cap0
    want_out, want_g = _eager(rast, leaves, ups)
    _, noise_g = _eager(rast, leaves, ups)
    for g, w in zip(out, want_out):
        assert torch.equal(g, w)
    _grad_noise_ok(got_g, want_g, noise_g)
    step.close()


def test_captured_step_through_render_on_the_reference_model():
    """render() on the reference's raw parameterisation (the model path) inside a captured step."""
    P, W, H = 10_000, 256, 256
    sc = syn.make_scene(P, W, H, seed=3)
    model = syn.make_raw_model(sc).to(DEV).requires_grad_()
    model.active_sh_degree = 1
    cam = syn.orbit_camera(W, H, 2.0, 1.0, 7.0).to(DEV)
    pipe = rmod.PipelineParams()
    bg = torch.zeros(3, device=DEV)
    ups = [t.to(DEV) for t in syn.make_upstream_grads(W, H, seed=6)]
    params = model.parameters()

    def fn():
        o = rmod.render(cam, model, pipe, bg)
        torch.autograd.backward([o["render"], o["rendered_depth"], o["rendered_alpha"]], list(ups))
        return o["render"], o["rendered_depth"], o["rendered_alpha"], o["radii"], o["viewspace_points"]

    def eager():
        for p in params:
            p.grad = None
        out = fn()
        torch.cuda.synchronize()
        return [t.detach().clone() for t in out[:4]], [p.grad.detach().clone() for p in params], out[4].grad.detach().clone()
    eager()
    want_out, want_g, want_vs = eager()
    _, noise_g, _ = eager()
    step = gs.CapturedStep(fn, params=params)
    for _ in range(2):
        out = step.replay()
    torch.cuda.synchronize()
    for g, w in zip(out[:4], want_out):
        assert torch.equal(g, w)
    _grad_noise_ok([p.grad for p in params], want_g, noise_g)
    assert out[4].grad is not None and out[4].grad.shape == want_vs.shape
    assert np.allclose(out[4].grad.cpu().numpy(), want_vs.cpu().numpy(), rtol=1e-3, atol=1e-7 * float(want_vs.abs().max()) + 1e-12)
    step.close()


def test_a_fresh_camera_per_frame_costs_no_device_synchronisation():
    """VERDICT r5 item 9 / ADVICE r5: the camera key of a NEW device view-matrix tensor is its content, read back once (a
    synchronising copy).  A caller that builds a camera per frame avoids it by handing the matrices over in host memory or by
    naming the camera (tag_camera): torch's sync debug mode raises on any synchronising torch call inside the render."""
    P, W, H = 8_000, 256, 192
    sc = syn.make_scene(P, W, H, seed=9).to(DEV)
    args = dict(means3D=sc.means3D, means2D=torch.zeros_like(sc.means3D), opacities=sc.opacities, shs=sc.shs, scales=sc.scales,
                rotations=sc.rotations)

    def settings(i, on_host, tag):
        cam = syn.orbit_camera(W, H, 2.0 + 0.5 * i, 1.0, 7.0)
        st = pu.hip_settings(cam, 3, (0.0, 0.0, 0.0))
        if on_host:
            st = st._replace(viewmatrix=cam.world_view_transform.clone(), projmatrix=cam.full_proj_transform.clone(),
                             campos=cam.camera_center.clone())
        if tag:
            R.tag_camera(st.viewmatrix, "fly-through")
        return st
    with torch.no_grad():
        R.GaussianRasterizer(settings(0, False, False))(**args)                      # the shape's capacity (staged path)
        R.GaussianRasterizer(settings(0, False, True))(**args)
        frames = [settings(i, on_host, not on_host) for i in range(1, 4) for on_host in (True, False)]
        torch.cuda.synchronize()
        keys_before = len(R._CAM_KEYS)
        torch.cuda.set_sync_debug_mode("error")
        try:
            imgs = [R.GaussianRasterizer(st)(**args)[0] for st in frames]
        finally:
            torch.cuda.set_sync_debug_mode("default")
        torch.cuda.synchronize()
        assert len(R._CAM_KEYS) == keys_before                                       # nobody's content was read back
        # the same frames through the default route (device matrices, content keys): the same images
        for i, img in zip((1, 1, 2, 2, 3, 3), imgs):
            want = R.GaussianRasterizer(settings(i, False, False))(**args)[0]
            assert torch.equal(img, want)
        # a device matrix whose content has been read once is recognised by its address: a NEW view object of the same memory
        # per call (`cam.world_view_transform.view(4, 4)`) costs no second read
        st = settings(5, False, False)
        R.GaussianRasterizer(st)(**args)
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            for _ in range(3):
                R.GaussianRasterizer(st._replace(viewmatrix=st.viewmatrix.view(4, 4)))(**args)
        finally:
            torch.cuda.set_sync_debug_mode("default")


def test_training_with_captured_steps_follows_the_eager_trajectory():
    """examples/fit_captured.py: the reference's raw model trained through render() + the fused image loss + Adam, once with one
    captured step per view (the optimizer stepping the parameters in place between replays) and once eagerly: both improve the
    PSNR by the same amount (the trajectories differ by the float atomics' order only)."""
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("fit_captured", os.path.join(root, "examples", "fit_captured.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    h_cap, _ = mod.fit(iters=150, P=4000, W=192, H=144, captured=True, verbose=False)
    h_eag, _ = mod.fit(iters=150, P=4000, W=192, H=144, captured=False, verbose=False)
    assert h_cap[-1][2] > h_cap[0][2] + 3.0, h_cap                      # PSNR rises by more than 3 dB in 150 iterations
    assert abs(h_cap[-1][2] - h_eag[-1][2]) < 0.3, (h_cap[-1], h_eag[-1])
    assert abs(h_cap[0][1] - h_eag[0][1]) <= 1e-5 * max(1.0, abs(h_eag[0][1]))      # the first step: the same loss

"""CPU-only checks of the virtual-view warp loss and the depth smoothness (scgaussian_amd/virtual.py, libscg_vw.so,
include/vw/scg_virtualwarp.h): the restatements the GPU tests compare against (tests/virtualwarp_refs.py) are held to what the
reference's own functions gave (tests/golden/ref_virtualwarp.npz); the reflection fold to autograd; the fifth library and its
binding to the header's text; the library's validation to its codes; the host arithmetic to the fixture; the plain-torch twin
(the path CPU tensors take) to the fp64 restatement under the GPU tests' bar."""
import types

import numpy as np
import pytest
import torch

import virtualwarp_refs as VR
from abi_compare import VOID, check_side_library
from scgaussian_amd import _lib, _lib_vw, synthetic, virtual

FX = np.load(VR.GOLDEN)
TAGS = [str(t) for t in FX["scenes"]]


def _scene(tag):
    return {k: FX[f"{tag}_{k}"] for k in VR.KEYS}


# ---- the restatements against the reference's recorded results ------------------------------------------------------------------
@pytest.mark.parametrize("tag", TAGS)
def test_reference_shaped_expression_equals_the_reference(tag):
    """In fp32 on the CPU the expression IS the reference's arithmetic: the loss bit for bit.  Its gradients differ from the
    recorded ones only by the order in which autograd adds the windows' terms (the expression picks the winner with a gather, the
    reference with a min): two fp32 evaluations of one function, held to each other by the bar the kernels are held to fp64 by,
    max(4 e_ref, 1 ulp), e_ref being the recorded gradients' own deviation from fp64.  In fp64 it lies within the fp32 result's
    own resolution."""
    sc = _scene(tag)
    r32, r64 = VR.warp_reference(sc, torch.float32), VR.warp_reference(sc)
    assert r32["loss"].dtype == np.float32 and np.array_equal(r32["loss"], FX[f"{tag}_loss"])
    for k in ("d_img", "d_depth"):
        want = FX[f"{tag}_{k}"]
        assert np.abs(r32[k] - want).max() <= VR.bar(np.abs(r64[k] - want).max(), r64[k]), k
        assert np.abs(r64[k] - want).max() <= 1e-4 * np.abs(want).max(), k
    assert abs(float(r64["loss"]) - float(FX[f"{tag}_loss"])) <= 1e-6
    assert (r64["winner"] >= 0).mean() > 0.3


@pytest.mark.parametrize("tag", TAGS)
def test_restatement_on_the_composed_records(tag):
    """The header's rule from the composed matrices: with the records left in fp64 it IS the reference-shaped expression (algebra
    alone: 1e-11); with the records rounded to fp32, as the kernels get them, it moves by the rounding's first-order effect — a tap
    shift below 2^-24 x 4 terms x 20 px ~ 5e-6 px, a loss's 1e-6 at these textures' slopes — far from what a wrong matrix would do
    (1e-2).  The seeds leave no near tie."""
    sc = _scene(tag)
    r64, r32 = VR.warp_reference(sc), VR.warp_reference(sc, torch.float32)
    exact = VR.warp_reference(sc, records=virtual.compose_records(sc["intrs"], sc["w2cs"], sc["vir_c2w"], dtype=np.float64))
    truth = VR.warp_reference(sc, records=virtual.compose_records(sc["intrs"], sc["w2cs"], sc["vir_c2w"]))
    for k in ("loss", "loss_map", "d_img", "d_depth", "s", "tap"):
        scale = np.abs(r64[k]).max()
        assert np.abs(exact[k] - r64[k]).max() <= 1e-11 * scale, k
        assert np.abs(truth[k] - r64[k]).max() <= (2e-5 if k == "tap" else 1e-5 * max(scale, 1e-2)), k
    for t in (exact, truth):
        assert np.array_equal(t["winner"], r64["winner"]) and np.array_equal(t["in_bounds"], r64["in_bounds"])
    # the seeds were chosen to leave none at four times the margin; held here at twice, since e_ref is this CPU's
    assert not VR.near_ties(r64, r32, truth, tie=2 * VR.TIE)["share"]


@pytest.mark.parametrize("tag", TAGS)
@pytest.mark.parametrize("form", ["g0", "g2", "g3"])
def test_smoothness_restatement_equals_the_reference(tag, form):
    guide = {"g0": None, "g2": FX[f"{tag}_guide"][0], "g3": FX[f"{tag}_guide"]}[form]
    depth = FX[f"{tag}_virtual_depth"]
    l32, g32 = VR.smooth_reference(depth, guide, torch.float32)
    l64, g64 = VR.smooth_reference(depth, guide)
    assert np.array_equal(l32, FX[f"{tag}_smooth_{form}"]) and np.array_equal(g32, FX[f"{tag}_smooth_d_depth_{form}"])
    assert abs(float(l64) - float(l32)) < 1e-6 and np.abs(g64 - g32).max() < 1e-6 * np.abs(g64).max() + 1e-9
    twin = virtual.smooth_loss(torch.from_numpy(depth), None if guide is None else torch.from_numpy(guide))       # CPU tensors: the twin
    assert np.array_equal(twin.numpy(), l32)


# ---- the reflection fold --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", [3, 4, 5, 6])
@pytest.mark.parametrize("W", [3, 4, 5, 6])
def test_reflection_fold_against_autograd(H, W):
    rng = np.random.default_rng(H * 10 + W)
    x, y, up = rng.uniform(0.05, 0.95, (3, H, W)), rng.uniform(0.05, 0.95, (3, H, W)), rng.uniform(0.5, 1.5, (H, W))
    X, Y = torch.from_numpy(x).requires_grad_(True), torch.from_numpy(y).requires_grad_(True)
    raw, term = VR.ssim_terms(X[None], Y[None])
    (term[0].sum(dim=0) * torch.from_numpy(up)).sum().backward()
    gx, gy = VR.window_gradients(x, y, up)
    scale = max(np.abs(X.grad.numpy()).max(), np.abs(Y.grad.numpy()).max())
    assert np.abs(gx - X.grad.numpy()).max() < 1e-12 * scale and np.abs(gy - Y.grad.numpy()).max() < 1e-12 * scale
    assert ((raw.detach().numpy() > 0) & (raw.detach().numpy() < 1)).any()


def test_fold_counts_are_the_reflections_of_the_padded_window():
    for n in range(3, 9):
        refl = lambda u: -u if u < 0 else (2 * (n - 1) - u if u >= n else u)      # noqa: E731
        for q in range(n):
            assert sorted(VR.fold_positions(q, n)) == sorted(u for u in range(-2, n + 2) if refl(u) == q)
            for p in range(n):
                direct = sum(1 for u in range(p - 2, p + 3) if refl(u) == q)
                assert direct == (VR.fold_count(p, q, n) if abs(p - q) <= 2 else 0), (n, q, p)      # every centre lies within 2 of q


# ---- the fifth library against its header ---------------------------------------------------------------------------------------
def test_fifth_library_exports_and_binds_exactly_its_header():
    abi = check_side_library(_lib_vw, "vw", "scg_virtualwarp.h", VOID)
    assert len(abi.functions) == 8 and not abi.structs
    assert {d.base for fn in abi.functions for d in fn.params if not d.pointer} <= {"int", "int32_t", "size_t"}
    assert sorted(abi.defines) == sorted("SCG_" + n for n in (
        "VW_ABI_VERSION", "VW_MAX_VIEWS", "VW_TILE", "VW_SMOOTH_PIXELS", "VW_RECORD_FLOATS", "VW_MIN_DIM", "VW_MAX_DIM",
        "VW_MAX_GUIDE_CHANNELS"))
    assert _lib_vw.VW_MAX_VIEWS >= 8 and _lib_vw.VW_TILE ** 2 == 256


# ---- scratch sizes and validation, without a GPU ----------------------------------------------------------------------------------
def test_scratch_sizes():
    lib = _lib_vw.load()
    for nv, H, W in ((1, 3, 3), (3, 13, 17), (16, 16, 16), (2, 17, 33), (3, 378, 504)):
        tiles = -(-H // 16) * -(-W // 16)
        assert lib.scg_vw_warp_scratch_bytes(nv, H, W) == 8 * (6 * nv * H * W + tiles) + 4 * 12 * H * W
    for bad in ((0, 8, 8), (17, 8, 8), (1, 2, 8), (1, 8, 2), (1, 16385, 8), (1, 8, 16385), (-1, 8, 8)):
        assert lib.scg_vw_warp_scratch_bytes(*bad) == 0
    assert [lib.scg_vw_smooth_scratch_bytes(h, w) for h, w in ((1, 1), (1, 256), (1, 257), (16, 33))] == [16, 16, 32, 48]
    assert lib.scg_vw_smooth_scratch_bytes(0, 4) == 0 and lib.scg_vw_smooth_scratch_bytes(4, 16385) == 0


def test_validation_returns_codes_without_a_gpu():
    """Every call below fails its validation before anything touches a device: the device pointers are never dereferenced."""
    lib = _lib_vw.load()
    err = lib.scg_vw_last_error
    fake, big = 0x1000, 1 << 30
    fwd = dict(nv=3, H=13, W=17, img=fake, depth=fake, mask=fake, colors=fake, records=fake, loss=fake, loss_map=fake, winner=fake,
               in_bounds=fake, scratch=fake, nbytes=big)
    call_f = lambda **k: lib.scg_vw_warp_forward(*{**fwd, **k}.values(), None)      # noqa: E731
    need = lib.scg_vw_warp_scratch_bytes(3, 13, 17)
    for k in ("img", "depth", "mask", "colors", "records", "loss", "loss_map", "winner", "in_bounds", "scratch"):
        assert call_f(**{k: None}) == -1 and b"NULL" in err(), k
    for k in ("img", "depth", "colors", "records", "loss", "loss_map"):
        assert call_f(**{k: fake + 2}) == -5 and b"aligned" in err(), k
    assert call_f(mask=fake + 1, winner=fake + 3, in_bounds=fake + 1, nbytes=need - 1) == -4 and b"scratch of" in err()
    assert call_f(scratch=fake + 8) == -5 and b"16-byte" in err()
    for k, bad in (("nv", 0), ("nv", 17), ("H", 2), ("W", 2), ("H", 16385), ("W", 16385), ("H", -1)):
        assert call_f(**{k: bad}) == -2, (k, bad)
    assert b"reflects" in err()
    bwd = dict(nv=3, H=13, W=17, img=fake, upstream=fake, winner=fake, scratch=fake, nbytes=big, d_img=fake, d_depth=fake)
    call_b = lambda **k: lib.scg_vw_warp_backward(*{**bwd, **k}.values(), None)      # noqa: E731
    for k in ("img", "upstream", "winner", "scratch", "d_img", "d_depth"):
        assert call_b(**{k: None}) == -1, k
    assert call_b(nbytes=need - 4) == -4 and call_b(d_depth=fake + 1) == -5 and call_b(nv=17) == -2 and call_b(W=2) == -2
    sf = dict(H=5, W=7, C=0, depth=fake, guide=None, loss=fake, scratch=fake, nbytes=16)
    call_s = lambda **k: lib.scg_vw_smooth_forward(*{**sf, **k}.values(), None)      # noqa: E731
    assert call_s(depth=None) == -1 and call_s(loss=None) == -1 and call_s(scratch=None) == -1
    assert call_s(guide=fake) == -3 and b"C = 0" in err()
    assert call_s(C=1) == -1 and call_s(C=3, guide=fake + 1) == -5
    assert call_s(C=-1) == -2 and call_s(C=65, guide=fake) == -2 and call_s(H=0) == -2 and call_s(W=16385) == -2
    assert call_s(nbytes=15) == -4 and call_s(scratch=fake + 4) == -5
    sb = dict(H=5, W=7, C=0, depth=fake, guide=None, upstream=fake, d_depth=fake)
    call_sb = lambda **k: lib.scg_vw_smooth_backward(*{**sb, **k}.values(), None)      # noqa: E731
    assert call_sb(upstream=None) == -1 and call_sb(d_depth=None) == -1 and call_sb(guide=fake) == -3 and call_sb(H=0) == -2
    assert call_sb(C=2) == -1 and call_sb(depth=fake + 1) == -5


# ---- the host arithmetic --------------------------------------------------------------------------------------------------------
def test_near_virtual_pose_equals_the_fixture():
    got = virtual.near_virtual_pose(FX["pose_c2ws"], FX["pose_near_far"], np.random.RandomState(int(FX["pose_seed"])))
    assert got.shape == (3, 4) and got.dtype == np.float64 and np.array_equal(got, FX["pose_out"])
    np.random.seed(int(FX["pose_seed"]))
    assert np.array_equal(virtual.near_virtual_pose(FX["pose_c2ws"], FX["pose_near_far"]), FX["pose_out"])     # the default: np.random
    R = got[:, :3]
    assert np.allclose(R.T @ R, np.eye(3), atol=1e-12)


def test_composed_records_are_the_chain_in_fp64():
    sc = _scene("a")
    rec = virtual.compose_records(sc["intrs"], sc["w2cs"], sc["vir_c2w"])
    assert rec.shape == (3, 12) and rec.dtype == np.float32
    K, E, c2w = sc["intrs"].astype(np.float64), sc["w2cs"].astype(np.float64), sc["vir_c2w"].astype(np.float64)
    p = np.array([5.0, 7.0, 1.0]) * 2.5
    for v in range(3):
        world = c2w[:, :3] @ (np.linalg.inv(K[0]) @ p) + c2w[:, 3]
        want = K[v] @ (E[v, :3, :3] @ world + E[v, :3, 3])
        got = 2.5 * (rec[v, :9].reshape(3, 3).astype(np.float64) @ [5.0, 7.0, 1.0]) + rec[v, 9:]
        assert np.allclose(got, want, rtol=1e-6, atol=1e-5)
    other = virtual.compose_records(sc["intrs"], sc["w2cs"], sc["vir_c2w"], intr=sc["intrs"][1])
    assert not np.array_equal(other, rec)
    with pytest.raises(_lib.ScgError):
        virtual.compose_records(sc["intrs"], sc["w2cs"][:2], sc["vir_c2w"])


def test_virtual_camera_builds_the_records_matrices():
    like = synthetic.orbit_camera(40, 30, 10.0, -5.0, 7.0)
    w2c = like.world_view_transform.T.numpy().astype(np.float64)
    cam = virtual.virtual_camera(np.linalg.inv(w2c)[:3], like)
    assert (cam.image_height, cam.image_width, cam.FoVx, cam.FoVy) == (30, 40, like.FoVx, like.FoVy)
    for a, b in ((cam.world_view_transform, like.world_view_transform), (cam.full_proj_transform, like.full_proj_transform),
                 (cam.camera_center, like.camera_center)):
        assert torch.allclose(a, b, atol=2e-6)
    moved = np.linalg.inv(w2c)
    moved[:3, 3] += [0.5, 0.0, 0.0]
    assert torch.allclose(virtual.virtual_camera(moved, like).camera_center - like.camera_center, torch.tensor([0.5, 0.0, 0.0]), atol=1e-5)


# ---- the twin: the path CPU tensors take ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", TAGS)
def test_twin_on_cpu_tensors_meets_the_bar(tag):
    sc = _scene(tag)
    r64, r32 = VR.warp_reference(sc), VR.warp_reference(sc, torch.float32)
    t = VR.tensors(sc)
    H, W = sc["virtual_depth"].shape
    img, depth = t["virtual_img"].requires_grad_(True), t["virtual_depth"].reshape(1, H, W).requires_grad_(True)
    loss = virtual.virtual_warp_loss(img, depth, sc["vir_c2w"], t["intrs"], t["w2cs"], t["img_colors"], t["vir_mask"].reshape(1, H, W))
    loss.backward()
    got = {"loss": loss.detach().numpy(), "d_img": img.grad.numpy(), "d_depth": depth.grad.numpy()[0]}
    for k, v in got.items():
        dev, e_ref, bound = VR.compare(k, v, r64, r32)
        print(tag, k, "twin deviation", dev, "e_ref", e_ref, "bound", bound)
        assert dev <= bound, (k, dev, e_ref, bound)
    warp = virtual.VirtualWarp(t["intrs"], t["w2cs"], t["img_colors"])
    warp.set_pose(sc["vir_c2w"])
    warp.loss(t["virtual_img"].detach(), t["virtual_depth"].detach(), t["vir_mask"])
    assert np.array_equal(warp.winner.numpy(), r64["winner"]) and np.array_equal(warp.in_bounds.numpy().astype(bool), r64["in_bounds"])
    assert warp.winner.dtype == torch.int8 and warp.loss_map.shape == (H, W)


def test_python_entry_points_refuse_what_the_kernels_do_not_take():
    sc = _scene("b")
    t = VR.tensors(sc)
    with pytest.raises(_lib.ScgError, match=r"\(H,W\)"):
        virtual.smooth_loss(t["virtual_depth"][None])                       # (1,H,W): the reference's slicing gives NaN
    with pytest.raises(_lib.ScgError, match="guide"):
        virtual.smooth_loss(t["virtual_depth"], t["virtual_depth"][:, :-1])
    with pytest.raises(_lib.ScgError, match="views"):
        virtual.VirtualWarp(t["intrs"][:1].expand(17, 3, 3), t["w2cs"][:1].expand(17, 4, 4), t["img_colors"][:1].expand(17, 3, 9, 11))
    with pytest.raises(_lib.ScgError, match="height and width"):
        virtual.VirtualWarp(t["intrs"], t["w2cs"], t["img_colors"][:, :, :2])
    with pytest.raises(_lib.ScgError, match="intrs"):
        virtual.VirtualWarp(t["intrs"][:1], t["w2cs"], t["img_colors"])
    warp = virtual.VirtualWarp(t["intrs"], t["w2cs"], t["img_colors"])
    with pytest.raises(_lib.ScgError, match="virtual_img"):
        warp.loss(t["virtual_img"][:, :-1], t["virtual_depth"], t["vir_mask"])
    with pytest.raises(_lib.ScgError, match="vir_mask"):
        warp.loss(t["virtual_img"], t["virtual_depth"], t["vir_mask"].float())
    view_gs = {str(v): {"image_color": t["img_colors"][v].permute(1, 2, 0), "intr": t["intrs"][v], "w2c": t["w2cs"][v], "height": 9,
                        "width": 11} for v in range(2)}
    assert torch.equal(virtual.VirtualWarp.from_view_gs(view_gs).colors, t["img_colors"])
    assert torch.equal(virtual.VirtualWarp.from_mono(types.SimpleNamespace(view_gs=view_gs)).colors, t["img_colors"])
    view_gs["1"]["height"] = 10
    with pytest.raises(_lib.ScgError, match="equal sizes"):
        virtual.VirtualWarp.from_view_gs(view_gs)
    with pytest.raises(_lib.ScgError, match="no view"):
        virtual.VirtualWarp.from_view_gs({})
    ns = types.SimpleNamespace()
    virtual.install(ns)
    assert ns.get_virtual_warp_loss is virtual.virtual_warp_loss and ns.get_smooth_loss is virtual.smooth_loss

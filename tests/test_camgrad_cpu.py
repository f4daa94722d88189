"""The camera gradients without a GPU: the fp64 numpy restatement of the rule (tests/camgrad_refs.py) against the oracle's autograd
on preprocess and on the full rasterizer, a mutant of each clause of the rule, the header's text against the library's exports and
the binding, every argument code, the library's entry of the build table, and CameraPose against fp64."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

import abi_compare
import camgrad_refs as CR
import geometry_refs as G
import parity_utils as pu
from scgaussian_amd import _lib, _lib_camgrad, build, pose
from scgaussian_amd import synthetic as syn

W, H, P = 40, 24, 300
MODES = ("sh_sr", "col_sr", "sh_cov")                  # SH colours | colors_precomp | cov3D_precomp


def _close(got35, want35, what):
    """The bar every parameter gradient is held to (parity_utils.assert_close at its defaults), per output tensor."""
    for g, w, name in zip(CR.split(got35), CR.split(want35), ("viewmatrix", "projmatrix", "campos")):
        pu.assert_close(torch.from_numpy(np.ascontiguousarray(g)), torch.from_numpy(np.ascontiguousarray(w)), (*what, name))
    assert not np.asarray(got35)[CR.DEAD].any() and not np.asarray(want35)[CR.DEAD].any(), what


@pytest.fixture(scope="module")
def scene():
    return syn.make_scene(P, W, H, seed=0), syn.orbit_camera(W, H, 10.0, -5.0, 7.0)


@pytest.fixture(scope="module")
def planted():
    return G.planted()


# ---- the restatement against the oracle's autograd ---------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("deg", (0, 1, 2, 3))
def test_restatement_matches_the_oracle_on_preprocess(scene, deg, mode):
    sc, cam = scene
    inputs = G.mode_inputs(sc, cam, deg, 1.0, mode)
    records = G.make_records(P, 3 + deg)
    want, pre = CR.oracle_preprocess_camera_grads(inputs, cam, deg, 1.0, records)
    assert 100 < int((pre["radii"] > 0).sum()) < P
    got = CR.camera_rule(inputs, cam, deg, 1.0, records, pre["radii"])
    _close(got, want, ("preprocess", mode, deg))
    campos_lives = mode != "col_sr" and deg > 0
    assert bool(np.abs(want[32:]).max() > 0) == campos_lives and bool(np.abs(got[32:]).max() > 0) == campos_lives


@pytest.mark.parametrize("mode,deg", [("sh_sr", 0), ("sh_sr", 1), ("sh_sr", 2), ("sh_sr", 3), ("col_sr", 3), ("sh_cov", 3)])
def test_restatement_matches_the_oracle_on_the_full_rasterizer(scene, mode, deg):
    sc, cam = scene
    inputs = G.mode_inputs(sc, cam, deg, 1.0, mode)
    want, records, radii = CR.oracle_rasterize_camera_grads(inputs, cam, deg, 1.0, syn.make_upstream_grads(W, H, seed=11))
    got = CR.camera_rule(inputs, cam, deg, 1.0, records, radii)
    _close(got, want, ("rasterize", mode, deg))
    assert np.abs(want[:32]).max() > 0


def test_restatement_matches_the_oracle_on_the_planted_edges(planted):
    """Clamped in x only, in y only and in both, each colour channel's clamp, the low-pass floor of det, culled members."""
    pl = planted
    for mode, deg in (("sh_sr", 3), ("sh_cov", 2), ("col_sr", 1)):
        inputs = pl.inputs(deg, mode)
        records = G.make_records(inputs["means3D"].shape[0], 5)
        want, pre = CR.oracle_preprocess_camera_grads(inputs, pl.cam, deg, pl.mod, records)
        _close(CR.camera_rule(inputs, pl.cam, deg, pl.mod, records, pre["radii"]), want, ("planted", mode, deg))
        for name in G.CULLED:
            assert not bool((pre["radii"][pl.members(name)] > 0).any())
        per = CR.camera_rule(inputs, pl.cam, deg, pl.mod, records, pre["radii"], per_gaussian=True)
        assert not per[(pre["radii"] == 0).numpy()].any()


@pytest.mark.parametrize("mutant", CR.MUTANTS)
def test_the_restatement_tells_each_mutant_apart(planted, mutant):
    pl = planted
    inputs = pl.inputs(3, "sh_sr")
    records = G.make_records(inputs["means3D"].shape[0], 5)
    want, pre = CR.oracle_preprocess_camera_grads(inputs, pl.cam, 3, pl.mod, records)
    _close(CR.camera_rule(inputs, pl.cam, 3, pl.mod, records, pre["radii"]), want, ("planted", "rule"))
    with pytest.raises(AssertionError):
        _close(CR.camera_rule(inputs, pl.cam, 3, pl.mod, records, pre["radii"], mutant=mutant), want, ("planted", mutant))


def test_the_record_map_inverts_the_coefficients(scene):
    sc, cam = scene
    inputs = G.mode_inputs(sc, cam, 3, 1.0, "sh_sr")
    pre = orc_pre = G.oracle_preprocess({k: v for k, v in inputs.items()}, cam, 3, 1.0)
    records = torch.nan_to_num(G.make_records(P, 9)).double()
    k = G.coefficients(orc_pre["conic"].double(), pre["opacity"].double(), records)
    back = CR.records_from_oracle(pre["conic"], pre["opacity"], torch.stack([k["x"], k["y"]], 1), torch.stack([k["a"], k["b"], k["c"]], 1),
                                  k["opacity"], k["depth"], k["rgb"])
    vis = (pre["radii"] > 0).numpy()
    used = list(G.USED_SLOTS)
    assert np.allclose(back[vis][:, used], records.numpy()[vis][:, used], rtol=1e-5, atol=1e-6)


# ---- the ABI -----------------------------------------------------------------------------------------------------------------------
def test_header_text_exports_and_binding_agree():
    abi = abi_compare.check_side_library(_lib_camgrad, "camgrad", "scg_camgrad.h", abi_compare.ANY)
    assert not abi.structs
    assert _lib_camgrad.CAMGRAD_MAX_DIM == 65535 * _lib.TILE and _lib_camgrad.CAMGRAD_OUT_FLOATS == 35


def test_every_argument_code_without_a_launch():
    lib = _lib_camgrad.load()
    err = lib.scg_camgrad_last_error
    nb, pb = C.c_int32(), C.c_uint64()
    for n, blocks in ((0, 0), (1, 1), (256, 1), (257, 2), (2 * 256 + 1, 3)):
        assert lib.scg_camgrad_sizes(n, C.byref(nb), C.byref(pb)) == 0 and (nb.value, pb.value) == (blocks, blocks * 27 * 4)
    assert lib.scg_camgrad_sizes(-1, C.byref(nb), C.byref(pb)) == -2 and b"P = -1" in err()
    assert lib.scg_camgrad_sizes(5, None, C.byref(pb)) == -1 and lib.scg_camgrad_sizes(5, C.byref(nb), None) == -1
    fake = 0x10000

    def call(H=24, W=40, tx=0.5, ty=0.3, mod=1.0, deg=3, M=16, n=300, view=fake, proj=fake, campos=fake, means=fake, opac=fake, shs=fake,
             col=None, scales=fake, rot=fake, cov=None, radii=fake, rec=fake, part=fake, out=fake, flags=0):
        return lib.scg_camgrad_backward(H, W, tx, ty, mod, deg, M, n, view, proj, campos, means, opac, shs, col, scales, rot, cov, radii,
                                        rec, part, out, flags, None)

    assert call(n=-1) == -2
    assert call(H=0) == -2 and call(W=_lib_camgrad.CAMGRAD_MAX_DIM + 1) == -2 and b"image size" in err()
    assert call(deg=4) == -2 and call(deg=-1) == -2 and b"sh_degree" in err()
    assert call(tx=0.0) == -2 and call(ty=float("nan")) == -2 and b"tanfov" in err()
    assert call(flags=2) == -2 and b"flag" in err()
    assert call(view=None) == -1 and call(proj=None) == -1 and call(campos=None) == -1
    assert call(out=None) == -1 and b"out35 is NULL" in err() and call(out=fake + 2) == -5
    assert call(radii=None) == -1 and b"radii is NULL" in err()
    assert call(rec=None) == -1 and call(rec=fake + 4) == -5 and b"dsplats" in err()
    assert call(part=None) == -1 and call(part=fake + 2) == -5 and b"partials" in err()
    assert call(means=None) == -1 and call(opac=None) == -1
    assert call(col=fake) == -3 and call(shs=None) == -3 and b"SHs or precomputed colors" in err()
    assert call(cov=fake) == -3 and call(scales=None) == -3 and call(rot=None) == -3 and call(scales=None, rot=None) == -3
    assert call(M=15) == -2 and call(deg=1, M=3) == -2 and b"(sh_degree+1)^2" in err()
    assert call(rot=fake + 4) == -5 and b"rotations" in err()

    m = _lib.ScgModel()

    def model_call(model=m, n=300, **kw):
        a = dict(H=24, W=40, tx=0.5, ty=0.3, mod=1.0, deg=3, view=fake, proj=fake, campos=fake, radii=fake, rec=fake, part=fake, out=fake,
                 flags=0)
        a.update(kw)
        return lib.scg_camgrad_backward_model(a["H"], a["W"], a["tx"], a["ty"], a["mod"], a["deg"], n, a["view"], a["proj"], a["campos"],
                                              None if model is None else C.byref(model), a["radii"], a["rec"], a["part"], a["out"],
                                              a["flags"], None)

    for f in ("zval", "rayo", "rayd", "features_dc", "features_rest", "opacity", "scaling", "rotation"):
        setattr(m.ray, f, fake)
    for f in ("xyz", "features_dc", "features_rest", "opacity", "scaling", "rotation"):
        setattr(m.bg, f, fake)
    m.ray.count, m.bg.count = 200, 100
    assert model_call(model=None) == -1 and b"model is NULL" in err()
    assert model_call(n=299) == -2 and b"ray.count + bg.count" in err()
    assert model_call(H=0) == -2 and model_call(deg=4) == -2 and model_call(flags=4) == -2 and model_call(view=None) == -1
    assert model_call(rec=fake + 8) == -5 and model_call(part=None) == -1 and model_call(out=None) == -1
    m.ray.count = -1
    assert model_call() == -2
    m.ray.count = 200
    m.ray.zval = None
    assert model_call() == -1 and b"zval / rayo / rayd" in err()
    m.ray.zval, m.bg.xyz = fake, None
    assert model_call() == -1 and b"xyz is NULL" in err()
    m.bg.xyz, m.bg.rotation = fake, fake + 4
    assert model_call() == -5 and b"rotation" in err()
    m.bg.rotation, m.bg.scaling = fake, None
    assert model_call() == -1


def test_python_entry_points_refuse_without_a_gpu(scene):
    from scgaussian_amd import camera_grad
    sc, cam = scene
    st = pu.oracle_settings(cam, 3, (0.0, 0.0, 0.0))
    with pytest.raises(_lib.ScgError, match="ROCm GPU"):
        camera_grad.camera_backward(st, (sc.means3D, sc.opacities, sc.shs, None, sc.scales, sc.rotations, None),
                                    torch.zeros(P, dtype=torch.int32), torch.zeros(P, 16))


# ---- the build ---------------------------------------------------------------------------------------------------------------------
def test_the_library_is_one_entry_of_the_side_library_table():
    assert len(build.SOURCES) == 17 and "camgrad.hip" not in build.SOURCES
    assert abi_compare.side_header("camgrad", "scg_camgrad.h") in build.HEADERS
    assert os.path.join(build.CSRC, "geometry_math.h") in build.HEADERS
    assert build.SIDE_LIBRARIES["camgrad"] == ("camgrad", {"camgrad.hip": ["-ffp-contract=off"]})
    src = open(os.path.join(build.CSRC, "camgrad.hip")).read()
    included = {line.split('"')[1] for line in src.splitlines() if line.startswith('#include "')}
    assert included == {"../../include/camgrad/scg_camgrad.h", "geometry_math.h", "host_align.h", "host_error.h", "reduce.h",
                        "scg_common.h", "sh_eval.h"}
    # one definition of the forward math: geometry.hip includes the header and no longer defines what moved into it
    geo = open(os.path.join(build.CSRC, "geometry.hip")).read()
    math_h = open(os.path.join(build.CSRC, "geometry_math.h")).read()
    assert '#include "geometry_math.h"' in geo
    for name in ("struct Mat16", "struct Proj", "struct GeoIn", "load_geo_in(", "void cov3d_from_scale_rot(", "bool project(", "void cov2d(",
                 "struct TensorSource", "struct ModelSource", "void sh_basis_grads("):
        assert math_h.count(name) == 1 and name not in geo, name


# ---- CameraPose --------------------------------------------------------------------------------------------------------------------
def _exp64(w):
    w = np.asarray(w, dtype=np.float64)
    th = np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    if th == 0:
        return np.eye(3)
    return np.eye(3) + math.sin(th) / th * K + (1 - math.cos(th)) / (th * th) * K @ K


def _pose64(cam, delta):
    wv = cam.world_view_transform.double().numpy()
    R = _exp64(np.asarray(delta[:3], dtype=np.float32)) @ wv[:3, :3].T
    t = wv[3, :3] + np.asarray(delta[3:], dtype=np.float32).astype(np.float64)
    wv2 = np.eye(4)
    wv2[:3, :3], wv2[3, :3] = R.T, t
    proj = syn.projection_matrix(cam.znear, cam.zfar, cam.FoVx, cam.FoVy).double().numpy().T
    return wv2, wv2 @ proj, -R.T @ t


ANGLES = (0.0, 1e-6, 1e-3, 0.1, np.nextafter(np.float32(pose.SERIES_BELOW), np.float32(0)), pose.SERIES_BELOW,
          np.nextafter(np.float32(pose.SERIES_BELOW), np.float32(1)), 1.0, 2.5, 3.1, 6.0)


@pytest.mark.parametrize("angle", ANGLES)
def test_camera_pose_matches_fp64(scene, angle):
    cam = scene[1]
    axis = np.array([0.3, -0.5, 0.8]) / np.linalg.norm([0.3, -0.5, 0.8])
    delta = np.concatenate([axis * float(angle), [0.05, -0.04, 0.06]]).astype(np.float32)
    pc = pose.CameraPose(cam)
    with torch.no_grad():
        pc.delta.copy_(torch.from_numpy(delta))
    want = _pose64(cam, delta)
    got = (pc.world_view_transform, pc.full_proj_transform, pc.camera_center)
    # Exp in fp32: both branches within a few ulp of fp64 (entries of a rotation are at most 1); the products with R0, t0 and the
    # projection add a few more: 16 ulp of the largest entry of each output
    for g, w in zip(got, want):
        assert g.dtype == torch.float32 and tuple(g.shape) == w.shape
        assert np.abs(g.detach().double().numpy() - w).max() <= 16 * 2.0 ** -24 * max(1.0, np.abs(w).max()), (angle, g, w)
    e = np.abs(pose.so3_exp(torch.from_numpy(delta[:3])).double().numpy() - _exp64(delta[:3])).max()
    assert e <= 4 * 2.0 ** -24, (angle, e)
    assert pc.image_width == cam.image_width and pc.FoVx == cam.FoVx and pc.znear == cam.znear      # everything else passes through
    # the gradient is finite everywhere, omega = 0 included, and reaches delta through all three outputs
    (got[0].sum() + got[1].sum() + got[2].sum()).backward()
    assert torch.isfinite(pc.delta.grad).all() and float(pc.delta.grad.abs().min()) > 0


def test_camera_pose_gradient_matches_fp64_autograd_either_side_of_the_switch(scene):
    cam = scene[1]
    for th in (0.0, 0.3, 0.49, 0.51, 2.0):
        w32 = (torch.tensor([0.3, -0.5, 0.8]) / torch.tensor([0.3, -0.5, 0.8]).norm() * th).requires_grad_(True)
        w64 = w32.detach().double().requires_grad_(True)
        c = torch.arange(9.0).reshape(3, 3) / 7.0 - 0.5
        (pose.so3_exp(w32) * c).sum().backward()
        (pose.so3_exp(w64) * c.double()).sum().backward()
        assert (w32.grad.double() - w64.grad).abs().max() <= 1e-5 * max(1.0, float(w64.grad.abs().max())), th


def test_retract_leaves_the_three_matrices_unchanged(scene):
    pc = pose.CameraPose(scene[1])
    with torch.no_grad():
        pc.delta.copy_(torch.tensor([0.2, -0.7, 0.4, 0.3, -0.1, 0.25]))
    before = [t.detach().clone() for t in (pc.world_view_transform, pc.full_proj_transform, pc.camera_center)]
    pc.retract()
    assert not pc.delta.any()
    for b, a in zip(before, (pc.world_view_transform, pc.full_proj_transform, pc.camera_center)):
        assert torch.equal(a.detach(), b)
    assert getattr(pc.world_view_transform, "_scg_camera_id", None) is not None                       # the camera names itself


def test_the_oracles_pose_recovery_loop_ends_below_a_tenth_of_the_initial_error():
    """The premise of tests/test_gpu_camgrad.py's pose recovery: scene and perturbation of examples/fit_pose.py are such that the
    ORACLE's loop (60 Adam steps on delta at 40 x 24 pixels) recovers the pose to below a tenth of its initial error."""
    e0, history, final = CR.fit_pose_module().fit(rasterize=CR.rasterize_oracle, dev="cpu", verbose=False)
    print("pose error: initial", e0, "after 60 iterations", final, history)
    assert 0.05 < e0 < 0.2 and final < 0.1 * e0

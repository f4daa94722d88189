"""tests/geometry_refs.py is right, without a GPU: its fp32 evaluation against the oracle's preprocess (values, decisions and
autograd — the clamped classes included, where the gradient is a decision and not a derivative), its fp64 autograd against
finite differences (the one check that shares a derivation with nothing), and the planted set's premises."""
import numpy as np
import pytest
import torch

import geometry_refs as GR
from scgaussian_amd import synthetic as syn

F32, F64 = torch.float32, torch.float64


@pytest.fixture(scope="module")
def pl():
    return GR.planted()


def _cast(inputs, dtype):
    return {k: v.to(dtype) for k, v in inputs.items()}


def _scenes(pl):
    W, H = 160, 96
    yield "random", syn.make_scene(600, W, H, seed=11, log_scale_mean=-3.0), syn.orbit_camera(W, H, 12.0, -6.0, 7.0), 0.8
    yield "planted", pl.scene, pl.cam, pl.mod


def test_planted_classes_hold_their_premises_and_fp32_decides_as_fp64(pl):
    for mode in ("sh_sr", "sh_cov"):
        ins = pl.inputs(3, mode)
        fw64 = GR.geometry_forward_ref(_cast(ins, F64), pl.cam, 3, pl.mod, mode, F64)
        fw32 = GR.geometry_forward_ref(ins, pl.cam, 3, pl.mod, mode, F32)
        if mode == "sh_sr":
            GR.assert_premises(pl, fw64)
        for k in ("in_front", "cl_x", "cl_y", "det_ok", "tiles_ok", "sh_clamped", "visible", "radii", "rect"):
            assert torch.equal(fw32[k], fw64[k]), (mode, k)
    assert len(pl.cls) == len(GR.CLASSES) * GR.PER_CLASS <= 257
    for deg in range(4):                                   # the SH clamp bits are certain at every degree the GPU tests use
        fw = GR.geometry_forward_ref(_cast(pl.inputs(deg, "sh_sr"), F64), pl.cam, deg, pl.mod, "sh_sr", F64)
        assert GR.sh_margin(fw) > 1e-4, deg


@pytest.mark.parametrize("mode,deg", [("sh_sr", 3), ("col_cov", 3), ("sh_cov", 2), ("col_sr", 1), ("sh_sr", 0)])
def test_fp32_restatement_equals_the_oracle_values_decisions_and_autograd(pl, mode, deg):
    for name, sc, cam, mod in _scenes(pl):
        ins = GR.mode_inputs(sc, cam, deg, mod, mode)
        P = sc.means3D.shape[0]
        rec = GR.make_records(P, seed=3)
        g = GR.geometry_backward_ref(ins, cam, deg, mod, mode, rec, F32)
        o = GR.oracle_backward(ins, cam, deg, mod, mode, rec)
        fw, pre = g["fw"], o["pre"]
        assert torch.equal(fw["radii"], pre["radii"]), name
        vis = pre["visible"]
        assert torch.equal(fw["visible"], vis) and int(vis.sum()) > 0 and int((~vis).sum()) > 0
        assert torch.equal(fw["rect"], pre["rect"] * vis[:, None]), name
        assert torch.equal(fw["sh_clamped"][vis], pre["clamped"][vis]), name
        # the clamp flags as the oracle takes them (it does not return them)
        k = GR.camera_constants(cam, F32)
        m3 = sc.means3D
        V = cam.world_view_transform.reshape(16)
        t = [V[i] * m3[:, 0] + V[4 + i] * m3[:, 1] + V[8 + i] * m3[:, 2] + V[12 + i] for i in range(3)]
        for ax, flag, lim in ((0, fw["cl_x"], k["limx"]), (1, fw["cl_y"], k["limy"])):
            r = t[ax] / t[2]
            assert torch.equal(flag[vis], ((r < -lim) | (r > lim))[vis]), (name, ax)
        for key in ("xy", "depth", "conic", "rgb", "opacity"):
            a, b = fw[key][vis].detach().double(), pre[key][vis].detach().double()
            assert float((a - b).abs().max()) <= 1e-6 * float(b.abs().max()), (name, key)
        for key in GR.OUTPUTS[mode] + ("means2D",):
            a, b = g[key].double(), o[key].double()
            assert bool(torch.isfinite(a).all())
            assert float(a[~vis].abs().max()) == 0.0 and float(b[~vis].abs().max()) == 0.0, (name, key)
            # per Gaussian, relative to that Gaussian's own gradient record: 1e-4 covers the conditioning of the chain at fp32
            # (measured: below 3e-5 everywhere); a wrong term or a wrong clamp decision is O(1)
            e = GR.per_gaussian_error(a, b)
            assert float(e.max()) < 1e-4, (name, key, float(e.max()), int(e.argmax()))
        if "shs" in g:
            K = (deg + 1) ** 2
            assert float(g["shs"][:, K:].abs().max() if K < 16 else 0.0) == 0.0


def _fd(pl, mode, deg):
    """fp64 autograd and second-order finite differences of the per-Gaussian scalar, on the planted set."""
    ins = _cast(pl.inputs(deg, mode), F64)
    P = len(pl.cls)
    rec = GR.make_records(P, seed=5).double()
    g = GR.geometry_backward_ref(ins, pl.cam, deg, pl.mod, mode, rec, F64)
    fw = g["fw"]
    coef = GR.coefficients(fw["conic"], fw["opacity"], rec)
    vis = fw["visible"]

    def terms(inputs, cov_offset=None, want=None):
        with torch.no_grad():
            out = GR.geometry_forward_ref(inputs, pl.cam, deg, pl.mod, mode, F64, cov_offset=cov_offset)
            return out[want] if want else torch.where(vis, GR.contract_terms(out, coef), torch.zeros(P, dtype=F64))
    f0 = terms(ins)
    k = GR.camera_constants(pl.cam, F64)
    z = ins["means3D"][:, 2].abs()
    # step 1e-6 x the input's scale: the depth for a position, the length that projects to the image's width for a scale (the
    # outputs vary with a scale over pixels, whatever its own size: the lowpass class has scales of 1e-5), 1 otherwise
    scale = {"means3D": z[:, None].expand(P, 3), "scales": (z * pl.W / k["fx"])[:, None].expand(P, 3),
             "cov3D_precomp": ((z / k["fx"]) ** 2 * pl.W)[:, None].expand(P, 6)}            # (W square pixels' worth)
    # the members that sit ON a clamp threshold are differentiated one-sidedly, towards the inside of the limit (x, y: towards
    # 0; z: away from the camera): on the other side the component is a constant
    side = {"means3D": torch.zeros(P, 3, dtype=F64)}
    for name in ("edge_x_on", "edge_y_on"):
        m = pl.members(name)
        ax = 0 if name[5] == "x" else 1
        side["means3D"][m, ax] = -torch.sign(ins["means3D"][m, ax])
        side["means3D"][m, 2] = 1.0
    side["means3D"][pl.members("near_over"), 2] = 1.0                  # (one step nearer is behind the cull plane)
    fd = {}
    for n in GR.OUTPUTS[mode]:
        v = ins[n]
        flat = v.reshape(P, -1)
        out = torch.zeros_like(flat)
        h = 1e-6 * scale.get(n, torch.ones_like(flat)).reshape(P, -1)
        sd = side.get(n, torch.zeros_like(flat)).reshape(P, -1)
        for j in range(flat.shape[1]):
            def at(mult):
                p = flat.clone()
                p[:, j] += mult * h[:, j]
                return terms({**ins, n: p.reshape(v.shape)})
            central = (at(1.0) - at(-1.0)) / (2 * h[:, j])
            if bool((sd[:, j] != 0).any()):
                s = sd[:, j]
                one = s * (-3 * f0 + 4 * at(s) - at(2 * s)) / (2 * h[:, j])
                central = torch.where(s != 0, one, central)
            out[:, j] = central
        fd[n] = out.reshape(v.shape)
    if "rotations" in ins:
        # The rotation gradient in TWO finite-difference legs joined by the chain rule at the projected covariance (A, B, C before
        # the low-pass term): d f / d q = sum_m (d f / d cov_m) (d cov_m / d q).  For the lowpass class the one-leg difference
        # cannot work in fp64: T Sigma T^T is 1e-9 of the 0.3 added to it, so a step in q moves f by 1e-9 of its own rounding
        # error times 1e6.  Each leg here is well resolved: cov_m itself is a sum of products with full relative precision, and
        # f varies with cov_m on the scale of 0.3.
        hc = 1e-6 * GR.LOWPASS
        dfdcov = torch.zeros(P, 3, dtype=F64)
        for m in range(3):
            off = torch.zeros(P, 3, dtype=F64)
            off[:, m] = hc
            dfdcov[:, m] = (terms(ins, off) - terms(ins, -off)) / (2 * hc)
        q = ins["rotations"]
        two = torch.zeros(P, 4, dtype=F64)
        for j in range(4):
            step = torch.zeros(P, 4, dtype=F64)
            step[:, j] = 1e-6
            dcov = (terms({**ins, "rotations": q + step}, want="cov2d_raw") - terms({**ins, "rotations": q - step}, want="cov2d_raw")) / 2e-6
            two[:, j] = (dfdcov * dcov).sum(1)
        fd["rotations_two_legs"] = torch.where(vis[:, None], two, torch.zeros_like(two))
    return g, fd, fw


@pytest.mark.parametrize("mode,deg", [("sh_sr", 3), ("col_cov", 3)])
def test_fp64_autograd_equals_finite_differences_for_every_class_without_an_active_clamp(pl, mode, deg):
    g, fd, fw = _fd(pl, mode, deg)
    for name in GR.CLASSES:
        if name in GR.CLAMPED or name in GR.CULLED:
            continue
        m = pl.members(name)
        assert not bool((fw["cl_x"] | fw["cl_y"])[m].any())
        for n in GR.OUTPUTS[mode]:
            # the one exception to the plain difference: the lowpass class's rotation gradient, taken in two legs (see _fd)
            got = fd["rotations_two_legs"] if (name, n) == ("lowpass", "rotations") else fd[n]
            zero = g[n][m].reshape(len(m), -1).abs().max(1).values == 0         # opacity 0, all three SH channels clamped:
            assert torch.equal(got[m][zero], torch.zeros_like(got[m][zero])), (name, n)   # the difference is exactly 0 too
            e = GR.per_gaussian_error(got[m], g[n][m])
            print(f"FD {mode} {name} {n}: worst err {float(e.max()):.2e}")
            assert float(e.max()) < 1e-6, (name, n, float(e.max()))
    for name in GR.CULLED:                                              # nothing depends on a culled Gaussian's inputs
        m = pl.members(name)
        for n in fd:
            assert float(fd[n][m].abs().max()) == 0.0 and float(g[n.replace("_two_legs", "")][m].abs().max()) == 0.0


def test_a_clamped_component_is_a_constant_of_the_covariance_and_not_of_the_pixel_position(pl):
    ins = _cast(pl.inputs(3, "sh_sr"), F64)
    rec = GR.make_records(len(pl.cls), seed=5).double()
    probe, probe_off = {}, {}
    g = GR.geometry_backward_ref(ins, pl.cam, 3, pl.mod, "sh_sr", rec, F64, probe=probe)
    off = GR.geometry_backward_ref(ins, pl.cam, 3, pl.mod, "sh_sr", rec, F64, clamp_off=("x", "y"), probe=probe_off)
    tv, tv_off = probe["tview"].grad, probe_off["tview"].grad
    for name in GR.CLAMPED:
        m = pl.members(name)
        for ax, flag in ((0, g["fw"]["cl_x"][m]), (1, g["fw"]["cl_y"][m])):
            if not bool(flag.any()):
                assert torch.equal(g["means3D"][m, ax], off["means3D"][m, ax])
                continue
            assert bool(flag.all())
            assert bool((tv[m, ax] == 0).all()), name                                     # through the covariance: exactly 0
            assert bool((tv_off[m, ax] != 0).all()), name                                 # ... which is the clamp's doing
            assert bool((g["means3D"][m, ax] != 0).all()), name                           # through the pixel position: not 0
            # the view matrix is the identity: the two differ by the covariance path's term and by nothing else
            assert torch.allclose(off["means3D"][m, ax] - g["means3D"][m, ax], tv_off[m, ax], rtol=1e-12, atol=1e-15)
            assert torch.equal(off["means3D"][m, 2], g["means3D"][m, 2]), name            # d/dt_z uses the clamped value either way
        for n in ("scales", "rotations", "shs", "opacities", "means2D"):
            assert torch.equal(g[n][m], off[n][m])
        assert float(g["means2D"][m, :2].abs().min()) > 0


def test_opacity_zero_and_culled_gaussians_give_exact_zeros(pl):
    for dtype in (F32, F64):
        g = GR.geometry_backward_ref(pl.inputs(3, "sh_sr"), pl.cam, 3, pl.mod, "sh_sr", GR.make_records(len(pl.cls), 9), dtype)
        m = pl.members("opacity_edges")
        zero = m[pl.scene.opacities[m, 0] == 0]
        assert len(zero) >= 5 and float(g["opacities"][zero].abs().max()) == 0.0
        assert float(g["opacities"][m[pl.scene.opacities[m, 0] > 0]].abs().min()) > 0
        for n, v in g.items():
            if n != "fw":
                assert bool(torch.isfinite(v).all()), n
                assert float(v[g["fw"]["radii"] == 0].abs().max()) == 0.0, n
        assert float(g["means2D"][:, 2].abs().max()) == 0.0

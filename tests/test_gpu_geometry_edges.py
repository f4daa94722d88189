"""The geometry stage ALONE (csrc/geometry.hip) on the planted set of tests/geometry_refs.py: clamp, cull and record edges.

Forward: the staged entry against the oracle's preprocess, bit for bit where the suite asks for bits, on every class.
Backward: scg_geometry_backward is called directly with gradient records of the test's own making (every used slot non-zero,
the unused ones NaN) and held to the fp64 restatement through loss_refs.held_to: per class and per output tensor,
err = max_i |hip_i - r64_i|_inf / |r64_i|_inf <= max(4 e32, 1e-6), e32 the larger of two independent fp32 evaluations of the
same reference (the restatement at fp32; the oracle's preprocess, which keeps the kernel's operation order, under autograd).
The stage has no atomics: nothing here allows for summation-order noise.  Every kernel form, the record counts around the
workgroup sizes, and both flags.  Model kernel: through render(), against autograd through the reference getters and the oracle.
"""
import functools

import numpy as np
import pytest
import torch

import geometry_refs as GR
import loss_refs as LR
import model_refs as MR
import parity_utils as pu
from oracle import torch_rasterizer as orc
from scgaussian_amd import _lib
from scgaussian_amd import model_path as mp
from scgaussian_amd import rasterizer as R
from scgaussian_amd import render as rmod
from scgaussian_amd import synthetic as syn

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, F64 = torch.float32, torch.float64
GRAD_NAMES = ("means3D", "means2D", "opacities", "shs", "colors_precomp", "scales", "rotations", "cov3D_precomp")

# (name, mode, degree, M): every form of the backward kernel
FORMS_60 = [("sh_sr-M16-d3", "sh_sr", 3, 16),            # staged, records staged in through LDS
            ("sh_sr-M16-d0", "sh_sr", 0, 16), ("sh_sr-M16-d1", "sh_sr", 1, 16), ("sh_sr-M16-d2", "sh_sr", 2, 16),     # staged out only
            ("sh_cov-M16-d3", "sh_cov", 3, 16)]
FORMS_256 = [("sh_sr-M9-d2", "sh_sr", 2, 9), ("sh_sr-M4-d1", "sh_sr", 1, 4),      # short records: the 256-thread form
             ("col_sr", "col_sr", 3, 0), ("col_cov", "col_cov", 3, 0)]              # no SH records
COUNTS = {60: (1, 59, 60, 61, 119, 120, 121), 256: (1, 255, 256, 257)}


@functools.lru_cache(maxsize=None)
def _planted():
    return GR.planted()


# (shared with tests/test_gpu_model_kernel_edges.py: they live in tests/model_refs.py)
_interleaved, _layout, _model_members, _raw_model = MR.interleaved, MR.layout, MR.model_members, MR.raw_model


def _inputs(pl, deg, mode, M):
    ins = dict(pl.inputs(deg, mode))
    if "shs" in ins and M < 16:
        ins["shs"] = ins["shs"][:, :M].contiguous()
    return ins


@functools.lru_cache(maxsize=None)
def _reference(mode, deg, M):
    """Per Gaussian of the planted set, computed once per form: the records (scaled so that every Gaussian's largest fp64 output
    gradient is 1), the fp64 gradients, and e32 per Gaussian and output (the larger of two fp32 evaluations' errors)."""
    pl = _planted()
    ins = _inputs(pl, deg, mode, M)
    P = len(pl.cls)
    raw = GR.make_records(P, seed=100 + deg + 10 * M)
    names = GR.OUTPUTS[mode] + ("means2D",)
    rec, _ = GR.normalise_records(raw, GR.geometry_backward_ref(ins, pl.cam, deg, pl.mod, mode, raw, F64), names)
    g64 = GR.geometry_backward_ref(ins, pl.cam, deg, pl.mod, mode, rec, F64)
    g32 = GR.geometry_backward_ref(ins, pl.cam, deg, pl.mod, mode, rec, F32)
    o32 = GR.oracle_backward(ins, pl.cam, deg, pl.mod, mode, rec)
    fw = g64["fw"]
    assert torch.equal(fw["radii"], o32["pre"]["radii"]) and torch.equal(fw["radii"], g32["fw"]["radii"])
    e32 = {n: torch.maximum(GR.per_gaussian_error(g32[n], g64[n]), GR.per_gaussian_error(o32[n], g64[n])) for n in names}
    for n in names:
        assert bool(torch.isfinite(e32[n]).all()), n
    return dict(ins=ins, rec=rec, g64={n: g64[n] for n in names}, e32=e32, fw=fw, names=names, deg=deg)


def _call_backward(st, dev_in, mode, radii, clamped, records, flags=0, prefill=None):
    """lib.scg_geometry_backward with pointers passed the way the binding's backward passes them.  prefill: {name: tensor} the
    outputs start from (default: NaN everywhere — an element the kernel does not write shows).  Returns {name: output}."""
    lib = _lib.load()
    P = dev_in["means3D"].shape[0]
    M = dev_in["shs"].shape[1] if "shs" in dev_in else 0
    fr = R._frame_for(st, P, M, torch.device(DEV, torch.cuda.current_device()))
    shapes = dict(means3D=(P, 3), means2D=(P, 3), opacities=dev_in["opacities"].shape, shs=(P, M, 3), colors_precomp=(P, 3),
                  scales=(P, 3), rotations=(P, 4), cov3D_precomp=(P, 6))
    out = {}
    for n in GR.OUTPUTS[mode] + ("means2D",):
        out[n] = torch.full(shapes[n], float("nan"), dtype=F32, device=DEV) if prefill is None else prefill[n].clone()
    in_ptrs = tuple(R.ptr(dev_in.get(n)) for n in ("means3D", "opacities", "shs", "colors_precomp", "scales", "rotations", "cov3D_precomp"))
    grads = tuple(R.ptr(out.get(n)) for n in GRAD_NAMES)
    dev = dev_in["means3D"].device
    R.check(lib.scg_geometry_backward(fr.ref, *in_ptrs, radii.data_ptr(), clamped.data_ptr(), records.data_ptr(), *grads,
                                      int(flags), R._stream(dev)), "scg_geometry_backward")
    torch.cuda.synchronize()
    return out


def _forward(sub, deg, mode, M):
    st = pu.hip_settings(sub.cam, deg, (0.0, 0.0, 0.0), sub.mod)
    dev_in = {k: v.to(DEV).contiguous() for k, v in _inputs(sub, deg, mode, M).items()}
    fs = R.forward_stages(st, dev_in["means3D"], dev_in["opacities"], shs=dev_in.get("shs"), colors_precomp=dev_in.get("colors_precomp"),
                          scales=dev_in.get("scales"), rotations=dev_in.get("rotations"), cov3D_precomp=dev_in.get("cov3D_precomp"))
    torch.cuda.synchronize()
    return st, dev_in, fs


def _run(form, idx, flags=0, prefill=None):
    """Forward of the planted members `idx` in the form's mode, then the backward alone on the form's records of those members."""
    name, mode, deg, M = form
    pl, ref = _planted(), _reference(mode, deg, M)
    sub = pl.subset(idx)
    st, dev_in, fs = _forward(sub, deg, mode, M)
    assert torch.equal(fs["radii"].cpu(), ref["fw"]["radii"][idx]), name          # the forward's decisions are the reference's
    rec = ref["rec"][idx].contiguous().to(DEV)
    out = _call_backward(st, dev_in, mode, fs["radii"], fs["clamped"], rec, flags, prefill)
    return sub, ref, fs, out, (st, dev_in, rec)


def _hold(tag, sub, ref, idx, out):
    """held_to per class present in `sub` and per output tensor."""
    cls = np.array(sub.cls)
    for n in ref["names"]:
        e = GR.per_gaussian_error(out[n].cpu(), ref["g64"][n][idx])
        e32 = ref["e32"][n][idx]
        for c in sorted(set(sub.cls)):
            m = torch.from_numpy(cls == c)
            LR.held_to(f"geometry backward {tag} {c} {n}", float(e[m].max()), float(e32[m].max()), LR.GRAD_FLOOR, elements=int(m.sum()))


def _exact_statements(sub, ref, idx, out):
    culled = torch.from_numpy(np.isin(np.array(sub.cls), GR.CULLED))
    assert bool((ref["fw"]["radii"][idx][culled] == 0).all()) and bool((ref["fw"]["radii"][idx][~culled] > 0).all())
    for n, v in out.items():
        v = v.cpu()
        assert bool(torch.isfinite(v).all()), n                                  # (the NaN of the unused record slots reached nothing)
        if bool(culled.any()):
            assert float(v[culled].abs().max()) == 0.0, n                            # radius 0: exactly 0 everywhere
    assert float(out["means2D"][:, 2].abs().max()) == 0.0
    op0 = (sub.scene.opacities.reshape(-1) == 0)
    if bool(op0.any()):
        assert float(out["opacities"].cpu().reshape(-1)[op0].abs().max()) == 0.0    # opacity 0: dL/dopacity is 0, not inf or NaN
    if "shs" in out:
        K = (ref["deg"] + 1) ** 2
        if K < out["shs"].shape[1]:
            assert float(out["shs"][:, K:].abs().max()) == 0.0                    # SH gradients above the active degree


# ------------------------------------------------------------------------------------------------------------------- forward

@pytest.mark.parametrize("mode,deg", [("sh_sr", 3), ("col_sr", 3), ("sh_cov", 3), ("col_cov", 3), ("sh_sr", 0), ("sh_sr", 1), ("sh_sr", 2)])
def test_forward_on_the_planted_set_equals_the_oracle_bit_for_bit(mode, deg):
    pl = _planted()
    st, dev_in, fs = _forward(pl, deg, mode, 16)
    pre = GR.oracle_preprocess(_inputs(pl, deg, mode, 16), pl.cam, deg, pl.mod)
    vis = pre["visible"].numpy()
    radii = fs["radii"].cpu()
    assert torch.equal(radii, pre["radii"])
    for c in GR.CLASSES:                                                         # the classes are what they were planted as
        assert bool((radii[pl.members(c)] > 0).all()) != (c in GR.CULLED) and bool((radii[pl.members(c)] == 0).all()) == (c in GR.CULLED), c
    rect = pre["rect"].numpy().astype(np.int64)
    want = np.stack([rect[:, 0] | (rect[:, 1] << 16), (rect[:, 2] - rect[:, 0]) | ((rect[:, 3] - rect[:, 1]) << 16)], 1) * vis[:, None]
    assert np.array_equal(pu.as_u32(fs["rects"]).astype(np.int64), want)
    keys = pu.as_u32(fs["depth_keys"])
    assert np.array_equal(keys[vis], pre["depth"].detach().numpy().view(np.uint32)[vis]) and np.all(keys[~vis] == 0xFFFFFFFF)
    cl = fs["clamped"].cpu().numpy()
    bits = (pre["clamped"].numpy().astype(np.uint8) * np.array([1, 2, 4], dtype=np.uint8)[None]).sum(1).astype(np.uint8)
    assert np.array_equal(cl[vis], bits[vis]) and np.all(cl[~vis] == 0)
    if mode.startswith("sh") and deg == 3:
        assert set(np.unique(cl[pl.members("sh_neg").numpy()])) >= {1, 2, 3, 5, 7}   # one, two and three channels clamped
    sp = fs["splats"].cpu().numpy()
    assert np.array_equal(sp[vis, 0:2], pre["xy"].detach().numpy()[vis])
    assert np.array_equal(sp[vis, 2:5], pre["conic"].detach().numpy()[vis])
    assert np.array_equal(sp[vis, 5], pre["opacity"].detach().numpy()[vis])
    assert np.array_equal(sp[vis, 11], pre["depth"].detach().numpy()[vis])
    assert pu.nrm_err(sp[vis, 8:11], pre["rgb"].detach().numpy()[vis]) < 1e-6


# ------------------------------------------------------------------------------------------------------------ backward alone

@pytest.mark.parametrize("form", FORMS_60 + FORMS_256, ids=lambda f: f[0])
def test_backward_alone_holds_every_class_to_fp64(form):
    pl = _planted()
    idx = torch.tensor(_interleaved(pl), dtype=torch.long)
    sub, ref, fs, out, (st, dev_in, rec) = _run(form, idx)
    _exact_statements(sub, ref, idx, out)
    again = _call_backward(st, dev_in, form[1], fs["radii"], fs["clamped"], rec)
    for n in out:
        assert torch.equal(out[n], again[n]), n                                   # no atomics in this stage: the same bits
    _hold(form[0], sub, ref, idx, out)


@pytest.mark.parametrize("form,block", [(f, 60) for f in FORMS_60] + [(f, 256) for f in FORMS_256],
                         ids=[f[0] for f in FORMS_60 + FORMS_256])
def test_backward_alone_at_the_record_count_edges(form, block):
    pl = _planted()
    cases = [(P, False) for P in COUNTS[block]] + [(2 * block + 1 if block == 60 else block + 1, True)]
    for P, all_culled in cases:
        idx = _layout(pl, P, block, all_culled)
        sub, ref, fs, out, _ = _run(form, idx)
        if all_culled:
            assert int((fs["radii"][:block] > 0).sum()) == 0 and int((fs["radii"][block:] > 0).sum()) > 0
        _exact_statements(sub, ref, idx, out)
        _hold(f"{form[0]} P={P}{' first workgroup culled' if all_culled else ''}", sub, ref, idx, out)
    # a single VISIBLE Gaussian (P = 1 above is the culled member the layout puts first)
    idx = pl.members("clamp_x")[:1]
    sub, ref, fs, out, _ = _run(form, idx)
    assert int(fs["radii"][0]) > 0
    _hold(f"{form[0]} P=1 visible", sub, ref, idx, out)


@pytest.mark.parametrize("form", [FORMS_60[0], FORMS_256[2]], ids=lambda f: f[0])
def test_a_clamped_component_gets_the_gradient_of_a_constant(form):
    """clamp_x / clamp_y members: the kernel's position gradient is the fp64 reference's with the clamp ON and differs from the
    reference's with the clamp flag ignored by what the reference says the flag is worth (two fp64 numbers)."""
    name, mode, deg, M = form
    pl = _planted()
    idx = torch.tensor(_interleaved(pl), dtype=torch.long)
    sub, ref, fs, out, _ = _run(form, idx)
    for cls, ax in (("clamp_x", 0), ("clamp_y", 1), ("edge_x_over", 0), ("edge_y_over", 1)):
        m = torch.from_numpy(np.array(sub.cls) == cls)
        off = GR.geometry_backward_ref(ref["ins"], pl.cam, deg, pl.mod, mode, ref["rec"], F64, clamp_off=("x", "y")[ax])["means3D"][idx][m]
        on = ref["g64"]["means3D"][idx][m]
        got = out["means3D"].cpu().double()[m]
        norm = on.abs().max(1).values
        gap = ((off - on)[:, ax].abs() / norm).max()                              # what ignoring the flag would change
        err_on = float(((got - on)[:, ax].abs() / norm).max())
        err_off = float(((got - off)[:, ax].abs() / norm).max())
        e32 = float(ref["e32"]["means3D"][idx][m].max())
        bar = max(LR.FACTOR * e32, LR.GRAD_FLOOR)
        print(f"clamp {name} {cls}: flag worth {float(gap):.3e}, |hip - on| {err_on:.3e}, |hip - off| {err_off:.3e}, bar {bar:.3e}")
        assert float(gap) > 100 * bar, (cls, float(gap), bar)                     # premise: the flag matters at this bar
        LR.held_to(f"geometry backward {name} {cls} means3D[{ax}] clamp on", err_on, e32, LR.GRAD_FLOOR)
        assert err_off > 0.5 * float(gap), (cls, err_off, float(gap))
        assert torch.equal(off[:, 2], on[:, 2])                                   # d/dz uses the clamped value either way


@pytest.mark.parametrize("form", [FORMS_60[0], FORMS_60[2], FORMS_60[4], FORMS_256[0], FORMS_256[3]], ids=lambda f: f[0])
def test_accumulate_adds_to_every_parameter_gradient_and_overwrites_means2D(form):
    pl = _planted()
    P = 121 if form in FORMS_60 else 257
    idx = _layout(pl, P, 60 if form in FORMS_60 else 256)
    sub, ref, fs, base, (st, dev_in, rec) = _run(form, idx)
    g = torch.Generator().manual_seed(41)
    prior = {n: torch.randn(v.shape, generator=g).to(DEV) for n, v in base.items()}
    acc = _call_backward(st, dev_in, form[1], fs["radii"], fs["clamped"], rec, _lib.BACKWARD_ACCUMULATE, prior)
    culled = (fs["radii"] == 0)
    assert int(culled.sum()) > 0
    for n in base:
        if n == "means2D":
            assert torch.equal(acc[n], base[n])                                   # per view: overwritten, not added
            continue
        want = prior[n] + base[n]                                                 # one fp32 addition per element, as in the kernel
        ulp = torch.finfo(F32).eps * want.abs()
        assert bool(((acc[n] - want).abs() <= ulp).all()), n
        assert torch.equal(acc[n][culled], prior[n][culled]), n                   # culled: exactly the prior
        assert not torch.equal(acc[n][~culled], prior[n][~culled]), n


@pytest.mark.parametrize("form", FORMS_60[1:4] + FORMS_256[:1], ids=lambda f: f[0])
def test_sh_tail_zero_leaves_the_tails_alone_and_writes_the_same_bits(form):
    pl = _planted()
    deg = form[2]
    K = (deg + 1) ** 2
    idx = _layout(pl, 121, 60)
    sub, ref, fs, base, (st, dev_in, rec) = _run(form, idx)
    prefill = {n: torch.full_like(v, float("nan")) for n, v in base.items()}
    prefill["shs"] = torch.zeros_like(base["shs"])                                # the promise: the tails hold zeros ...
    prefill["shs"][:, :K] = 777.0                                                 # ... and the active coefficients anything
    got = _call_backward(st, dev_in, form[1], fs["radii"], fs["clamped"], rec, _lib.BACKWARD_SH_TAIL_ZERO, prefill)
    for n in base:
        assert torch.equal(got[n], base[n]), n
    assert float(base["shs"][:, :K].abs().max()) > 0


# -------------------------------------------------------------------------------------------------------------- model kernel

@pytest.mark.parametrize("deg", [0, 3])
@pytest.mark.parametrize("n_ray", [120, 0, 61, 1])
def test_model_kernel_on_the_planted_set_equals_autograd_through_the_getters_and_the_oracle(deg, n_ray):
    pl = _planted()
    idx = _model_members(pl)
    P = len(idx)
    sub = pl.subset(idx)
    model = _raw_model(pl, idx, n_ray)
    model.active_sh_degree = deg
    # CPU: through the reference getters the decisions are the planted ones (no member had to be dropped: the positions of
    # the threshold members are reproduced exactly, and no other decision is within the activations' rounding of flipping)
    ins = dict(means3D=model.get_xyz, opacities=model.get_opacity, shs=model.get_features, scales=model.get_scaling,
               rotations=model.get_rotation)
    want = GR.geometry_forward_ref({k: v.double() for k, v in sub.inputs(deg, "sh_sr").items()}, pl.cam, deg, pl.mod, "sh_sr", F64)
    have = GR.geometry_forward_ref(ins, pl.cam, deg, pl.mod, "sh_sr", F32)
    for k in ("in_front", "cl_x", "cl_y", "det_ok", "tiles_ok", "sh_clamped", "visible"):
        assert torch.equal(have[k], want[k]), k
    for prefix, comps in (("edge_x", (0, 2)), ("edge_y", (1, 2)), ("near_", (2,))):
        m = torch.from_numpy(np.char.startswith(np.array(sub.cls), prefix))
        assert int(m.sum()) > 0 and torch.equal(model.get_xyz[m][:, comps], sub.scene.means3D[m][:, comps]), prefix
    cam, bg = pl.cam, (0.1, 0.2, 0.3)
    grads = syn.make_upstream_grads(pl.W, pl.H, seed=5)
    md = model.to(DEV)
    md.requires_grad_()
    md.active_sh_degree = deg
    act = mp.activate(**mp.tensors_of(md))
    # oracle side as in test_gpu_model_path.py (reference getters under autograd, values replaced by the kernels')
    leaves, inputs = pu.model_oracle_side(model, act)
    m2 = torch.zeros(P, 3, requires_grad=True)
    oc, orad, od, oa = orc.rasterize(inputs["means3D"], m2, inputs["opacities"], pu.oracle_settings(cam, deg, bg, pl.mod),
                                     shs=inputs["shs"], scales=inputs["scales"], rotations=inputs["rotations"])
    ((oc * grads[0]).sum() + (od * grads[1]).sum() + (oa * grads[2]).sum()).backward()
    assert rmod.model_fast_path_available(md, rmod.PipelineParams())
    out = rmod.render(cam.to(DEV), md, rmod.PipelineParams(), torch.tensor(bg, device=DEV), scaling_modifier=pl.mod)
    loss = (out["render"] * grads[0].to(DEV)).sum() + (out["rendered_depth"] * grads[1].to(DEV)).sum() + \
        (out["rendered_alpha"] * grads[2].to(DEV)).sum()
    loss.backward()
    torch.cuda.synchronize()
    assert torch.equal(out["radii"].cpu(), orad)
    culled = torch.from_numpy(np.isin(np.array(sub.cls), GR.CULLED))
    assert torch.equal(orad == 0, culled)
    pu.assert_close(out["viewspace_points"].grad, m2.grad, ("planted model backward", deg, n_ray, "means2D"))
    names = ["zval", "features_dc", "features_rest", "opacity", "scaling", "rotation"] if n_ray else []
    names += ["bg_xyz", "bg_features_dc", "bg_features_rest", "bg_opacity", "bg_scaling", "bg_rotation"] if n_ray < P else []
    for n in names:
        g_hip, g_ref = getattr(md, n).grad, getattr(leaves, n).grad
        assert g_hip is not None and g_ref is not None, n
        sel = culled[n_ray:] if n.startswith("bg_") else culled[:n_ray]
        assert float(g_hip.cpu()[sel].abs().max() if bool(sel.any()) else 0.0) == 0.0, n
        if "rest" in n and deg == 0:
            assert float(g_ref.abs().max()) == 0.0 and float(g_hip.abs().max()) == 0.0, n
        else:
            assert float(g_ref.abs().max()) > 0, n
            pu.assert_close(g_hip, g_ref, ("planted model backward", deg, n_ray, n))
    # per class: a clamped Gaussian's position gradient is not zero and is the oracle's — the statement the suite lacked
    cls = np.array(sub.cls)
    for c in GR.CLAMPED:
        for n, sl in (("zval", slice(0, n_ray)), ("bg_xyz", slice(n_ray, P))):
            m = torch.from_numpy(cls[sl] == c)
            if not bool(m.any()):
                continue
            g_hip, g_ref = getattr(md, n).grad.cpu()[m], getattr(leaves, n).grad[m]
            assert float(g_ref.abs().max()) > 0 and float(g_hip.abs().max()) > 0, (c, n)
            pu.assert_close(g_hip, g_ref, ("planted model backward", deg, n_ray, c, n))

"""The model-path geometry kernels ALONE (csrc/geometry.hip: geometry_hist_model_kernel / geometry_forward_model_kernel,
geometry_backward_model_kernel, model_activate_kernel) on the pool of tests/model_refs.py: the planted clamp / cull classes as a
raw model plus the value classes, at the set edges (P = 181 and 120, every split of model_refs.SIZES) and at every SH degree.

Part A, forward: scg_forward_model against scg_forward on scg_model_activate's outputs, the same capacity, every output and every
field of the workspace the forward writes, as raw bits.  The two geometry kernels are two instantiations of one body
(geometry_forward_one) over two sources; the model source activates in registers with the device functions scg_model_activate
stores the results of, and the file is compiled with contraction off, so no operation differs and no field needed a tolerance.

Part B, backward: there is no staged entry for the model backward, so scg_backward_model runs on the state of a model forward with
an all-zero dL/dcolor, no dL/ddepth and dL/dalpha, and `dsplats` = records of the test's own making (GR.make_records: used slots
non-zero, unused ones NaN) declared pre-zeroed.  Every sum the blend backward adds carries a factor of the upstream gradient, so it
adds signed zeros and the geometry kernel reads the planted records.  The first test pins that premise on the tensor path, where
the stage CAN be called alone; every backward of this file re-reads its record buffer and compares it with the planted words.
No member of the pool broke the premise (none had to be left out).

Bar: loss_refs.held_to(err, e32, GRAD_FLOOR) = max(4 e32, 1e-6) per class (sub-classes ':sat', ':iso', ':disc': tests/model_refs.py) and
per output (zval | bg_xyz, features_dc, features_rest, opacity, scaling, rotation of either set, means2D), err =
max_i |hip_i - r64_i|_inf / |r64_i|_inf over the class's members (two outputs take another denominator, for reasons of
conditioning that tests/model_refs.py states with the measured numbers: dL/dzval, and dL/drotation of the ':iso' members; the
scale gradient of the ':disc' members has an e32 that includes the rounding of the stage's inputs).  No element is left out and no share is allowed for: the stage has
no atomics.  Every gradient buffer lies between guard bands (guarded_alloc, both fills).
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import guarded_alloc as GA
import loss_refs as LR
import model_refs as MR
import parity_utils as pu
from scgaussian_amd import _lib
from scgaussian_amd import model_path as mp
from scgaussian_amd import rasterizer as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32 = torch.float32
SENTINEL = 0x4B1D5EED                                         # a finite float no gradient of these scenes equals
CASES = [(P, n) for P in (181, 120) for n in MR.SIZES[P]]


def _bits(t):
    return t.detach().contiguous().cpu().view(torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


class _Scene:
    """One model of the pool on the device and its forward through scg_forward_model."""

    def __init__(self, deg, P, n_ray, bg_all_culled_first=False):
        pl = MR.pool()
        self.deg, self.P, self.n_ray, self.pl = deg, P, n_ray, pl
        self.idx = MR.scene_layout(pl, P, n_ray, MR.case_start(P, n_ray), bg_all_culled_first)
        self.labels = np.array(pl.labels(self.idx))
        self.ref = MR.case_reference(deg, self.idx, n_ray)
        self.sets = [(p, sl) for p, sl in (("ray", slice(0, n_ray)), ("bg", slice(n_ray, P))) if sl.stop > sl.start]
        self.st = pu.hip_settings(pl.cam, deg, (0.0, 0.0, 0.0), pl.mod)
        self.model = pl.model(self.idx, n_ray).to(DEV)
        self.tensors = mp.tensors_of(self.model)
        self.args = mp._ModelArgs(self.tensors)
        out = R.forward_fused(self.st, None, None, None, None, None, None, None, True, model=self.args)
        assert out is not None
        torch.cuda.synchronize()
        self.color, self.radii, self.depth, self.alpha, self.state = out
        self.H, self.W = pl.H, pl.W
        # admission, again: the kernel's decisions are the ones all three CPU evaluations agree on
        assert torch.equal(self.radii.cpu(), self.ref["radii"]), (deg, P, n_ray)
        assert torch.equal(self.field(self.state, "clamped"), self.ref["clamp_bits"]), (deg, P, n_ray)
        self.culled = self.ref["radii"] == 0
        for p, sl in () if bg_all_culled_first else self.sets:   # a culled member first and last in either set
            assert bool(self.culled[sl.start]) and bool(self.culled[sl.stop - 1]), (p, n_ray)

    def field(self, state, name):
        """A field of ScgWorkspaceLayout as the forward of `state` left it (CPU; floats as int32 words)."""
        ws, plan, P, hw = state["ws"], state["plan"], self.P, self.H * self.W
        n_tiles = ((self.W + 15) // 16) * ((self.H + 15) // 16)
        count = int(state["num_rendered"])
        off, n, dtype = {"splats": (plan.splats, 12 * P, torch.int32), "rects": (plan.rects, 2 * P, torch.int32),
                         "depth_keys": (plan.depth_keys, P, torch.int32), "clamped": (plan.clamped, P, torch.uint8),
                         "ranges": (plan.ranges, 2 * n_tiles, torch.int32), "point_list": (plan.point_list, count, torch.int32),
                         "final_T": (plan.final_T, hw, torch.int32), "n_contrib": (plan.n_contrib, hw, torch.int32)}[name]
        return ws[off: off + n * dtype.itemsize].view(dtype).cpu()

    def names(self, p):
        return MR.out_names(p)[:-1]

    def backward(self, flags=0, prefill=None, fill=GA.FILL_A):
        """scg_backward_model on this forward's state with the planted records.  prefill: None (NaN everywhere — an element the
        kernel does not write shows) or {name: CPU tensor}.  Every gradient buffer and the record buffer lie between guard bands
        of `fill`.  Returns {name: CPU tensor} (means2D: (P,3))."""
        lib = _lib.load()
        P, dev = self.P, torch.device(DEV, torch.cuda.current_device())
        with GA.guarded(fill) as reg:
            out = {}
            for p, sl in self.sets:
                for n in self.names(p):
                    out[n] = torch.empty(tuple(getattr(self.model, n).shape), dtype=F32, device=DEV)
            out["means2D"] = torch.empty((P, 3), dtype=F32, device=DEV)
            for n, v in out.items():
                if prefill is None:
                    v.fill_(float("nan"))
                else:
                    v.copy_(prefill[n])
            rec = torch.empty((P, 16), dtype=F32, device=DEV)
            rec.copy_(self.ref["rec"])
            dcol = torch.zeros((3, self.H, self.W), dtype=F32, device=DEV)
        g = _lib.ScgModelGrads()
        for n, v in out.items():
            if n != "means2D":
                setattr(g.bg if n.startswith("bg_") else g.ray, n[3:] if n.startswith("bg_") else n, v.data_ptr())
        st = self.state
        R.check(lib.scg_backward_model(st["frame"].ref, self.args.ref, self.radii.data_ptr(), st["cap"], st["ws"].data_ptr(),
                                       dcol.data_ptr(), None, None, rec.data_ptr(), 1, C.byref(g), out["means2D"].data_ptr(),
                                       int(flags), None, R._stream(dev)), "scg_backward_model")
        torch.cuda.synchronize()
        assert reg.check() == [], (self.deg, P, self.n_ray, flags)                 # no store past a buffer's end or before its start
        assert torch.equal(_bits(rec), _bits(self.ref["rec"])), "the blend backward changed a planted record"
        return {n: v.cpu() for n, v in out.items()}

    def rows(self, out, p, n):
        sl = dict(self.sets)[p]
        return out[n][sl] if n == "means2D" else out[n]

    def hold(self, tag, out):
        """held_to per (sub-)class present and per output of either set; every miss of the case is reported, not the first alone."""
        missed = []
        for p, sl in self.sets:
            labels = self.labels[sl]
            for n in MR.out_names(p):
                want, e32, scale = self.ref["sets"][p][n]
                e = MR.gaussian_error(self.rows(out, p, n), want, scale)
                for c in sorted(set(labels)):
                    m = torch.from_numpy(labels == c)
                    try:
                        LR.held_to(f"model backward {tag} {c} {p}.{n}", float(e[m].max()), float(e32[m].max()), LR.GRAD_FLOOR,
                                   elements=int(m.sum()))
                    except AssertionError as err:
                        missed.append(err.args[0])
        assert not missed, missed

    def exact_statements(self, out):
        K = (self.deg + 1) ** 2
        for n, v in out.items():
            assert bool(torch.isfinite(v).all()), n                                  # every element written; no NaN of an unused slot
        assert float(out["means2D"][:, 2].abs().max()) == 0.0
        assert float(out["means2D"][self.culled].abs().max()) == 0.0
        for p, sl in self.sets:
            culled, labels = self.culled[sl], self.labels[sl]
            sat = torch.from_numpy(np.char.find(labels, ":sat") >= 0)
            for n in self.names(p):
                assert float(out[n][culled].abs().max()) == 0.0, n                   # radius 0: exactly 0 in every output
                if bool((~culled).any()) and not (n.endswith("rest") and self.deg == 0):
                    assert float(out[n][~culled].abs().max()) > 0.0, n
            rest = out["features_rest" if p == "ray" else "bg_features_rest"]
            if K < 16:
                assert float(rest[:, K - 1:].abs().max()) == 0.0                     # SH gradients above the active degree
            if bool(sat.any()):                                                      # sigmoid exactly 0 or 1: dL/dlogit is 0
                assert float(out["opacity" if p == "ray" else "bg_opacity"][sat].abs().max()) == 0.0


@functools.lru_cache(maxsize=None)
def _scene(deg, P, n_ray, bg_all_culled_first=False):
    return _Scene(deg, P, n_ray, bg_all_culled_first)


# ------------------------------------------------------------------------------------------ the premise, on the tensor path

def _tensor_forward(sc):
    """scg_forward on scg_model_activate's outputs of the scene's model + the device-side concatenation of its SH tensors, right
    after the model forward of the same camera: the same capacity."""
    t = sc.tensors
    xyz, opa, sca, rot = mp.activate(**t)
    shs = torch.cat((torch.cat((t["features_dc"], t["bg_features_dc"])), torch.cat((t["features_rest"], t["bg_features_rest"]))), 1).contiguous()
    out = R.forward_fused(sc.st, xyz, opa, shs, None, sca, rot, None, True)
    assert out is not None
    torch.cuda.synchronize()
    assert out[4]["cap"] == sc.state["cap"] and out[4]["plan"].total == sc.state["plan"].total
    return (xyz, opa, shs, None, sca, rot, None), out


@pytest.mark.parametrize("deg", [0, 1, 2, 3])
def test_premise_zero_upstream_leaves_the_planted_records_to_the_geometry_backward(deg):
    """Tensor path, the form this file's kernels correspond to (SH colours, scale + rotation, 16 coefficients) at every degree and on
    the members part B uses: scg_backward with zero dL/dcolor, NULL dL/ddepth and dL/dalpha and pre-zeroed planted records gives
    the bits of scg_geometry_backward called directly on the same records, and the record buffer keeps its words."""
    lib = _lib.load()
    dev = torch.device(DEV, torch.cuda.current_device())
    for P, n_ray in ((181, 121), (120, 0)):
        sc = _Scene(deg, P, n_ray)
        ins, (_c, radii, _d, _a, state) = _tensor_forward(sc)
        assert torch.equal(radii, sc.radii)
        in_ptrs = tuple(R.ptr(v) for v in ins)
        shapes = dict(means3D=(P, 3), means2D=(P, 3), opacities=(P, 1), shs=(P, 16, 3), scales=(P, 3), rotations=(P, 4))
        got = []
        for direct in (False, True):
            out = {n: torch.full(s, float("nan"), dtype=F32, device=DEV) for n, s in shapes.items()}
            grads = tuple(R.ptr(out.get(n)) for n in ("means3D", "means2D", "opacities", "shs", "colors_precomp", "scales", "rotations", "cov3D_precomp"))
            rec = sc.ref["rec"].to(DEV)
            fr = state["frame"]
            if direct:
                clamped = state["ws"].data_ptr() + state["plan"].clamped
                R.check(lib.scg_geometry_backward(fr.ref, *in_ptrs, radii.data_ptr(), clamped, rec.data_ptr(), *grads, 0, R._stream(dev)),
                        "scg_geometry_backward")
            else:
                dcol = torch.zeros((3, sc.H, sc.W), dtype=F32, device=DEV)
                R.check(lib.scg_backward(fr.ref, *in_ptrs, radii.data_ptr(), state["cap"], state["ws"].data_ptr(), dcol.data_ptr(), None,
                                         None, rec.data_ptr(), 1, *grads, 0, None, R._stream(dev)), "scg_backward")
            torch.cuda.synchronize()
            assert torch.equal(_bits(rec), _bits(sc.ref["rec"])), (deg, P, "records", direct)
            got.append(out)
        for n in shapes:
            assert bool(torch.isfinite(got[1][n]).all()), n
            assert _same_bits(got[0][n], got[1][n]), (deg, P, n)
        assert float(got[1]["means3D"].abs().max()) > 0


# ------------------------------------------------------------------------------------------------- part A: forward, bit for bit

@pytest.mark.parametrize("deg", [0, 1, 2, 3])
def test_model_forward_equals_the_tensor_forward_on_the_activated_model_bit_for_bit(deg):
    for P, n_ray in CASES:
        sc = _scene(deg, P, n_ray)
        _ins, (color, radii, depth, alpha, state) = _tensor_forward(sc)
        tag = (deg, P, n_ray)
        assert torch.equal(radii, sc.radii), tag
        assert int(state["num_rendered"]) == int(sc.state["num_rendered"]) > 0, tag
        for name, a, b in (("color", color, sc.color), ("depth", depth, sc.depth), ("alpha", alpha, sc.alpha)):
            assert _same_bits(a, b), tag + (name,)
        vis = (sc.radii > 0).cpu()
        for name in ("splats", "rects", "depth_keys", "clamped", "ranges", "point_list", "final_T", "n_contrib"):
            a, b = sc.field(state, name), sc.field(sc.state, name)
            if name == "splats":                                                     # a culled Gaussian's record is not read
                a, b = a.reshape(P, 12)[vis], b.reshape(P, 12)[vis]
            assert a.numel() > 0 and torch.equal(a, b), tag + (name,)
        assert float(sc.alpha.max()) > 0


# ----------------------------------------------------------------------------------------------- part B: backward against fp64

@pytest.mark.parametrize("P", [181, 120])
@pytest.mark.parametrize("deg", [0, 1, 2, 3])
def test_model_backward_alone_holds_every_class_and_output_to_fp64_at_every_split(deg, P):
    for n_ray in MR.SIZES[P]:
        sc = _scene(deg, P, n_ray)
        out = sc.backward(0, None, GA.FILL_A)
        again = sc.backward(0, None, GA.FILL_B)
        for n in out:
            assert _same_bits(out[n], again[n]), (deg, P, n_ray, n)                  # no atomics in this stage: the same bits
        sc.exact_statements(out)
        sc.hold(f"d{deg} P={P} n_ray={n_ray}", out)


@pytest.mark.parametrize("deg", [0, 1, 2, 3])
def test_model_backward_with_the_background_sets_first_workgroup_culled(deg):
    sc = _Scene(deg, 181, 61, bg_all_culled_first=True)
    assert int((sc.radii[61:121] > 0).sum()) == 0 and int((sc.radii[121:] > 0).sum()) > 0 and int((sc.radii[:61] > 0).sum()) > 0
    out = sc.backward(0, None, GA.FILL_A)
    assert all(_same_bits(out[n], v) for n, v in sc.backward(0, None, GA.FILL_B).items())
    sc.exact_statements(out)
    sc.hold(f"d{deg} P=181 n_ray=61 first background workgroup culled", out)


@pytest.mark.parametrize("P", [181, 120])
@pytest.mark.parametrize("deg", [0, 1, 2])
def test_sh_tail_zero_writes_only_what_its_rule_allows_and_the_same_bits(deg, P):
    """SCG_BACKWARD_SH_TAIL_ZERO: the words of a features_rest record at or above 3 (K - 1) keep their bits, except those that share
    a stored float4 with a word that can be non-zero (model_refs.rest_words_the_tail_rule_may_write: the head of a record, or the
    next record's head; and the scalar words behind a partial workgroup's last whole float4), which receive zeros.  Everything
    else equals the flags-0 bits.  First with the tails holding zeros (the caller's promise), then with a sentinel word."""
    K = (deg + 1) ** 2
    sent = torch.tensor([SENTINEL], dtype=torch.int32).view(F32)
    for n_ray in MR.SIZES[P]:
        sc = _scene(deg, P, n_ray)
        base = sc.backward(0, None, GA.FILL_A)
        for sentinel, fill in ((False, GA.FILL_A), (True, GA.FILL_B)):
            prefill = {n: torch.full_like(v, float("nan")) for n, v in base.items()}
            for p, sl in sc.sets:
                r = prefill["features_rest" if p == "ray" else "bg_features_rest"]
                r[:, K - 1:] = sent if sentinel else 0.0
                r[:, :K - 1] = 777.0                                                 # the active coefficients: anything
            got = sc.backward(_lib.BACKWARD_SH_TAIL_ZERO, prefill, fill)
            for n in base:
                if not n.endswith("features_rest"):
                    assert _same_bits(got[n], base[n]), (deg, P, n_ray, n)
            for p, sl in sc.sets:
                n = "features_rest" if p == "ray" else "bg_features_rest"
                rows = sl.stop - sl.start
                g, b = _bits(got[n]).reshape(rows, 45), _bits(base[n]).reshape(rows, 45)
                tail = torch.zeros(rows, 45, dtype=torch.bool)
                tail[:, 3 * (K - 1):] = True
                assert torch.equal(g[~tail], b[~tail]), (deg, P, n_ray, n, "active words")
                if not sentinel:
                    assert torch.equal(g, b) and int(g[tail].abs().max()) == 0, (deg, P, n_ray, n)
                    continue
                may = MR.rest_words_the_tail_rule_may_write(rows, deg) if deg > 0 else torch.zeros(rows, 45, dtype=torch.bool)
                assert bool((g[tail & ~may] == SENTINEL).all()), (deg, P, n_ray, n, "a tail word outside the rule was written")
                assert bool(((g[tail & may] == 0) | (g[tail & may] == SENTINEL)).all()), (deg, P, n_ray, n)
                assert bool((tail & ~may).any())


@pytest.mark.parametrize("P", [181, 120])
@pytest.mark.parametrize("deg", [0, 3])
def test_accumulate_adds_one_fp32_sum_to_every_parameter_gradient_and_overwrites_means2D(deg, P):
    gen = torch.Generator().manual_seed(41 + deg)
    for n_ray in MR.SIZES[P]:
        sc = _scene(deg, P, n_ray)
        base = sc.backward(0, None, GA.FILL_A)
        prior = {n: torch.randn(v.shape, generator=gen) for n, v in base.items()}
        for fill in (GA.FILL_A, GA.FILL_B):
            acc = sc.backward(_lib.BACKWARD_ACCUMULATE, prior, fill)
            for n in base:
                if n == "means2D":
                    assert _same_bits(acc[n], base[n]), (deg, P, n_ray)              # per view: overwritten, not added
                    continue
                assert _same_bits(acc[n], prior[n] + base[n]), (deg, P, n_ray, n)    # fl(prefill + g0), every element
        vis = ~sc.culled
        assert int(sc.culled.sum()) > 0 and int(vis.sum()) > 0

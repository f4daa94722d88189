"""The init stage without a GPU: the fixtures the reference's own code produced (tests/golden/ref_init.npz, ref_init_edges.npz), the
plain torch restatement held to them, the packing of view_gs into the arena, the splitting of a schedule into launches (against a fake
library) and the argument validation of the C entry points."""
import ctypes as C

import numpy as np
import pytest
import torch

import init_refs as ir
from scgaussian_amd import _lib
from scgaussian_amd import init_stage as IS


@pytest.fixture(scope="module")
def fx():
    return ir.fixture()


@pytest.fixture(scope="module")
def fe():
    return ir.fixture_edges()


def _close(a32, a64, floor):
    a64 = np.asarray(a64, dtype=np.float64)
    return float(np.abs(np.asarray(a32, dtype=np.float64) - a64).max()) <= floor * max(1.0, float(np.abs(a64).max()))


def test_fixture_fp32_record_lies_within_the_floor_of_the_fp64_record(fx):
    assert int(fx["iters"]) == 40 and list(fx["halve_at"]) == [10, 20, 30]
    assert [len(fx[f"A_in_{a}{b}_z_val"]) for a, b in fx["A_pairs"]] == [1, 65, 1, 257, 65, 257]
    for k in ("losses", "it0_loss", "it0_loss_state", "final_z", "final_best", "final_min", "after1_z", "after1_best", "after1_min",
              "after2_z", "after2_best", "after2_min", "loaded_z"):
        assert fx[f"A_f32_{k}"].dtype == np.float32 and fx[f"A_f64_{k}"].dtype == np.float64
        assert _close(fx[f"A_f32_{k}"], fx[f"A_f64_{k}"], ir.FLOOR), k
    g64 = fx["A_f64_it0_grad"]
    assert float(np.abs(fx["A_f32_it0_grad"] - g64).max()) <= ir.GRAD_FLOOR * float(np.abs(g64).max())
    # the scene has what it was built for: ~20 % masked out, depths behind the other view, terms far outside it
    vg = ir.load_scene(fx, "A")
    masked = sum(int(((vg[a]["match_infos"][b]["blender_mask"] * vg[b]["match_infos"][a]["blender_mask"]) <= 0).sum())
                 for a, b in ir.arena(vg))
    N = len(g64)
    assert 0.1 * N < masked < 0.3 * N
    assert int((g64 == 0).sum()) == masked                                   # a masked-out match has no gradient
    assert float(fx["A_f64_it0_loss_state"].max()) > 1.0                     # projects (far) outside the other view
    z0 = ir.flat(vg, {a: {b: vg[a]["match_infos"][b]["z_val"] for b in vg[a]["match_infos"]} for a in vg}).numpy()
    assert int((z0 < 0).sum()) >= 10
    # the aliasing quirk of get_z_val(): best after two iterations is z after the first; min is the smaller of L0 and L1
    for p in ("f32", "f64"):
        assert np.array_equal(fx[f"A_{p}_after1_best"], fx[f"A_{p}_after1_z"])
        assert np.array_equal(fx[f"A_{p}_after2_best"], fx[f"A_{p}_after1_z"])
        assert np.array_equal(fx[f"A_{p}_after1_min"], fx[f"A_{p}_it0_loss_state"])
        assert bool((fx[f"A_{p}_after2_min"] <= fx[f"A_{p}_after1_min"]).all())
        assert np.array_equal(fx[f"A_{p}_loaded_z"], fx[f"A_{p}_final_best"])
    # scene B: no valid match — NaN scalar, zero gradient, depths that never move, finite terms
    for p in ("f32", "f64"):
        assert np.isnan(fx[f"B_{p}_it0_loss"]) and np.isnan(fx[f"B_{p}_losses"]).all()
        assert not fx[f"B_{p}_it0_grad"].any() and np.isfinite(fx[f"B_{p}_it0_loss_state"]).all()
        z0 = np.concatenate([fx[f"B_in_{a}{b}_z_val"].reshape(-1) for a, b in fx["B_pairs"]])
        assert np.array_equal(fx[f"B_{p}_final_z"], z0.astype(fx[f"B_{p}_final_z"].dtype))


def test_plain_torch_restatement_reproduces_the_reference_records(fx):
    """tests/init_refs.py (the torch leg of the timing tool and of the GPU tests) against the reference's fp64 run."""
    vg = ir.load_scene(fx, "A", dtype=torch.float64)
    loss, state = ir.matchloss_from_base(vg)
    (5 * loss).backward()
    grad = ir.flat(vg, {a: {b: vg[a]["match_infos"][b]["z_val"].grad for b in vg[a]["match_infos"]} for a in vg}).numpy()
    assert abs(5 * float(loss.detach()) - float(fx["A_f64_it0_loss"])) <= 1e-12
    assert np.abs(ir.flat(vg, state).numpy() - fx["A_f64_it0_loss_state"]).max() <= 1e-12
    assert np.abs(grad - fx["A_f64_it0_grad"]).max() <= 1e-12 * np.abs(grad).max()
    vg = ir.load_scene(fx, "A", dtype=torch.float64)
    out = ir.torch_init_loop(vg, 40, (10, 20, 30))
    z = ir.flat(vg, {a: {b: vg[a]["match_infos"][b]["z_val"] for b in vg[a]["match_infos"]} for a in vg}).numpy()
    assert np.abs(z - fx["A_f64_final_z"]).max() <= 1e-9
    assert np.abs(ir.flat(vg, out["best"]).numpy() - fx["A_f64_final_best"]).max() <= 1e-9
    assert np.abs(ir.flat(vg, out["min_loss"]).numpy() - fx["A_f64_final_min"]).max() <= 1e-9
    assert np.abs(np.array([float(v) for v in out["losses"]]) - fx["A_f64_losses"]).max() <= 1e-10


VALUE_KEYS = ("losses", "it0_loss", "it0_loss_state", "final_z", "final_best", "final_min", "after1_z", "after1_best", "after1_min",
              "after2_z", "after2_best", "after2_min", "loaded_z")


def test_edge_fixture_holds_what_it_was_built_for(fe):
    # scene C: three sizes, three intrinsics, a dictionary order that is not the name order, pairs of 63, 64 and 2
    assert list(fe["C_views"]) == [2, 0, 1] and [tuple(p) for p in fe["C_pairs"]] == [(2, 0), (2, 1), (0, 2), (0, 1), (1, 2), (1, 0)]
    assert list(fe["C_counts"]) == [63, 64, 63, 2, 64, 2] and int(fe["C_iters"]) == 12 and list(fe["C_halve_at"]) == [6]
    assert [tuple(r) for r in fe["C_wh"]] == [(64, 96), (96, 64), (80, 48)]
    assert len({fe["C_intr"][n].tobytes() for n in range(3)}) == 3 and len({fe["C_w2c"][n].tobytes() for n in range(3)}) == 3
    # scene D: seven views, 42 segments of 1, 2, 3 and 5 matches, 64 < N < 128, a segment across element 64
    counts = fe["D_counts"]
    offs = np.concatenate([[0], np.cumsum(counts)[:-1]])
    assert len(fe["D_views"]) == 7 and len(counts) == 42 and set(counts) == {1, 2, 3, 5} and 64 < counts.sum() < 128
    assert list(fe["D_views"]) != sorted(fe["D_views"]) and int(fe["D_iters"]) == 12 and len(fe["D_halve_at"]) == 0
    assert bool(((offs < 64) & (offs + counts > 64)).any())
    for tag in "CD":
        N = int(fe[f"{tag}_counts"].sum())
        for k in VALUE_KEYS:
            assert fe[f"{tag}_f32_{k}"].dtype == np.float32 and fe[f"{tag}_f64_{k}"].dtype == np.float64
            assert _close(fe[f"{tag}_f32_{k}"], fe[f"{tag}_f64_{k}"], ir.FLOOR), (tag, k)
        g64 = fe[f"{tag}_f64_it0_grad"]
        assert g64.shape == (N,) and fe[f"{tag}_f64_losses"].shape == (12,) and fe[f"{tag}_in_rays_o"].shape == (N, 3)
        assert float(np.abs(fe[f"{tag}_f32_it0_grad"] - g64).max()) <= ir.GRAD_FLOOR * float(np.abs(g64).max())
        vg = ir.load_scene(fe, tag)
        assert list(vg) == [f"view{i}" for i in fe[f"{tag}_views"]]
        masked = sum(int(((vg[a]["match_infos"][b]["blender_mask"] * vg[b]["match_infos"][a]["blender_mask"]) <= 0).sum())
                     for a, b in ir.arena(vg))
        assert int((g64 == 0).sum()) == masked and 0 < masked < N
        for p in ("f32", "f64"):
            assert np.array_equal(fe[f"{tag}_{p}_after2_best"], fe[f"{tag}_{p}_after1_z"])
            assert np.array_equal(fe[f"{tag}_{p}_after1_min"], fe[f"{tag}_{p}_it0_loss_state"])
            assert np.array_equal(fe[f"{tag}_{p}_loaded_z"], fe[f"{tag}_{p}_final_best"])


@pytest.mark.parametrize("tag", ["C", "D"])
def test_plain_torch_restatement_reproduces_the_edge_records(fe, tag):
    """Unequal views: the size of the EARLIER view in dictionary order, the camera of the TARGET view.  In fp64 the restatement is
    the record up to the order of its matrix products; in fp32 it is held to the fp64 record as the kernel is: max(4 * e32, floor),
    e32 = the reference's own fp32 record against its fp64 one."""
    iters, halve_at = int(fe[f"{tag}_iters"]), tuple(int(h) for h in fe[f"{tag}_halve_at"])
    rec = lambda p, k: fe[f"{tag}_{p}_{k}"]                                                  # noqa: E731
    grad_of = lambda vg: ir.flat(vg, {a: {b: mi["z_val"].grad for b, mi in v["match_infos"].items()} for a, v in vg.items()})   # noqa: E731
    for dtype in (torch.float64, torch.float32):
        vg = ir.load_scene(fe, tag, dtype=dtype)
        loss, state = ir.matchloss_from_base(vg)
        (5 * loss).backward()
        it0 = {"it0_loss": np.array(5 * float(loss.detach())), "it0_loss_state": ir.flat(vg, state), "it0_grad": grad_of(vg)}
        vg = ir.load_scene(fe, tag, dtype=dtype)
        out = ir.torch_init_loop(vg, iters, halve_at)
        run = {"final_z": ir.flat(vg, ir.z_of(vg)), "final_best": ir.flat(vg, out["best"]), "final_min": ir.flat(vg, out["min_loss"]),
               "losses": np.array([float(v) for v in out["losses"]])}
        if dtype == torch.float64:
            assert abs(float(it0["it0_loss"]) - float(rec("f64", "it0_loss"))) <= 1e-12
            assert np.abs(it0["it0_loss_state"].numpy() - rec("f64", "it0_loss_state")).max() <= 1e-12
            assert np.abs(it0["it0_grad"].numpy() - rec("f64", "it0_grad")).max() <= 1e-12 * np.abs(rec("f64", "it0_grad")).max()
            for k in ("final_z", "final_best", "final_min"):
                assert np.abs(run[k].numpy() - rec("f64", k)).max() <= 1e-9, k
            assert np.abs(run["losses"] - rec("f64", "losses")).max() <= 1e-10
        else:
            for k, v in {**it0, **run}.items():
                ir.held(f"cpu fp32 restatement {tag} {k}", v, rec("f64", k), rec("f32", k), grad=(k == "it0_grad"))


def test_arena_packing_of_unequal_views(fe):
    """Scene C: width and height come from the earlier view in DICTIONARY order (view2 before view0 before view1), K and w2c from
    the target view."""
    vg = ir.load_scene(fe, "C")
    st = IS.InitStage.from_view_gs(vg)
    assert [(a, b) for a, b, _o, _m in st.segments] == ir.arena(vg) and st.N == 258
    table = np.frombuffer(st.table.numpy().tobytes(), dtype=IS._SEG_DTYPE)
    first = {("view2", "view0"): "view2", ("view0", "view2"): "view2", ("view2", "view1"): "view2", ("view1", "view2"): "view2",
             ("view0", "view1"): "view0", ("view1", "view0"): "view0"}
    sizes = {"view2": (64, 96), "view0": (96, 64), "view1": (80, 48)}
    for rec, (a, b, off, M) in zip(table, st.segments):
        assert (int(rec["offset"]), int(rec["count"])) == (off, M)
        assert (float(rec["width"]), float(rec["height"])) == sizes[first[a, b]], (a, b)
        assert np.array_equal(rec["intr"], vg[b]["intr"].numpy().reshape(9)) and not np.array_equal(rec["intr"], vg[a]["intr"].numpy().reshape(9))
        assert np.array_equal(rec["w2c"], vg[b]["w2c"].numpy()[:3].reshape(12))


def test_partials_bytes_at_the_launch_limits():
    lib = _lib.load()
    for N in (1, 64, 65):
        for n in (0, 1, 64, 65, 4096):
            assert lib.scg_init_stage_partials_bytes(N, n) == max(n, 1) * ((N + 63) // 64) * 4, (N, n)
        assert lib.scg_init_stage_partials_bytes(N, 4097) == 0 and lib.scg_init_stage_partials_bytes(N, -1) == 0
    for n in (0, 1, 4096, 4097, -1):
        assert lib.scg_init_stage_partials_bytes(0, n) == 0
    assert _lib.INIT_STAGE_MAX_STEPS == IS.MAX_STEPS == 4096


def test_arena_packing(fx):
    vg = ir.load_scene(fx, "A")
    vg["view0"]["width"], vg["view0"]["height"] = 96, 64                     # sizes differ per view: the earlier key's is used
    vg["view1"]["width"], vg["view1"]["height"] = 100, 70
    vg["view2"]["width"], vg["view2"]["height"] = 110, 80
    st = IS.InitStage.from_view_gs(vg)
    assert [(a, b) for a, b, _o, _m in st.segments] == ir.arena(vg)
    assert [m for *_x, m in st.segments] == [1, 65, 1, 257, 65, 257]
    assert [o for _a, _b, o, _m in st.segments] == [0, 1, 66, 67, 324, 389] and st.N == 646
    assert st.lr == 0.5 and st.loss_scale == 5.0 and st.iteration == 0 and st.empty_pairs == []
    table = np.frombuffer(st.table.numpy().tobytes(), dtype=IS._SEG_DTYPE)
    assert table.itemsize == C.sizeof(_lib.ScgInitSegment) == 100
    first = {("view0", "view1"): "view0", ("view1", "view0"): "view0", ("view0", "view2"): "view0", ("view2", "view0"): "view0",
             ("view1", "view2"): "view1", ("view2", "view1"): "view1"}
    views = st.z_views()
    for rec, (a, b, off, M) in zip(table, st.segments):
        assert (int(rec["offset"]), int(rec["count"])) == (off, M)
        assert (float(rec["width"]), float(rec["height"])) == (vg[first[a, b]]["width"], vg[first[a, b]]["height"])
        assert np.array_equal(rec["intr"], vg[b]["intr"].numpy().reshape(9))                 # the TARGET view's camera
        assert np.array_equal(rec["w2c"], vg[b]["w2c"].numpy()[:3].reshape(12))
        mi, back = vg[a]["match_infos"][b], vg[b]["match_infos"][a]
        assert torch.equal(st.uv_t[off:off + M], back["uv"])                                 # the PARTNER's pixels
        assert torch.equal(st.rays_o[off:off + M], mi["rays_o"]) and torch.equal(st.rays_d[off:off + M], mi["rays_d"])
        valid = (mi["blender_mask"] * back["blender_mask"]) > 0
        assert torch.equal(st.wgt[off:off + M], valid.float() / valid.sum())
        assert torch.equal(views[a][b], mi["z_val"].detach()) and views[a][b].shape == (M, 1)
        assert views[a][b].data_ptr() == st.z.data_ptr() + 4 * off                           # a view, not a copy
    st.install(vg)
    p = vg["view2"]["match_infos"]["view1"]["z_val"]
    assert isinstance(p, torch.nn.Parameter) and p.requires_grad and p.shape == (257, 1)
    with torch.no_grad():
        p[3, 0] = 123.0
    assert float(st.z[389 + 3]) == 123.0
    assert IS._is_arena(st, [vg[a]["match_infos"][b]["z_val"] for a, b in ir.arena(vg)])
    # nested results have the reference's shapes; load_best copies best into z
    st.best_z.fill_(7.0)
    assert st.best_state_dict()["view0"]["view2"].shape == (65, 1) and st.min_loss_state()["view0"]["view2"].shape == (65,)
    st.load_best(vg)
    assert float(vg["view0"]["match_infos"]["view1"]["z_val"][0, 0]) == 7.0
    # a pair without a valid match: weight zero everywhere, remembered for the NaN of the scalar
    sb = IS.InitStage.from_view_gs(ir.load_scene(fx, "B"))
    assert sb.empty_pairs == [("view0", "view1"), ("view1", "view0")] and not sb.wgt.any()


class _FakeLib:
    def __init__(self):
        self.calls = []

    def scg_init_stage_run(self, *args):
        self.calls.append(args)
        return 0


def _fake(monkeypatch):
    lib = _FakeLib()
    monkeypatch.setattr(IS._lib, "load", lambda: lib)
    monkeypatch.setattr(IS, "_current_stream", lambda t: None)
    return lib


def test_schedule_splitting_against_a_fake_library(fx, monkeypatch):
    lib = _fake(monkeypatch)
    st = IS.InitStage.from_view_gs(ir.load_scene(fx, "A"))
    st.run_schedule(2000, halve_at=(500, 1000, 1500))
    first, steps, lrs = ([c[i] for c in lib.calls] for i in (12, 13, 14))
    assert first == [0, 500, 1000, 1500] and steps == [500] * 4 and lrs == [0.5, 0.25, 0.125, 0.0625]
    assert st.iteration == 2000 and st.lr == 0.0625
    c = lib.calls[0]
    assert c[1] == 6 and c[2] == 646 and c[15:18] == (0.9, 0.999, 1e-15) and c[18] == 5.0
    assert c[22] == 500 * 11 * 4 and c[21] is not None and c[19] is None and c[20] is None      # partials: (500, ceil(646 / 64))
    assert st.partials().shape == (2000, 11) and st.losses().shape == (2000,)
    # a boundary at the first iteration halves before it; boundaries outside the run are ignored; indices are global
    lib.calls.clear()
    st = IS.InitStage.from_view_gs(ir.load_scene(fx, "A"), lr=0.8, record_losses=False)
    st.run_schedule(7, halve_at=(0, 3, 7, 100))
    assert [(c[12], c[13], c[14]) for c in lib.calls] == [(0, 3, 0.4), (3, 4, 0.2)] and lib.calls[0][21] is None
    st.run_schedule(5, halve_at=(0, 3, 7, 9))                                # continues at iteration 7: halves at 7 and at 9
    assert [(c[12], c[13], c[14]) for c in lib.calls[2:]] == [(7, 2, 0.1), (9, 3, 0.05)]
    st.run(0)
    assert len(lib.calls) == 4
    # more iterations than one launch takes
    lib.calls.clear()
    st.run(2 * IS.MAX_STEPS + 5)
    assert [(c[12], c[13]) for c in lib.calls] == [(12, 4096), (12 + 4096, 4096), (12 + 8192, 5)]
    with pytest.raises(_lib.ScgError, match="not recorded"):
        st.losses()


def test_launching_on_cpu_tensors_is_refused(fx):
    st = IS.InitStage.from_view_gs(ir.load_scene(fx, "A"))
    with pytest.raises(_lib.ScgError, match="no CPU path"):
        st.run(1)
    with pytest.raises(_lib.ScgError, match="no CPU path"):
        IS.match_loss_from_base(ir.load_scene(fx, "A"))


def test_argument_validation_returns_codes_without_a_gpu():
    lib = _lib.load()
    assert lib.scg_struct_bytes(6) == C.sizeof(_lib.ScgInitSegment)
    assert lib.scg_init_stage_partials_bytes(646, 40) == 40 * 11 * 4
    assert lib.scg_init_stage_partials_bytes(646, 0) == 11 * 4 and lib.scg_init_stage_partials_bytes(64, 1) == 4
    assert lib.scg_init_stage_partials_bytes(65, 1) == 8
    assert lib.scg_init_stage_partials_bytes(0, 1) == 0 and lib.scg_init_stage_partials_bytes(10, -1) == 0
    assert lib.scg_init_stage_partials_bytes(10, _lib.INIT_STAGE_MAX_STEPS + 1) == 0
    f = 0x1000                     # never dereferenced: validation fails first

    def call(seg=f, nseg=2, N=100, inputs=(f, f, f, f), z=f, state=(f, f, f, f), first=0, n=4, lr=0.5, betas=(0.9, 0.999),
             outs=(None, None), partials=None, pbytes=0):
        return lib.scg_init_stage_run(seg, nseg, N, *inputs, z, *state, first, n, lr, betas[0], betas[1], 1e-15, 5.0, *outs,
                                      partials, pbytes, None)
    assert call(N=-1) == -2 and call(nseg=-1) == -2 and call(nseg=0) == -2
    assert call(N=0, seg=None, nseg=0, inputs=(None,) * 4, z=None) == 0                       # nothing to do
    assert call(n=-1) == -2 and call(n=_lib.INIT_STAGE_MAX_STEPS + 1) == -2 and b"n_steps" in lib.scg_last_error()
    assert call(first=-1) == -2 and call(first=2**31 - 1) == -2
    assert call(seg=None) == -1 and call(z=None) == -1
    for k in range(4):
        assert call(inputs=tuple(None if j == k else f for j in range(4))) == -1
        assert call(state=tuple(None if j == k else f for j in range(4))) == -1
    assert call(betas=(1.0, 0.999)) == -2 and call(betas=(0.9, -0.1)) == -2
    assert call(inputs=(f, f, f + 4, f)) == -5 and b"uv_t" in lib.scg_last_error()           # float2 loads
    assert call(z=f + 2) == -5 and call(outs=(f + 1, None), n=0) == -5
    assert call(partials=f, pbytes=4 * 2 * 4 - 1) == -4 and b"partials" in lib.scg_last_error()

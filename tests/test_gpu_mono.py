"""The scene setup on the GPU (csrc/mono.hip, scgaussian_amd/mono.py) against its numpy restatement (tests/mono_refs.py), bit for
bit, at the edges of its launches and of its rule; against the reference's own create_from_mono (tests/golden/ref_mono.npz) at the
bars of tests/test_mono_cpu.py; and through its consumers.

"Bit for bit" on floats: equal bit patterns, or NaN on both sides (the sign and payload of a NaN an operation PRODUCES are the
processor's choice and differ between the host that restates and the GPU)."""
import os

import numpy as np
import pytest
import torch

import mono_refs as MR
from scgaussian_amd import _arena, _lib, mono, optim as O, render as rmod, seed, synthetic as syn
from scgaussian_amd.init_stage import InitStage

pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_mono.npz")
OUT = tuple(n for n, _t in mono.MonoPlan.OUTPUTS) + ("counts",)
F = np.float32


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind != "f":
        return bool(np.array_equal(a, b))
    return bool(np.all((a.view(np.int32) == b.view(np.int32)) | (np.isnan(a) & np.isnan(b))))


def check(setup, want=None):
    want = MR.restate(setup.plan) if want is None else want
    for k in OUT:
        got = getattr(setup, k).cpu().numpy()
        assert same_bits(got, want[k].reshape(got.shape)), (k, np.argwhere(~np.isclose(got, want[k].reshape(got.shape), rtol=0, atol=0,
                                                                                          equal_nan=True))[:4])
    return want


# ---- the scene of the launch and rule edges -----------------------------------------------------------------------------------
SIZES = [(40, 56), (48, 64), (36, 60), (50, 70), (33, 47)]          # (H, W): five views of unequal size
COUNTS = {(0, 1): 1, (0, 2): 63, (0, 3): 64, (0, 4): 65, (1, 2): 255, (1, 3): 256, (1, 4): 257, (2, 3): 513, (2, 4): 512, (3, 4): 2}
K_EDGE = 31                                                         # view 1: mask 0 up to column 31, 1 from column 32


def edge_scene():
    """Five views.  View 0 has no mask; view 1 a step mask (0 west of column 32, 1 east); views 2 and 4 a mask of 1e-25 (the fp32
    product of two such samples underflows to 0); view 3 a mask of ones.  Segments of 1 ... 513 matches, two of them (256, 512) ending
    exactly on a workgroup boundary with another segment behind them.  Pair (1, 2) carries the planted pixels, pair (1, 3) exactly one
    valid match, pair (0, 3) only valid ones, pair (2, 4) none."""
    rng = np.random.default_rng(11)
    masks = [None, np.zeros(SIZES[1]), np.full(SIZES[2], 1e-25), np.ones(SIZES[3]), np.full(SIZES[4], 1e-25)]
    masks[1][:, K_EDGE + 1:] = 1.0
    cams = MR.cameras(SIZES, rng, masks=masks)
    md = MR.match_data(cams, COUNTS, rng)
    n = [c.image_name for c in cams]
    W1, H1 = SIZES[1][1], SIZES[1][0]
    x_edge = F((K_EDGE + 0.5) / W1)                                 # ix = 31 exactly: the east tap's weight is exactly 0
    planted = [(0, 0), (1, 1), (0, 1), (1, 0),                                                         # m = 0 and 1
               (-0.2, 0.5), (1.3, 0.5), (0.5, -0.4), (0.5, 1.7), (-3, -3),                             # every tap outside: invalid
               (x_edge, 0.5), (np.nextafter(x_edge, F(2)), 0.5), (np.nextafter(x_edge, F(-2)), 0.5),   # the zero-ness edge
               (0.5 / W1, 0.5 / H1), ((W1 - 0.5) / W1, 0.5 / H1), (0.5 / W1, (H1 - 0.5) / H1), ((W1 - 0.5) / W1, (H1 - 0.5) / H1),
               (np.nan, 0.5), (0.5, np.nan), (np.inf, 0.5), (0.5, -np.inf), (2.0 ** 33, 0.5), (0.5, -2.0 ** 33), (np.nan, np.inf)]
    md[n[1]][n[2]][:len(planted)] = np.array(planted, dtype=np.float64)
    md[n[2]][n[1]][:len(planted)] = rng.uniform(0.1, 0.9, size=(len(planted), 2))
    west = rng.uniform(0.05, 0.3, size=(256, 2))                    # pair (1, 3): all in the mask's zeros but one
    west[7] = (0.8, 0.5)
    md[n[1]][n[3]] = west
    md[n[3]][n[1]] = rng.uniform(0.1, 0.9, size=(256, 2))
    md[n[0]][n[3]] = rng.uniform(0.1, 0.9, size=(64, 2))             # pair (0, 3): every match valid
    md[n[3]][n[0]] = rng.uniform(0.1, 0.9, size=(64, 2))
    md[n[0]][n[1]] = np.array([[0.4, 0.6]])                          # the pair of one match: valid
    md[n[1]][n[0]] = np.array([[0.8, 0.5]])
    return cams, md, rng.random(2 * sum(COUNTS.values()), dtype=np.float32)


@pytest.fixture(scope="module")
def edges():
    cams, md, u = edge_scene()
    setup = mono.MonoSetup.build(cams, md, DEV, u)
    return cams, md, u, setup, MR.restate(setup.plan)


def test_every_output_bit_for_bit_at_the_launch_and_rule_edges(edges):
    cams, md, u, setup, want = edges
    plan = setup.plan
    block = _lib.load().scg_mono_block()
    sizes = [s[3] for s in plan.segments]
    assert {1, block - 1, block, block + 1, 63, 64, 65, 2 * block, 2 * block + 1} <= set(sizes) and len(sizes) == 20
    assert sizes[sizes.index(block) + 1] == block + 1               # the segment behind the one that ends on a workgroup boundary
    check(setup, want)
    # the planted pixels did what they were planted for
    seg = {(a, b): (off, M) for a, b, off, M in plan.segments}
    n = plan.keys
    off, _M = seg[(n[1], n[2])]
    bm, valid = want["blender_mask"][off:off + 23], want["valid"][off:off + 23]
    assert (bm[4:9] == 0).all() and (valid[4:9] == 0).all()         # outside
    assert bm[9] == 0 and valid[9] == 0                             # ix = 31 exactly: the tap of weight 1 is masked, the other weighs 0
    assert 0 < bm[10] < 1e-5 and valid[10] == 1                     # one ulp east: valid
    assert bm[11] == 0 and valid[11] == 0                           # one ulp west
    assert (bm[16:23] == 0).all() and (want["color"][off + 16:off + 23] == 0).all()       # NaN, inf, 2^33: samples nothing
    assert np.isnan(want["uv"][off + 16, 0]) and np.isnan(want["rays_d"][off + 16]).all() # ... and NaN otherwise propagates
    assert np.isinf(want["uv"][off + 18, 0]) and want["uv"][off + 20, 0] == F(2.0 ** 33) * F(64)
    corner = want["color"][off + 12]                                 # a pixel centre samples that pixel alone (0.5 / 48 is not exact)
    assert np.allclose(corner, np.asarray(cams[1].image)[0, 0].astype(F) / F(255), rtol=1e-6, atol=0)
    # the pairs
    counts = dict(zip([(a, b) for a, b, _o, _M in plan.segments], want["counts"]))
    assert counts[(n[1], n[3])] == counts[(n[3], n[1])] == 1 and counts[(n[0], n[3])] == 64 and counts[(n[0], n[1])] == 1
    assert counts[(n[2], n[4])] == counts[(n[4], n[2])] == 0
    o24, M24 = seg[(n[2], n[4])]
    assert (want["blender_mask"][o24:o24 + M24] > 0).any() and (want["wgt"][o24:o24 + M24] == 0).all()        # underflow, not zeros
    assert sorted(setup.empty_pairs()) == sorted([(n[2], n[4]), (n[4], n[2])])
    o13, _ = seg[(n[1], n[3])]
    assert want["wgt"][o13 + 7] == 1 and want["wgt"][o13:o13 + 256].sum() == 1
    o02, M02 = seg[(n[0], n[2])]                                     # no mask: the sum of the in-bounds weights, not 1
    edge = want["blender_mask"][o02:o02 + M02]
    assert ((edge > 0) & (edge < 0.999)).any() or (edge == 0).any()


def test_image_kernel_all_byte_values_and_unequal_views(edges):
    cams, _md, _u, setup, _want = edges
    assert len({c["H"] * c["W"] for c in setup.plan.consts}) == 5
    for cam, k in zip(cams, setup.keys):
        got = setup.view_gs[k]["image_color"].cpu().numpy()
        assert same_bits(got, np.asarray(cam.image).astype(F) / F(255))
    ramp = np.arange(256 * 3, dtype=np.int64).reshape(16, 16, 3) % 256
    ramp = ramp.astype(np.uint8)
    cams2 = [MR.camera("a", ramp, np.eye(3), (0, 0, 0), 1.0, 1.0, (1, 2)), MR.camera("b", ramp[::-1].copy(), np.eye(3), (0, 0, 0), 1.0, 1.0, (1, 2))]
    s = mono.MonoSetup.build(cams2, {"a": {"b": np.array([[0.5, 0.5]])}, "b": {"a": np.array([[0.5, 0.5]])}}, DEV, np.zeros(2, dtype=F))
    want = (np.arange(256, dtype=np.float64) / 255.0).astype(F)
    assert same_bits(s.view_gs["a"]["image_color"].cpu().numpy().reshape(-1), want[ramp.reshape(-1)])
    check(s)


def test_forty_two_short_segments():
    rng = np.random.default_rng(5)
    cams = MR.cameras([(24 + i, 32 + 2 * i) for i in range(7)], rng)
    counts = {(i, j): 1 + (i + 2 * j) % 5 for i in range(7) for j in range(i + 1, 7)}
    md = MR.match_data(cams, counts, rng)
    setup = mono.MonoSetup.build(cams, md, DEV, rng.random(2 * sum(counts.values()), dtype=np.float32))
    assert setup.plan.nseg == setup.plan.ngroups == 42
    want = check(setup)
    assert (want["counts"] > 0).all() and setup.empty_pairs() == []


def test_the_depths_are_the_cpu_generators(edges):
    cams, md, _u, _setup, _want = edges
    torch.manual_seed(321)
    a = mono.MonoSetup.build(cams, md, DEV)
    torch.manual_seed(321)
    u = np.concatenate([torch.rand(M, 1).numpy().reshape(M) for _a, _b, _o, M in a.segments])
    assert same_bits(a.u.cpu().numpy(), u)
    check(a)


# ---- the reference's fixture --------------------------------------------------------------------------------------------------
def test_against_the_reference_fixture():
    cams, md, u, ref = MR.fixture_scene(np.load(GOLDEN))
    setup = mono.MonoSetup.build(cams, md, DEV, u)
    check(setup)
    got = {k: getattr(setup, k).cpu().numpy() for k in OUT}
    wide = MR.restate(setup.plan, wide=True)
    for k in ("uv", "z", "valid"):
        assert same_bits(got[k], ref[k].reshape(got[k].shape)), k
    for i, k in enumerate(setup.keys):
        v = setup.view_gs[k]
        for name in ("image_color", "intr", "w2c", "near_far"):
            assert same_bits(v[name].cpu().numpy(), ref[name][i]), (k, name)
    for k in ("color", "blender_mask", "rays_o", "rays_d", "cam_rays_d"):
        tol, e_ref = MR.bar(ref[k], wide[k])
        e = float(np.max(np.abs(got[k].astype(np.float64) - wide[k])))
        print(f"{k}: kernel {e:.3e}, reference {e_ref:.3e}, bar {tol:.3e}")
        assert e <= tol, (k, e, tol)


# ---- consumers ----------------------------------------------------------------------------------------------------------------
def equal_views(n_views=3, M=200, size=(48, 64), seed_=2):
    """Views of one size looking at one cloud of points: the matches are the points' projections, so the init stage has something
    to converge to."""
    rng = np.random.default_rng(seed_)
    cams = MR.cameras([size] * n_views, rng, fovs=[55.0] * n_views)
    H, W = size
    pts = np.stack([rng.uniform(-1.2, 1.2, M), rng.uniform(-0.9, 0.9, M), rng.uniform(3.5, 6.0, M)], 1)
    proj = []
    for cam in cams:
        c = mono.view_constants(cam)
        pc = pts @ c["w2c32"][:3, :3].astype(np.float64).T + c["w2c32"][:3, 3].astype(np.float64)
        px = pc @ c["intr32"].astype(np.float64).T
        proj.append(np.stack([px[:, 0] / px[:, 2] / W, px[:, 1] / px[:, 2] / H], 1))
    md = {a.image_name: {b.image_name: proj[i].copy() for j, b in enumerate(cams) if j != i} for i, a in enumerate(cams)}
    return cams, md, rng.random(n_views * (n_views - 1) * M, dtype=np.float32)


def tensor_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and same_bits(a.detach().cpu().numpy(), b.detach().cpu().numpy())


def inside(t, arena):
    return arena.data_ptr() <= t.data_ptr() and t.data_ptr() + t.numel() * t.element_size() <= arena.data_ptr() + arena.numel()


def test_consumers_read_the_arena_in_place(edges):
    _cams, _md, _u, setup, _want = edges
    stage = InitStage.from_mono(setup)
    packed = InitStage.from_view_gs(setup.view_gs)
    assert stage.segments == packed.segments and sorted(stage.empty_pairs) == sorted(packed.empty_pairs) and len(stage.empty_pairs) == 2
    for k in ("rays_o", "rays_d", "uv_t", "wgt", "z", "table"):
        assert tensor_bits(getattr(stage, k), getattr(packed, k)), k
        assert inside(getattr(stage, k), setup.arena) and not inside(getattr(packed, k), setup.arena), k
    assert _arena.is_arena(stage.z, [setup.view_gs[a]["match_infos"][b]["z_val"] for a, b, _o, _M in stage.segments], stage.segments)
    with pytest.raises(_lib.ScgError, match="unequal sizes"):          # the seed path alone needs views of one size
        seed.SeedInputs.from_mono(setup, stage)
    with pytest.raises(_lib.ScgError, match="unequal sizes"):
        seed.SeedInputs.from_view_gs(setup.view_gs, packed)

    cams, md, u = equal_views()
    setup = mono.MonoSetup.build(cams, md, DEV, u)
    stage, packed = InitStage.from_mono(setup), InitStage.from_view_gs(setup.view_gs)
    inputs, repacked = seed.SeedInputs.from_mono(setup, stage), seed.SeedInputs.from_view_gs(setup.view_gs, packed)
    for k in ("rays_o", "rays_d", "uv_t", "wgt", "z", "table"):
        assert tensor_bits(getattr(stage, k), getattr(packed, k)), k
    assert inputs.segments == repacked.segments and (inputs.H, inputs.W, inputs.V) == (repacked.H, repacked.W, repacked.V)
    assert np.array_equal(inputs.table_host, repacked.table_host) and tensor_bits(inputs.table_dev, repacked.table_dev)
    for k in ("color", "uv", "cam_z"):
        assert tensor_bits(getattr(inputs, k), getattr(repacked, k)), k
        assert inside(getattr(inputs, k), setup.arena) and not inside(getattr(repacked, k), setup.arena), k
    for k in ("rays_o", "rays_d", "z", "min_loss"):
        assert getattr(inputs, k).data_ptr() == getattr(stage, k).data_ptr(), k
    assert inputs.table_dev.data_ptr() == setup.seed_table.data_ptr() and all(a is b for a, b in zip(inputs.views, setup.view_gs.values()))
    other = mono.MonoSetup.build(cams, md, DEV, u)
    with pytest.raises(_lib.ScgError, match="another setup"):
        seed.SeedInputs.from_mono(other, stage)


# ---- determinism and graph replay -----------------------------------------------------------------------------------------------
def test_two_builds_give_equal_bytes_and_a_graph_replays_the_launches():
    cams, md, u = edge_scene()
    a, b = mono.MonoSetup.build(cams, md, DEV, u), mono.MonoSetup.build(cams, md, DEV, u)
    for k in a.plan.regions:
        assert torch.equal(getattr(a, k).view(-1).view(torch.uint8), getattr(b, k).view(-1).view(torch.uint8)), k
    # other match pixels, written in place behind a capture of the three launches
    rng = np.random.default_rng(99)
    md2 = {x: {y: rng.uniform(-0.02, 1.02, size=np.asarray(m).shape) for y, m in d.items()} for x, d in md.items()}
    want = mono.MonoSetup.build(cams, md2, DEV, u)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        a.launch()
    a.match_pixel.copy_(want.match_pixel)
    for k in OUT:
        getattr(a, k).zero_()
    graph.replay()
    torch.cuda.synchronize()
    for k in OUT:
        assert torch.equal(getattr(a, k).view(-1).view(torch.uint8), getattr(want, k).view(-1).view(torch.uint8)), k
    check(a, MR.restate(want.plan))


# ---- end to end -----------------------------------------------------------------------------------------------------------------
class Model:
    """The attribute names of the reference's GaussianModel that the render and optimizer paths read."""
    max_sh_degree = 3
    active_sh_degree = 0


def test_end_to_end_from_cameras_to_an_optimizer_step(monkeypatch, capsys):
    cams, md, u = equal_views(M=300)
    H, W = np.asarray(cams[0].image).shape[:2]
    gm = Model()
    mono.install(gm, DEV)
    # every way a tensor reaches the host is counted over the setup and the packing
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
    gm.create_from_mono(cams, md, 2.5, u=u)
    stage = InitStage.from_mono(gm.mono_setup)
    inputs = seed.SeedInputs.from_mono(gm.mono_setup, stage)
    monkeypatch.undo()
    assert len(reads) <= 1, reads
    assert gm.spatial_lr_scale == 2.5 and gm.match_data is md and gm.view_gs is gm.mono_setup.view_gs and stage.empty_pairs == []

    seed.install(gm, stage)
    stage.run_schedule(40, halve_at=(10, 20, 30))
    stage.load_best(gm.view_gs)
    assert bool(torch.isfinite(stage.z).all()) and bool(torch.isfinite(stage.min_loss).all())
    print("init-stage loss, first and last of 40 iterations:", float(stage.losses()[0]), float(stage.losses()[-1]))
    stage.min_loss[::2] = 0.01                                       # some matches are kept and some dropped, whatever forty
    stage.min_loss[1::4] = 0.5                                       # iterations reached
    gm.create_from_pcd(stage.min_loss_state(), inputs=inputs)
    n = gm._zval.shape[0]
    assert f"Number of points at initialisation :  {n}" in capsys.readouterr().out and 0 < n < stage.N
    assert gm.img_colors.shape == (3, 3, H, W) and gm.sparse_depths.shape == (3, H, W)
    opt = O.ArenaAdam([{"params": [getattr(gm, a)], "lr": 1e-3, "name": a.lstrip("_")}
                       for a in ("_zval", "_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation")], lr=0.0, eps=1e-15)
    cam = syn.orbit_camera(W, H, 2.0, 1.0, 7.0).to(DEV)
    pipe = rmod.PipelineParams()
    out = rmod.render(cam, gm, pipe, torch.zeros(3, device=DEV))
    (out["render"].sum() + out["rendered_depth"].sum()).backward()
    opt.step()
    torch.cuda.synchronize()
    for k in ("render", "rendered_depth", "rendered_alpha"):
        assert bool(torch.isfinite(out[k]).all()), k
    for a in ("_zval", "_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation"):
        assert bool(torch.isfinite(getattr(gm, a)).all()), a

"""The init stage's snapshot on the GPU (scgaussian_amd/matchpoint.py, csrc/matchpoint.hip) against the numpy restatement of
tests/matchpoint_refs.py (held to the reference's recorded arrays by tests/test_matchpoint_cpu.py), against the recorded arrays
themselves, against the seeding step's sparse depths, and through its files.

Every comparison is bit for bit: the feature is a re-layout plus a fixed chain of separately rounded fp32 operations, and min / max
are exact in any order.  "Bit for bit" on floats: equal bit patterns, or NaN on both sides (the sign and payload of a NaN an
operation PRODUCES are the processor's choice and differ between the host that restates and the GPU).

Sizes come from the header's defines: T records per tile of the body, G matches per workgroup, B pixels per workgroup of each of
the two pixel kernels."""
import os

import numpy as np
import pytest
import torch
from PIL import Image

import matchpoint_refs as MR
import mono_refs as MonoR
import ply_refs as P
from scgaussian_amd import _lib, _lib_mp, matchpoint, mono, ply_io, seed
from scgaussian_amd.init_stage import InitStage

pytestmark = pytest.mark.gpu
DEV = "cuda"
f32, u32 = np.float32, np.uint32
T, G = _lib_mp.MP_TILE_RECORDS, _lib_mp.MP_MATCH_GROUP
BR, BQ = _lib_mp.MP_RESOLVE_PIXELS, _lib_mp.MP_QUANT_PIXELS


def tensors(arena):
    return {k: torch.from_numpy(np.ascontiguousarray(arena[k], dtype=f32)).to(DEV) for k in MR.IN_KEYS}


def inputs_of(arena, t=None):
    t = tensors(arena) if t is None else t
    return matchpoint.MatchpointInputs.from_flat(t["rays_o"], t["rays_d"], t["z"], t["color"], t["uv"], t["cam_z"], arena["counts"],
                                                 arena["seg_view"], arena["sizes"])


def assert_snapshot(snap, want, what=""):
    """The four regions against a restatement, and zeros everywhere else in the buffer."""
    body, planes, byte_planes, ranges = snap.host_views()
    n = want["body"].shape[0]
    assert body.shape == (n, 27)
    assert MR.same_bits(np.ascontiguousarray(body[:, :12]).view(f32), want["xyz"]), ("xyz", what)
    assert np.array_equal(body[:, 12:], want["body"][:, 12:]), ("normals and colour bytes", what)
    assert len(planes) == len(want["planes"])
    for v, (p, q) in enumerate(zip(planes, byte_planes)):
        assert MR.same_bits(p, want["planes"][v]), ("depth plane", v, what)
        assert np.array_equal(q, want["bytes"][v]), ("byte plane", v, what, np.argwhere(q != want["bytes"][v])[:4])
    assert MR.same_bits(ranges, want["ranges"]), ("ranges", what, ranges, want["ranges"])
    h, l = snap.to_host().numpy(), snap.layout
    assert h.size == l.total
    assert not h[27 * n:l.depth_offset].any() and not h[l.depth_offset + l.depth_bytes:l.byte_offset].any(), ("gaps", what)
    assert not h[l.byte_offset + l.byte_bytes:l.range_offset].any() and not h[l.range_offset + l.range_bytes:].any(), ("gaps", what)
    for (H, W), rec in zip(snap.sizes, snap.views_host):
        first = l.byte_offset + int(rec["first_byte"])
        assert not h[first + H * W:first + (H * W + 3) // 4 * 4].any(), ("plane padding", what)


def check(arena, what=""):
    with np.errstate(all="ignore"):
        want = MR.restate(arena)
    snap = matchpoint.pack(inputs_of(arena))
    assert snap.buffer.device.type == "cuda"
    assert_snapshot(snap, want, what)
    return snap, want


# ---- 1. the record tile -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 2, 3, 4, 5, T - 1, T, T + 1, 2 * T + 1, G - 1, G, G + 1, 2 * G + 3])
def test_every_byte_phase_of_the_bodys_tail(N):
    snap, _ = check(MR.random_arena([N], [0], [(5, 6)], seed=N), N)
    assert snap.layout.body_bytes == (27 * N + 3) // 4 * 4


# ---- 2. segments ------------------------------------------------------------------------------------------------------------------
SEGMENTS = {
    "1_to_513": ([1, 63, 64, 65, 255, 256, 257, 513], [0, 1, 2, 0, 1, 2, 0, 1], 3),
    "42_short": ([(1, 2, 3, 5)[s % 4] for s in range(42)], [s // 6 for s in range(42)], 7),
    "ends_on_a_workgroup": ([G, 3, G - 3, 2 * G, 1], [0, 1, 2, 1, 0], 3),
    "empty_between_full": ([G, 0, G, 5, 0, 0, 7, 0], [0, 1, 2, 0, 1, 2, 1, 0], 3),
    "view_without_a_pair": ([40, 70, 9], [0, 2, 0], 4),
    "one_match": ([1], [1], 2),
}


@pytest.mark.parametrize("name", list(SEGMENTS))
def test_segments(name):
    counts, seg_view, V = SEGMENTS[name]
    sizes = [(12 + 3 * v, 16 - v) for v in range(V)]
    _snap, want = check(MR.random_arena(counts, seg_view, sizes, seed=len(counts)), name)
    if name == "view_without_a_pair":                                      # constant planes: NaN after the division, black
        for v in (1, 3):
            assert not want["planes"][v].any() and not want["bytes"][v].any() and want["ranges"][v].tolist() == [0, 0]


# ---- 3. views of unequal size, pixel counts around the workgroups -----------------------------------------------------------------
def test_unequal_views_in_one_call():
    sizes = [(1, 1), (1, 5), (5, 1), (3, 7), (17, 33), (64, 48)]
    counts = [1, 4, 4, 30, 300, 900, 2, 50]
    snap, want = check(MR.random_arena(counts, [0, 1, 2, 3, 4, 5, 1, 4], sizes, seed=3), "unequal")
    assert [tuple(p.shape) for p in snap.planes] == sizes and want["planes"][0][0, 0] != 0
    assert want["ranges"][0, 0] == want["ranges"][0, 1] and not want["bytes"][0].any()       # the 1 x 1 view is constant


def test_pixel_counts_around_both_workgroups():
    counts_px = sorted({1, 2, 3, 4, 5, BR - 1, BR, BR + 1, 2 * BR + 1, BQ - 1, BQ, BQ + 1, 2 * BQ + 1})
    sizes = [(1, p) for p in counts_px] + [(p, 1) for p in (3, BR + 1, BQ + 1)] + [(3, (BQ - 1) // 3), (7, (2 * BQ + 1) // 7 + 1)]
    counts = [min(2 * h * w, 400) for h, w in sizes]
    snap, _ = check(MR.random_arena(counts, list(range(len(sizes))), sizes, seed=5, spill=0.5), "pixel counts")
    assert snap.layout.resolve_groups == sum(-(-h * w // BR) for h, w in sizes)


def test_the_timing_shape_seven_views():
    """7 views of 378 x 504 and 42 pairs of 2 000 matches: more pixels than the clearing launch has threads in one round."""
    V, M = 7, 2000
    sizes = [(378, 504)] * V
    snap, _ = check(MR.random_arena([M] * (V * (V - 1)), [s // (V - 1) for s in range(V * (V - 1))], sizes, seed=9), "7 views")
    assert snap.layout.pixels == 7 * 378 * 504 > 1024 * 1024


# ---- 4. planted uv ----------------------------------------------------------------------------------------------------------------
def test_planted_uv():
    H, W = 6, 9
    inf, nan = np.inf, np.nan
    planted = [(-3.25, 2.5), (W + 2.5, 1.5), (float(W), 3.5), (4.5, H - 0.5), (5.5, -0.75), (-0.0, -0.0), (2.0 ** 33, 1.2),
               (2.2, 2.0 ** 33), (-2.0 ** 33, -2.0 ** 33), (W - 1 + 0.999, H - 1 + 0.999), (np.nextafter(f32(W - 1), f32(0)), 0.5)]
    no_depth = [(inf, 1.5), (-inf, 1.5), (1.5, inf), (1.5, -inf), (nan, 1.5), (1.5, nan), (nan, inf), (inf, -inf)]
    dup = [(3.2, 3.7), (3.9, 3.1), (3.5, 3.5)]                             # three matches of one pair on pixel (3, 3)
    first = planted + no_depth + dup
    a = MR.random_arena([len(first), 12, 5], [0, 1, 0], [(H, W), (4, 4)], seed=11)
    a["uv"][:len(first)] = np.array(first, dtype=f32)
    a["uv"][-5:] = [(3.1, 3.1), (0.5, 2.5), (8.5, 1.5), (6.5, 4.5), (nan, nan)]      # the third segment: view 0 again, later in the arena
    snap, want = check(a, "planted uv")
    depth = (a["z"] * a["cam_z"]).astype(f32)
    p0 = want["planes"][0]
    n0 = len(first)
    last = n0 + 12
    # latest wins, within a pair and across the pairs of one view
    assert p0[3, 3] == depth[last] and p0[2, 0] == depth[last + 1] and p0[1, 8] == depth[last + 2]
    assert p0[3, 8] == depth[2] and p0[5, 4] == depth[3] and p0[0, 5] == depth[4] and p0[0, 0] == depth[8] and p0[5, 2] == depth[7]
    assert p0[5, 8] == depth[9] and p0[0, 7] == depth[10]
    # the matches without a finite uv are records like any other and write no depth
    written = {float(x) for x in p0[p0 != 0]}
    assert all(float(depth[k]) not in written for k in range(len(planted), len(planted) + len(no_depth))) and float(depth[-1]) not in written
    assert not np.isnan(want["xyz"][len(planted):len(planted) + len(no_depth)]).any()
    again = matchpoint.pack(inputs_of(a))
    assert again.buffer.data_ptr() != snap.buffer.data_ptr() and torch.equal(again.buffer, snap.buffer)


# ---- 5. planted values ------------------------------------------------------------------------------------------------------------
def _plant(v):
    """A colour with fp32(colour * 255) == v, searched around v / 255 (the nearest product when no fp32 factor gives v)."""
    v = f32(v)
    if not np.isfinite(v):
        return v
    c = f32(v / f32(255))
    cands, lo, hi = [c], c, c
    for _ in range(6):
        lo, hi = np.nextafter(lo, f32(-np.inf)), np.nextafter(hi, f32(np.inf))
        cands += [lo, hi]
    for x in cands:
        if f32(x * f32(255)) == v:
            return x
    return c


def test_planted_colour_bytes_and_unfused_positions():
    targets = np.array(P.PLANTED + P.PLANTED_BEYOND, dtype=f32)           # -1, 255, 256, 2^31, +-inf, NaN among them
    want_bytes = [62, 0, 1, 255, 0, 0, 0, 0, 1, 254, 255, 255, 0, 1, 194, 0, 128] + [0] * len(P.PLANTED_BEYOND)
    n = targets.size
    rng = np.random.default_rng(9)
    o, d, z = (rng.normal(size=(20000, 3)).astype(f32), rng.normal(size=(20000, 3)).astype(f32), rng.uniform(0.5, 9.0, (20000, 1)).astype(f32))
    unfused = (o + (d * z).astype(f32)).astype(f32)
    fused = (o.astype(np.float64) + d.astype(np.float64) * z.astype(np.float64)).astype(f32)     # one rounding
    rows = np.flatnonzero((unfused != fused).all(axis=1))[:T + 5]
    assert rows.size == T + 5
    N = rows.size + n
    a = MR.random_arena([N - 7, 7], [0, 1], [(8, 8), (3, 3)], seed=13)
    a["rays_o"][:rows.size], a["rays_d"][:rows.size], a["z"][:rows.size] = o[rows], d[rows], z[rows, 0]
    c = np.array([_plant(v) for v in targets], dtype=f32)
    a["color"][rows.size:, 0], a["color"][rows.size:, 1], a["color"][rows.size:, 2] = c, c[::-1], np.roll(c, 5)
    with np.errstate(all="ignore"):
        assert P.byte_rule((c * f32(255)).astype(f32)).tolist() == want_bytes
    snap, want = check(a, "planted colours")
    body = snap.host_views()[0]
    assert body[rows.size:, 24].tolist() == want_bytes and body[rows.size:, 25].tolist() == want_bytes[::-1]
    assert np.array_equal(np.ascontiguousarray(body[:rows.size, :12]).view(u32).reshape(-1, 3), MR.bits(unfused[rows]))
    assert (want["xyz"][:rows.size] != fused[rows]).all()


def test_planted_depths_per_view():
    """One view per kind of depth, so that each kind meets its own min and max."""
    nan, inf = f32(np.nan), f32(np.inf)
    den = np.array([1], u32).view(f32)[0]
    kinds = {"nan_z": [(nan, 1), (2, 1), (3, 1)], "nan_cam": [(2, nan), (1, 1)], "inf": [(inf, 1), (2, 1), (-1, 1)],
             "both_inf": [(inf, 1), (-inf, 1), (5, 1)], "inf_times_zero": [(inf, 0), (1, 1)], "negative": [(-3, 1), (-1, 2), (4, 0.5)],
             "denormal": [(den, 1), (den * 3, 1), (-den, 1)], "negative_zero": [(-0.0, 1), (2, 1)], "constant": [(2.5, 1)] * 4,
             "huge": [(3e38, 1), (-3e38, 1), (1, 1)], "only_negative_zero": [(-0.0, 1)] * 4, "tiny_range": [(1, 1), (np.nextafter(f32(1), f32(2)), 1)] * 2,
             "cam_negative": [(2, -1.5), (-1, -4), (1, 0.25)], "cam_denormal": [(1, den), (2, den)], "cam_inf": [(2, inf), (1, 1)],
             "underflow": [(1e-30, 1e-30), (1, 1)]}
    sizes = [(2, 2)] * len(kinds)
    counts = [len(v) for v in kinds.values()]
    a = MR.random_arena(counts, list(range(len(kinds))), sizes, seed=17)
    at = 0
    for vals in kinds.values():
        for k, (z, cz) in enumerate(vals):
            a["z"][at], a["cam_z"][at], a["uv"][at] = z, cz, (k % 2 + 0.5, k // 2 + 0.5)
            at += 1
    _snap, want = check(a, "planted depths")
    names = list(kinds)
    r, q = want["ranges"], want["bytes"]
    for k in ("nan_z", "nan_cam", "inf_times_zero"):                      # a NaN in the plane: a NaN range and a black image
        assert np.isnan(r[names.index(k)]).all() and not q[names.index(k)].any(), k
    assert r[names.index("inf")].tolist() == [-1, np.inf] and not q[names.index("inf")].any()      # max - min = inf: 0 or NaN everywhere
    assert r[names.index("both_inf")].tolist() == [-np.inf, np.inf] and not q[names.index("both_inf")].any()
    assert r[names.index("negative")].tolist() == [-3, 2] and q[names.index("negative")].tolist() == [[0, 51], [255, 153]]
    assert r[names.index("denormal")].tolist() == [-den, den * 3] and q[names.index("denormal")].tolist() == [[128, 255], [0, 64]]
    assert np.signbit(r[names.index("negative_zero"), 0]) and q[names.index("negative_zero")].tolist() == [[0, 255], [0, 0]]
    for k in ("constant", "only_negative_zero"):                         # 0 / 0
        i = names.index(k)
        assert r[i, 0] == r[i, 1] and not q[i].any(), k
    assert np.signbit(r[names.index("only_negative_zero")]).all()
    with np.errstate(over="ignore"):
        assert np.isinf(f32(r[names.index("huge"), 1]) - f32(r[names.index("huge"), 0]))       # the range overflows: all 0
        assert not q[names.index("huge")].any()
    assert q[names.index("tiny_range")].tolist() == [[0, 255], [0, 255]]                        # max - min is one ulp of 1
    assert r[names.index("cam_negative")].tolist() == [-3, 4] and q[names.index("cam_negative")].tolist() == [[0, 255], [118, 109]]
    assert r[names.index("cam_denormal")].tolist() == [0, den * 2] and q[names.index("cam_denormal")].tolist() == [[128, 255], [0, 0]]
    assert r[names.index("cam_inf")].tolist() == [0, np.inf] and not q[names.index("cam_inf")].any()
    assert r[names.index("underflow")].tolist() == [0, 1] and q[names.index("underflow")].tolist() == [[0, 255], [0, 0]]


def test_quantiser_edges_through_a_unit_plane():
    """A plane with min = 0 and max = 1, so that n = d: every k / 255 and (k + 0.5) / 255 and one ulp either side of both."""
    k = np.arange(256, dtype=np.float64)
    mid = np.concatenate((k / 255, (k + 0.5) / 255)).astype(f32)
    vals = np.concatenate((mid, np.nextafter(mid, f32(-1)), np.nextafter(mid, f32(2)), [f32(0), f32(1)])).astype(f32)
    vals = vals[(vals >= 0) & (vals <= 1)]
    n = vals.size
    a = MR.random_arena([n], [0], [(1, n)], seed=19)
    a["z"][:], a["cam_z"][:] = vals, 1
    a["uv"][:, 0], a["uv"][:, 1] = np.arange(n) + 0.5, 0.5
    _snap, want = check(a, "quantiser edges")
    assert want["ranges"].tolist() == [[0, 1]] and np.array_equal(want["norm"][0][0], vals)
    q = want["bytes"][0][0].astype(np.int64)
    exact = vals.astype(np.float64) * 255 + 0.5
    assert np.abs(q - np.floor(exact)).max() <= 1 and set(q.tolist()) == set(range(256))


# ---- 6. the reference's recorded arrays -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", MR.SCENES)
@pytest.mark.parametrize("how", ["flat", "view_gs"])
def test_fixture_every_array(tag, how):
    import eval_refs as E
    fx, arena = np.load(MR.GOLDEN), MR.golden_arena(np.load(MR.SEED_GOLDEN), tag)
    inputs = inputs_of(arena) if how == "flat" else matchpoint.MatchpointInputs.from_view_gs(MR.view_gs_of(arena, DEV))
    assert inputs.sizes == arena["sizes"] and [s[2:] for s in inputs.segments] == [s[2:] for s in inputs_of(arena).segments]
    snap = matchpoint.pack(inputs)
    body, planes, byte_planes, ranges = snap.host_views()
    assert np.array_equal(np.ascontiguousarray(body[:, :12]).view(u32).reshape(-1, 3), MR.bits(fx[f"{tag}_xyz"]))
    assert not body[:, 12:24].any() and np.array_equal(body[:, 24:], P.byte_rule(fx[f"{tag}_rgb"]))
    assert np.array_equal(body[:, 24:], fx[f"{tag}_rgb"].astype(np.uint8))                 # all inside 0..255: numpy's cast is defined
    for v in range(len(arena["sizes"])):
        raw, norm = fx[f"{tag}_raw_{v}"], fx[f"{tag}_norm_{v}"]
        assert np.array_equal(planes[v].view(u32), raw.view(u32)), v
        assert np.array_equal(byte_planes[v], E.quantise(torch.from_numpy(norm)).numpy()), v
        assert ranges[v].tolist() == [raw.min(), raw.max()]
    assert_snapshot(snap, MR.restate(arena), (tag, how))
    if how == "view_gs":
        assert snap.keys == [f"view{v}" for v in range(len(arena["sizes"]))]


# ---- 7. the seeding step's sparse depths ------------------------------------------------------------------------------------------
def test_depth_planes_equal_the_seeding_steps():
    V, H, W = 3, 20, 31
    counts, seg_view = [300, 1, 257, 64, 0, 129], [0, 0, 1, 1, 2, 2]
    a = MR.random_arena(counts, seg_view, [(H, W)] * V, seed=23)
    a["uv"][5], a["uv"][6], a["uv"][7] = (np.nan, 2), (np.inf, 2), (2.0 ** 33, 2)
    a["uv"][400:420] = a["uv"][300:320]                                   # the pixels of view 1's first pair hit again, later
    t = tensors(a)
    s_in = seed.SeedInputs.from_flat(t["rays_o"], t["rays_d"], t["z"], t["color"], t["uv"], t["cam_z"], counts, seg_view, V, H, W)
    sparse = seed.seed_arrays(s_in, None)["sparse_depths"]
    snap = matchpoint.pack(inputs_of(a, t))
    assert torch.equal(torch.stack(snap.planes).view(torch.int32), sparse.view(torch.int32))
    assert int((sparse != 0).sum()) > 500


# ---- 8. files -----------------------------------------------------------------------------------------------------------------------
def _read_back(folder, name, keys, want):
    raw = (folder / name).read_bytes()
    assert raw == MR.ply_bytes(want)
    for v, k in enumerate(keys):
        plane = np.load(folder / f"{k}.npy")
        assert plane.dtype == f32 and MR.same_bits(plane, want["planes"][v]), k
        img = np.asarray(Image.open(folder / f"sparsedepth_{k}.png"))
        assert img.dtype == np.uint8 and img.shape == want["bytes"][v].shape + (3,), k
        assert all(np.array_equal(img[:, :, c], want["bytes"][v]) for c in range(3)), k
    assert sorted(os.listdir(folder)) == sorted([name] + [f"{k}.npy" for k in keys] + [f"sparsedepth_{k}.png" for k in keys])


def test_write_is_read_back(tmp_path):
    sizes = [(17, 33), (1, 5), (64, 48)]
    a = MR.random_arena([70, 40, 3, 129], [0, 0, 1, 2], sizes, seed=29)           # in the order a view_gs is walked
    a["color"] = np.clip(a["color"], 0, 0.999).astype(f32)
    want = MR.restate(a)
    snap = matchpoint.pack(inputs_of(a))
    folder = tmp_path / "init_point_cloud" / "iteration_2000"             # the directory is created
    snap.write(str(folder / "point_cloud_matchpoint.ply"))
    _read_back(folder, "point_cloud_matchpoint.ply", [0, 1, 2], want)
    # the file is ply_io.write_vertex_ply's, byte for byte
    cols = np.concatenate((want["xyz"], np.zeros_like(want["xyz"]), want["rgb"]), axis=1)
    ply_io.write_vertex_ply(str(tmp_path / "old.ply"), P.COLOR_NAMES, cols, ["f4"] * 6 + ["u1"] * 3)
    assert (tmp_path / "old.ply").read_bytes() == (folder / "point_cloud_matchpoint.ply").read_bytes()
    # ... and through the model's method, from a view_gs with names
    g = type("G", (), {})()
    g.view_gs = MR.view_gs_of(a, DEV)
    matchpoint.install(g)
    g.save_ply_at_matchpoint(str(tmp_path / "named" / "cloud.ply"))
    _read_back(tmp_path / "named", "cloud.ply", list(g.view_gs), want)


class Model:
    """The attribute names of the reference's GaussianModel that the seeding step writes."""
    max_sh_degree = 3
    active_sh_degree = 0


def test_drop_in_between_the_init_stage_and_create_from_pcd(tmp_path, capsys):
    rng = np.random.default_rng(31)
    cams = MonoR.cameras([(48, 64)] * 3, rng, fovs=[55.0] * 3)
    md = MonoR.match_data(cams, 150, rng)
    gm = Model()
    mono.install(gm, DEV)
    gm.create_from_mono(cams, md, 2.5, u=rng.random(6 * 150, dtype=np.float32))
    setup = gm.mono_setup
    stage = InitStage.from_mono(setup)
    seed.install(gm, stage)
    matchpoint.install(gm, stage)
    stage.run(6)
    stage.load_best(gm.view_gs)
    stage.min_loss[::2] = 0.01                                            # some matches are kept and some dropped
    stage.min_loss[1::2] = 0.5
    state = stage.min_loss_state()
    seed_inputs = seed.SeedInputs.from_mono(setup, stage)
    twin = Model()
    seed.create_from_pcd(twin, state, stage=stage, inputs=seed_inputs)    # the model without the snapshot
    before = setup.arena.clone()
    path = tmp_path / "init_point_cloud" / "iteration_2000" / "point_cloud_matchpoint.ply"
    gm.save_ply_at_matchpoint(str(path))
    assert torch.equal(before, setup.arena)                               # z, uv, colours, rays, tables: bitwise unchanged
    inputs = matchpoint.MatchpointInputs.from_mono(setup, stage)
    for k in ("color", "uv", "cam_z", "rays_o", "rays_d", "z"):           # read in place: nothing was copied
        assert getattr(inputs, k).data_ptr() == getattr(setup, k).data_ptr(), k
    assert inputs.table_dev.data_ptr() == setup.seed_table.data_ptr()
    arena = {k: getattr(setup, k).cpu().numpy() for k in MR.IN_KEYS}
    arena.update(counts=[s[3] for s in setup.segments], seg_view=[setup.keys.index(s[0]) for s in setup.segments], sizes=[(48, 64)] * 3)
    _read_back(path.parent, path.name, setup.keys, MR.restate(arena))
    gm.create_from_pcd(state, inputs=seed_inputs)
    n = gm._zval.shape[0]
    assert 0 < n < stage.N and f"Number of points at initialisation :  {n}" in capsys.readouterr().out
    for k in ("_zval", "_rayo", "_rayd", "_features_dc", "_features_rest", "_scaling", "_rotation", "_opacity", "sparse_depths", "masks"):
        x, y = getattr(gm, k).detach(), getattr(twin, k).detach()
        assert x.shape == y.shape and torch.equal(x.view(torch.uint8) if x.dtype == torch.bool else x.view(torch.int32),
                                                  y.view(torch.uint8) if y.dtype == torch.bool else y.view(torch.int32)), k
    # the snapshot holds every match, the seeded model the kept ones
    assert os.path.getsize(path) == len(MR.ply_bytes({"body": np.zeros((stage.N, 27), np.uint8)}))


# ---- 9. schedule ------------------------------------------------------------------------------------------------------------------
def _schedule_arena(seed_=37):
    return MR.random_arena([G + 1, 40, 300], [0, 1, 2], [(17, 33), (5, 1), (40, 30)], seed=seed_)


def test_pack_in_a_graph_replays_on_rewritten_depths():
    a = _schedule_arena()
    t = tensors(a)
    inputs = inputs_of(a, t)
    matchpoint.pack(inputs)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        snap = matchpoint.pack(inputs)
    b = _schedule_arena(41)
    for k in ("z", "uv", "color"):
        t[k].copy_(torch.from_numpy(b[k]).to(DEV))
        a[k] = b[k]
    snap.buffer.fill_(0xAB)
    graph.replay()
    torch.cuda.synchronize()
    assert_snapshot(snap, MR.restate(a), "replayed")


def test_a_call_on_a_side_stream():
    a = _schedule_arena(43)
    inputs = inputs_of(a)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        snap = matchpoint.pack(inputs)
        assert_snapshot(snap, MR.restate(a), "side stream")
    torch.cuda.current_stream().wait_stream(side)


def test_save_ply_at_matchpoint_reads_the_device_once(tmp_path, monkeypatch):
    a = _schedule_arena(47)
    g = type("G", (), {})()
    g.view_gs = MR.view_gs_of(a, DEV)
    inputs = matchpoint.MatchpointInputs.from_view_gs(g.view_gs)
    matchpoint.save_ply_at_matchpoint(g, str(tmp_path / "warm" / "cloud.ply"))
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
    snap = matchpoint.pack(inputs)
    assert reads == []
    host = snap.to_host()
    snap.write(str(tmp_path / "parts" / "cloud.ply"))
    assert reads == ["to"] and host.is_pinned()
    matchpoint.save_ply_at_matchpoint(g, str(tmp_path / "whole" / "cloud.ply"))            # packs the inputs from view_gs itself
    matchpoint.save_ply_at_matchpoint(g, str(tmp_path / "given" / "cloud.ply"), inputs=inputs)
    monkeypatch.undo()
    assert reads == ["to", "to", "to"], reads
    names = sorted(os.listdir(tmp_path / "warm"))
    assert len(names) == 7
    for folder in ("parts", "whole", "given"):
        assert sorted(os.listdir(tmp_path / folder)) == names
        assert all((tmp_path / folder / n).read_bytes() == (tmp_path / "warm" / n).read_bytes() for n in names)

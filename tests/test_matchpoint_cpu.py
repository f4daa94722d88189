"""CPU-only checks of the init stage's snapshot (scgaussian_amd/matchpoint.py, libscg_mp.so, include/mp/scg_matchpoint.h): the
numpy restatement the GPU tests compare against (tests/matchpoint_refs.py) is held to the arrays the reference's own
save_ply_at_matchpoint handed its writers (tests/golden/ref_matchpoint.npz) bit for bit — every operation is one IEEE fp32
operation on both sides, so there is no tolerance — and its file to ply_io.write_vertex_ply's; the fourth library and its binding
to the header's text; the library's validation to its codes; the layout to its arithmetic."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import matchpoint_refs as MR
import ply_refs as P
from abi_compare import ANY, check_side_library
from scgaussian_amd import _lib, _lib_mp, matchpoint, ply_io
FX = np.load(MR.GOLDEN)
SEED_FX = np.load(MR.SEED_GOLDEN)


# ---- the restatement against the reference's recorded arrays --------------------------------------------------------------------
@pytest.mark.parametrize("tag", MR.SCENES)
def test_restatement_equals_the_reference_bit_for_bit(tag):
    arena = MR.golden_arena(SEED_FX, tag)
    assert MR.pair_pixels_distinct(arena) and np.array_equal(FX[f"{tag}_sizes"], np.array(arena["sizes"]))
    assert len(set(arena["sizes"])) == (2 if tag == "A" else 1)
    got = MR.restate(arena)
    assert MR.same_bits(got["xyz"], FX[f"{tag}_xyz"]) and MR.same_bits(got["rgb"], FX[f"{tag}_rgb"])
    assert not np.isnan(got["xyz"]).any()
    for v in range(len(arena["sizes"])):
        raw, norm = FX[f"{tag}_raw_{v}"], FX[f"{tag}_norm_{v}"]
        assert np.array_equal(got["planes"][v].view(np.uint32), raw.view(np.uint32)), (tag, v)
        assert np.array_equal(got["norm"][v].view(np.uint32), norm.view(np.uint32)), (tag, v)
        assert got["ranges"][v, 0] == raw.min() and got["ranges"][v, 1] == raw.max()
        assert got["bytes"][v].min() == 0 and got["bytes"][v].max() == 255
    assert sum(int((FX[f"{tag}_raw_{v}"] != 0).sum()) for v in range(len(arena["sizes"]))) > 100
    # the fixture holds exactly these arrays and is smaller than the one its inputs come from
    want = {f"{tag}_{k}" for k in ("sizes", "xyz", "rgb")} | {f"{tag}_{k}_{v}" for k in ("raw", "norm") for v in range(len(arena["sizes"]))}
    assert {k for k in FX.files if k.startswith(tag + "_")} == want
    assert os.path.getsize(MR.GOLDEN) < os.path.getsize(MR.SEED_GOLDEN)


def test_recorded_scene_keeps_the_planted_pixels():
    arena = MR.golden_arena(SEED_FX, "A")
    pairs = [tuple(int(x) for x in p) for p in SEED_FX["A_pairs"]]
    offs = np.concatenate([[0], np.cumsum(arena["counts"])])
    big, b2 = int(offs[pairs.index((2, 1))]), int(offs[pairs.index((2, 0))])
    assert np.array_equal(arena["uv"][big + 4:big + 10], SEED_FX["A_in_uv"][big + 4:big + 10])
    v = arena["seg_view"][pairs.index((2, 1))]
    H, W = arena["sizes"][v]
    px = [MR.pixel_of(u, w, H, W) for u, w in arena["uv"][big + 4:big + 10]]
    assert [p[1] for p in px[:3]] == [0, W - 1, W - 1] and px[3][0] == H - 1 and px[4][0] == 0
    assert px[5] == MR.pixel_of(*arena["uv"][b2], H, W)                    # one pixel from two pairs of one view
    later = max(big + 9, b2)
    assert FX[f"A_raw_{v}"][px[5]] == np.float32(arena["z"][later] * arena["cam_z"][later])
    # the cropped view: matches beyond its smaller size land on its last row and column
    Hc, Wc = arena["sizes"][1]
    assert (Hc, Wc) == (40, 70) and (FX["A_raw_1"][Hc - 1] != 0).sum() > 3 and (FX["A_raw_1"][:, Wc - 1] != 0).sum() > 3


@pytest.mark.parametrize("tag", MR.SCENES)
def test_restated_file_is_ply_ios(tmp_path, tag):
    r = MR.restate(MR.golden_arena(SEED_FX, tag))
    cols = np.concatenate((r["xyz"], np.zeros_like(r["xyz"]), r["rgb"]), axis=1)
    assert r["rgb"].min() >= 0 and r["rgb"].max() < 256                    # where numpy's cast is defined
    path = tmp_path / "point_cloud_matchpoint.ply"
    ply_io.write_vertex_ply(str(path), P.COLOR_NAMES, cols, ["f4"] * 6 + ["u1"] * 3)
    assert path.read_bytes() == MR.ply_bytes(r)


def test_restatement_rules_on_a_hand_made_scene():
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    a = MR.random_arena([4, 3], [0, 1], [(3, 4), (2, 2)], seed=1)
    a["uv"][:] = [(1.5, 1.5), (1.2, 1.9), (-3, 7), (inf, 1), (0.5, 0.5), (nan, 0), (2 ** 33, -2 ** 33)]
    a["z"][:] = [1, 2, 3, 4, -0.0, 6, 7]
    a["cam_z"][:] = 1
    r = MR.restate(a)
    assert r["planes"][0].tolist() == [[0, 0, 0, 0], [0, 2, 0, 0], [3, 0, 0, 0]]          # latest wins; inf writes nothing
    assert r["planes"][1].tolist() == [[0, 7], [0, 0]] and np.signbit(r["planes"][1][0, 0])      # NaN writes nothing, 2^33 is clamped
    assert r["ranges"].tolist() == [[0, 3], [0, 7]] and np.signbit(r["ranges"][1, 0])             # among the zeros -0.0 is the min
    assert r["bytes"][0][1, 1] == 170 and r["bytes"][0][2, 0] == 255 and r["bytes"][1].tolist() == [[0, 255], [0, 0]]
    a["uv"][6] = (0.2, 0.2)
    r = MR.restate(a)                                                       # the later match takes the pixel of the -0.0
    assert r["planes"][1].tolist() == [[7, 0], [0, 0]] and not np.signbit(r["ranges"][1, 0])
    a["z"][6] = nan
    r = MR.restate(a)
    assert np.isnan(r["ranges"][1]).all() and not r["bytes"][1].any() and r["body"].shape == (7, 27)


# ---- the fourth library against its header --------------------------------------------------------------------------------------
def test_fourth_library_exports_and_binds_exactly_its_header():
    abi = check_side_library(_lib_mp, "mp", "scg_matchpoint.h", ANY)
    assert len(abi.functions) == 6 and list(abi.structs) == ["ScgMpLayout", "ScgMpView", "ScgMpPack"]
    assert not any(f.array for fields in abi.structs.values() for f in fields)
    assert sorted(abi.defines) == sorted("SCG_" + n for n in (
        "MP_ABI_VERSION", "MP_RECORD_BYTES", "MP_TILE_RECORDS", "MP_MATCH_GROUP", "MP_RESOLVE_PIXELS", "MP_QUANT_PIXELS",
        "MP_MAX_SEGMENTS", "MP_MAX_VIEWS", "MP_MAX_DIM", "MP_MAX_MATCHES", "MP_MAX_PIXELS"))
    assert [_lib_mp.load().scg_mp_struct_bytes(k) for k in range(-1, 4)] == [0, 96, 24, 96, 0]
    assert [C.sizeof(s) for s in _lib_mp.STRUCTS] == [96, 24, 96]
    assert _lib_mp.MP_MATCH_GROUP % _lib_mp.MP_TILE_RECORDS == 0 and (_lib_mp.MP_TILE_RECORDS * _lib_mp.MP_RECORD_BYTES) % 4 == 0
    assert _lib_mp.MP_MAX_SEGMENTS == _lib.SEED_MAX_SEGMENTS


# ---- the layout -----------------------------------------------------------------------------------------------------------------
def _hw(sizes):
    return (C.c_int32 * (2 * len(sizes)))(*[x for s in sizes for x in s])


def _layout(N, sizes):
    L, views = _lib_mp.ScgMpLayout(), (_lib_mp.ScgMpView * len(sizes))()
    rc = _lib_mp.load().scg_mp_layout(N, len(sizes), _hw(sizes), C.byref(L), views)
    return rc, L, views


def test_layout_arithmetic():
    lib = _lib_mp.load()
    for N, sizes in ((0, [(1, 1)]), (1, [(1, 1)]), (5, [(1, 5), (5, 1), (3, 7)]), (65, [(17, 33), (64, 48)]), (4000, [(378, 504)] * 7),
                     (2 ** 31 - 1, [(65535, 16383)]), (3, [(1, 1)] * 1024)):
        rc, L, views = _layout(N, sizes)
        assert rc == 0
        px = [h * w for h, w in sizes]
        pad = [(p + 3) // 4 * 4 for p in px]
        assert (L.body_offset, L.body_bytes) == (0, (27 * N + 3) // 4 * 4)
        assert (L.depth_bytes, L.byte_bytes, L.range_bytes, L.pixels) == (4 * sum(px), sum(pad), 8 * len(sizes), sum(px))
        assert L.resolve_groups == sum(-(-p // 256) for p in px) and L.quant_groups == sum(-(-p // 1024) for p in px)
        ends = (L.body_bytes, L.depth_offset + L.depth_bytes, L.byte_offset + L.byte_bytes, L.range_offset + L.range_bytes)
        for end, nxt in zip(ends, (L.depth_offset, L.byte_offset, L.range_offset, L.total)):
            assert nxt % 256 == 0 and 0 <= nxt - end < 256
        for v, rec in enumerate(views):
            assert (rec.H, rec.W) == sizes[v] and rec.first_pixel == sum(px[:v]) and rec.first_byte == sum(pad[:v])
            assert rec.resolve_group == sum(-(-p // 256) for p in px[:v]) and rec.quant_group == sum(-(-p // 1024) for p in px[:v])
        assert lib.scg_mp_workspace_bytes(len(sizes), _hw(sizes)) == 4 * sum(px) + 8 * L.resolve_groups
    assert lib.scg_mp_layout(1, 1, _hw([(1, 1)]), C.byref(L), None) == 0             # the view table is optional
    # what it refuses
    assert lib.scg_mp_layout(1, 1, _hw([(1, 1)]), None, None) == -1 and b"out is NULL" in lib.scg_mp_last_error()
    assert lib.scg_mp_layout(1, 1, None, C.byref(L), None) == -1
    assert lib.scg_mp_layout(-1, 1, _hw([(1, 1)]), C.byref(L), None) == -2
    assert lib.scg_mp_layout(1, 0, _hw([(1, 1)]), C.byref(L), None) == -2 and lib.scg_mp_layout(1, 1025, _hw([(1, 1)] * 1025), C.byref(L), None) == -2
    for bad in ((0, 5), (5, 0), (65536, 1), (1, 65536), (-3, 4)):
        assert _layout(1, [(2, 2), bad])[0] == -2 and b"view 1" in lib.scg_mp_last_error()
        assert lib.scg_mp_workspace_bytes(2, _hw([(2, 2), bad])) == 0
    assert _layout(1, [(65535, 65535)])[0] == -2 and b"2^31" in lib.scg_mp_last_error()      # a single view beyond the pixel limit
    assert _layout(1, [(32768, 32768), (32768, 32768)])[0] == -2                            # ... and two that are so together
    assert lib.scg_mp_workspace_bytes(0, None) == 0


# ---- validation, without a GPU ----------------------------------------------------------------------------------------------------
def _args(N, counts, seg_view, sizes, fake=0x1000):
    """(ScgMpPack with fake device pointers, layout, the objects that keep its host tables alive)."""
    rc, L, views = _layout(N, sizes)
    assert rc == 0
    seg = (_lib.ScgSeedSegment * len(counts))()
    off = 0
    for s, (M, v) in enumerate(zip(counts, seg_view)):
        seg[s].offset, seg[s].count, seg[s].view = off, M, v
        off += M
    a = _lib_mp.ScgMpPack()
    a.struct_bytes = C.sizeof(a)
    a.N, a.V, a.nseg = N, len(sizes), len(counts)
    a.segments, a.views = C.addressof(seg), C.addressof(views)
    for n in ("segments_dev", "views_dev", "rays_o", "rays_d", "z", "color", "uv", "cam_z"):
        setattr(a, n, fake)
    return a, L, (seg, views)


def test_validation_returns_codes_without_a_gpu():
    """Every call below fails its validation before anything touches a device: the device pointers are never dereferenced."""
    lib = _lib_mp.load()
    fake, big = 0x1000, 1 << 24
    call = lambda a, buf=fake, nbuf=big, ws=fake, nws=big: lib.scg_mp_pack(C.byref(a), buf, nbuf, ws, nws, None)      # noqa: E731
    err = lib.scg_mp_last_error
    sizes = [(3, 7), (5, 4)]
    a, L, keep = _args(10, [4, 0, 6], [0, 1, 1], sizes)
    assert lib.scg_mp_pack(None, fake, big, fake, big, None) == -1 and b"args is NULL" in err()
    # buffers
    assert call(a, buf=None) == -1 and call(a, ws=None) == -1
    assert call(a, nbuf=L.total - 1) == -4 and b"buffer of" in err()
    assert call(a, nws=4 * 41 + 8 * 2 - 1) == -4 and b"workspace of" in err()
    assert call(a, buf=fake + 8) == -5 and call(a, ws=fake + 2) == -5
    # the struct and the counts
    a.struct_bytes -= 8
    assert call(a) == -2 and b"struct_bytes" in err()
    a.struct_bytes += 8
    for field, bad in (("N", 0), ("N", -1), ("V", 0), ("V", 1025), ("nseg", 0), ("nseg", 1025)):
        old = getattr(a, field)
        setattr(a, field, bad)
        assert call(a) == -2, (field, bad)
        setattr(a, field, old)
    # null pointers
    for n in ("segments", "segments_dev", "views", "views_dev", "rays_o", "rays_d", "z", "color", "uv", "cam_z"):
        old = getattr(a, n)
        setattr(a, n, None)
        assert call(a) == -1, n
        setattr(a, n, old)
    a.uv = fake + 2
    assert call(a) == -5 and b"4-byte" in err()
    a.uv = fake
    # the segment table: a gap, an overlap, a view out of range, a negative count, a short and a long cover
    seg = keep[0]
    seg[2].offset = 5
    assert call(a) == -2 and b"segment 2 starts at 5" in err()
    seg[2].offset = 3
    assert call(a) == -2 and b"segment 2 starts at 3" in err()
    seg[2].offset = 4
    for bad in (2, -1):
        seg[1].view = bad
        assert call(a) == -2 and b"segment 1 has view" in err()
    seg[1].view = 1
    seg[1].count = -1
    assert call(a) == -2
    seg[1].count = 0
    seg[2].count = 5
    assert call(a) == -2 and b"cover 9 of N = 10" in err()
    seg[2].count = 7
    assert call(a) == -2 and b"runs past N = 10" in err()
    seg[2].count = 6
    # the view table: a size out of range, a record that is not the layout's
    views = keep[1]
    views[1].W = 0
    assert call(a) == -2 and b"view 1" in err()
    views[1].W = 65536
    assert call(a) == -2
    views[1].W = 4
    for field in ("first_pixel", "first_byte", "resolve_group", "quant_group"):
        setattr(views[1], field, getattr(views[1], field) + 1)
        assert call(a) == -2 and b"the layout gives" in err(), field
        setattr(views[1], field, getattr(views[1], field) - 1)
    views[0].H = 4                                                     # a taller first view moves the second one's planes
    assert call(a) == -2 and b"view 1" in err()
    views[0].H = 3
    # limits: too many pixels
    a2, _L2, keep2 = _args(1, [1], [0], [(2, 2), (2, 2)])
    keep2[1][0].H, keep2[1][0].W, keep2[1][1].H, keep2[1][1].W = 32768, 32768, 32768, 32768
    assert call(a2) == -2 and b"2^31" in err()


def test_python_entry_points_refuse_host_tensors_and_empty_models():
    a = MR.random_arena([3, 2], [0, 1], [(4, 4), (2, 3)])
    t = {k: torch.from_numpy(a[k]) for k in MR.IN_KEYS}
    with pytest.raises(_lib.ScgError, match="no CPU path"):
        matchpoint.MatchpointInputs.from_flat(t["rays_o"], t["rays_d"], t["z"], t["color"], t["uv"], t["cam_z"], a["counts"],
                                              a["seg_view"], a["sizes"])
    with pytest.raises(_lib.ScgError, match="no CPU path"):
        matchpoint.MatchpointInputs.from_view_gs(MR.view_gs_of(a))
    with pytest.raises(_lib.ScgError, match="no match pair"):
        matchpoint.MatchpointInputs.from_view_gs({"a": {"height": 4, "width": 4, "match_infos": {}}})
    with pytest.raises(_lib.ScgError, match="no view"):
        matchpoint.MatchpointInputs.from_view_gs({})
    with pytest.raises(_lib.ScgError, match="no view_gs"):
        matchpoint.save_ply_at_matchpoint(object(), "nowhere.ply")
    g = type("G", (), {})()
    matchpoint.install(g)
    assert g.save_ply_at_matchpoint.func is matchpoint.save_ply_at_matchpoint
    lay, views = matchpoint.layout_of(5, [(3, 7), (5, 4)])
    assert lay.pixels == 41 and views["first_byte"].tolist() == [0, 24] and views.dtype.itemsize == 24
    with pytest.raises(_lib.ScgError, match="65535"):
        matchpoint.layout_of(5, [(3, 65536)])

"""The scene setup without a GPU: the numpy restatement (tests/mono_refs.py) against the reference's own create_from_mono
(tests/golden/ref_mono.npz), the host constants, the C entries' argument codes, and the dictionary over the arena.

Bars against the fixture.  uv, z, image_color, intr, w2c and valid: bit for bit.  color, blender_mask, rays_o, rays_d, cam_rays_d:
within max(4 e_ref, 1 fp32 ulp) of the float64 yardstick (mono_refs.bar): e_ref is the reference's own fp32 deviation from it on the
same input, computed here from the fixture; the factor 4 is the one tests/test_gpu_eval.py uses."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import mono_refs as MR
from scgaussian_amd import _lib, mono

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_mono.npz")
E_NULL, E_RANGE, E_ALIGN = -1, -2, -5


@pytest.fixture(scope="module")
def fx():
    cams, md, u, ref = MR.fixture_scene(np.load(GOLDEN))
    plan = mono.MonoPlan(cams, md, u)
    return cams, md, u, ref, plan, MR.restate(plan), MR.restate(plan, wide=True)


def test_restatement_is_the_reference_bit_for_bit_where_the_rule_is_exact(fx):
    cams, _md, _u, ref, plan, got, _wide = fx
    assert plan.N == 2 * (2 + 65 + 257) and [s[3] for s in plan.segments] == [2, 65, 2, 257, 65, 257]
    for k in ("uv", "z", "valid"):
        assert np.array_equal(got[k], ref[k]), k
    p0 = 0
    for i, c in enumerate(plan.consts):
        n = c["H"] * c["W"]
        assert np.array_equal(got["image_color"][p0:p0 + n].reshape(c["H"], c["W"], 3), ref["image_color"][i])
        assert np.array_equal(c["intr32"], ref["intr"][i]) and np.array_equal(c["w2c32"], ref["w2c"][i])
        assert np.array_equal(plan.near_far[i], ref["near_far"][i])
        p0 += n
    assert 0 < got["valid"].sum() < plan.N                     # the masks decide something
    edge = got["blender_mask"][:67]                            # view 0 has no mask: the sum of the in-bounds weights
    assert (edge == 0).any() and ((edge > 0) & (edge < 0.999)).any() and (edge > 0.999).any()


def test_restatement_is_within_the_reference_own_error_of_float64(fx):
    _cams, _md, _u, ref, _plan, got, wide = fx
    for k in ("color", "blender_mask", "rays_o", "rays_d", "cam_rays_d"):
        tol, e_ref = MR.bar(ref[k], wide[k])
        e = float(np.max(np.abs(got[k].astype(np.float64) - wide[k])))
        print(f"{k}: restatement {e:.3e}, reference {e_ref:.3e}, bar {tol:.3e}")
        assert e <= tol, (k, e, tol)


def test_byte_over_255_is_the_correctly_rounded_quotient():
    b = np.arange(256)
    want = (b.astype(np.float64) / 255.0).astype(np.float32)      # fp64 quotient of two small integers, rounded once: exact enough
    got = b.astype(np.float32) / np.float32(255)                  # that double rounding cannot bite (no quotient lies near a tie)
    assert np.array_equal(got, want) and np.array_equal(got, (torch.arange(256).float() / 255.0).numpy())


def test_view_constants_invert_the_fp32_matrices(fx):
    cams = fx[0]
    for cam in cams:
        c = mono.view_constants(cam)
        assert c["intr32"].dtype == np.float32 and c["w2c32"].dtype == np.float32 and c["Kinv"].dtype == np.float64
        assert np.abs(c["intr32"].astype(np.float64) @ c["Kinv"] - np.eye(3)).max() < 1e-14
        assert np.abs(c["w2c32"].astype(np.float64) @ c["c2w"] - np.eye(4)).max() < 1e-14
        assert np.array_equal(c["Rw2c"], c["w2c32"][:3, :3].astype(np.float64))
        H, W = np.asarray(cam.image).shape[:2]
        assert c["intr32"][0, 0] == np.float32(mono.fov2focal(cam.FovX, W)) and c["intr32"][1, 2] == np.float32(H / 2.0)
        # no orthonormality assumed: a sheared "rotation" is still inverted
    cam = MR.camera("s", cams[0].image, np.array([[1.0, 0.2, 0], [0, 1.1, 0.1], [0.3, 0, 0.9]]), (0.1, 0.2, 0.3), 1.0, 0.8, (1, 2))
    c = mono.view_constants(cam)
    assert np.abs(c["w2c32"].astype(np.float64) @ c["c2w"] - np.eye(4)).max() < 1e-14


def _args():
    a = _lib.ScgMono()
    a.struct_bytes = C.sizeof(_lib.ScgMono)
    a.V, a.nseg, a.ngroups, a.N = 2, 2, 2, 10
    a.image_pixels, a.mask_pixels, a.max_view_pixels = 200, 0, 100
    for name, _t in _lib.ScgMono._fields_[9:]:
        setattr(a, name, 0x1000)
    a.masks = None
    return a


def test_argument_codes_without_a_gpu():
    lib = _lib.load()
    assert lib.scg_mono_block() == 256
    assert [lib.scg_mono_struct_bytes(k) for k in range(5)] == [C.sizeof(_lib.ScgMono), 272, 16, 8, 0]
    calls = (lib.scg_mono_images, lib.scg_mono_matches, lib.scg_mono_pairs)
    for call in calls:
        assert call(None, None) == E_NULL
        for field, value in (("struct_bytes", 8), ("V", 0), ("V", 1025), ("nseg", 0), ("nseg", 65537), ("N", 0), ("ngroups", 0),
                             ("ngroups", 1 << 24), ("max_view_pixels", 0), ("max_view_pixels", 201), ("mask_pixels", -1)):
            a = _args()
            setattr(a, field, value)
            assert call(C.byref(a), None) == E_RANGE, field
        a = _args()
        a.image_pixels, a.max_view_pixels = 1 << 32, 1 << 31
        assert call(C.byref(a), None) == E_RANGE
        for name, _t in _lib.ScgMono._fields_[9:]:
            if name == "masks":                            # NULL is what a scene without masks passes
                continue
            a = _args()
            setattr(a, name, None)
            assert call(C.byref(a), None) == E_NULL, name
        a = _args()
        a.mask_pixels = 5                                  # masks NULL with pixels to read
        assert call(C.byref(a), None) == E_NULL
        a = _args()
        a.views = 0x1004
        assert call(C.byref(a), None) == E_ALIGN
        a = _args()
        a.uv = 0x1002
        assert call(C.byref(a), None) == E_ALIGN
        a = _args()
        a.masks, a.mask_pixels = 0x1002, 5
        assert call(C.byref(a), None) == E_ALIGN
        assert b"aligned" in lib.scg_last_error()
    with pytest.raises(_lib.ScgError, match="GPU"):
        mono.MonoSetup.build([], {}, device="cpu")


def test_plan_refuses_what_the_kernels_do_not_take(fx):
    cams, md, u = fx[0], fx[1], fx[2]
    bad = {a: dict(v) for a, v in md.items()}
    bad[cams[0].image_name][cams[1].image_name] = np.zeros((3, 2))
    with pytest.raises(_lib.ScgError, match="its reverse"):
        mono.MonoPlan(cams, bad, None)
    with pytest.raises(_lib.ScgError, match="u holds"):
        mono.MonoPlan(cams, md, u[:-1])
    f = MR.camera("f", cams[0].image.astype(np.float32), np.eye(3), (0, 0, 0), 1.0, 1.0, (1, 2))
    with pytest.raises(_lib.ScgError, match="uint8"):
        mono.MonoPlan([f, cams[1]], {"f": {cams[1].image_name: np.zeros((1, 2))}, cams[1].image_name: {"f": np.zeros((1, 2))}})


def test_dictionary_keys_shapes_and_arena_order(fx):
    cams, md, _u, ref, plan, got, _wide = fx
    arena = torch.zeros(plan.total_bytes, dtype=torch.uint8)
    plan.fill(arena)
    vg = plan.view_gs(arena)
    assert list(vg.keys()) == [c.image_name for c in cams] == plan.keys
    lo, hi = arena.data_ptr(), arena.data_ptr() + arena.numel()
    walked, off = [], 0
    for i, (a, v) in enumerate(vg.items()):
        assert tuple(v.keys()) == mono.PER_VIEW
        H, W = plan.consts[i]["H"], plan.consts[i]["W"]
        assert (v["height"], v["width"]) == (H, W) and v["image_color"].shape == (H, W, 3)
        assert v["intr"].shape == (3, 3) and v["w2c"].shape == (4, 4) and v["near_far"].shape == (2,)
        assert np.array_equal(v["intr"].numpy(), ref["intr"][i]) and np.array_equal(v["w2c"].numpy(), ref["w2c"][i])
        assert np.array_equal(v["near_far"].numpy(), ref["near_far"][i])
        assert list(v["match_infos"].keys()) == [c.image_name for c in cams if c.image_name != a]
        for b, info in v["match_infos"].items():
            M = np.asarray(md[a][b]).shape[0]
            assert tuple(info.keys()) == mono.PER_PAIR
            assert isinstance(info["z_val"], torch.nn.Parameter) and info["z_val"].shape == (M, 1) and info["z_val"].requires_grad
            for k, tail in (("rays_o", 3), ("rays_d", 3), ("cam_rays_d", 3), ("color", 3), ("uv", 2), ("match_pixel", 2)):
                assert info[k].shape == (M, tail) and info[k].dtype == torch.float32 and info[k].is_contiguous()
            assert info["blender_mask"].shape == (M,)
            assert np.array_equal(info["match_pixel"].numpy(), np.asarray(md[a][b]).astype(np.float32))
            for k in mono.PER_PAIR:
                t = info[k]
                assert lo <= t.data_ptr() and t.data_ptr() + t.numel() * 4 <= hi
                base = plan.regions["z" if k == "z_val" else k][0]
                assert t.data_ptr() == lo + base + off * 4 * (t.numel() // M), (k, a, b)
            walked.append((a, b, off, M))
            off += M
    assert walked == plan.segments
    # what _arena.walk reads off the dictionary is the plan's own walk
    from scgaussian_amd import _arena
    keys, pairs = _arena.walk(vg)
    assert keys == plan.keys and [p[:4] for p in pairs] == plan.segments
    # the group table: every segment cut into blocks of scg_mono_block() elements, in order
    groups = plan._staged["tab_groups"].view(np.int32).reshape(-1, 2)
    want = [(s, f) for s, seg in enumerate(plan.segments) for f in range(0, seg[3], plan.block)]
    assert [tuple(g) for g in groups] == want and plan.ngroups == len(want) == 8
    segs = plan._staged["tab_segments"].view(np.int32).reshape(-1, 4)
    assert [plan.segments[t][:2] for t in segs[:, 3]] == [(b, a) for a, b, _o, _M in plan.segments]

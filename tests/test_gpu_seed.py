"""The seeding step on the GPU (scgaussian_amd/seed.py, csrc/seed.hip) against the reference's recorded create_from_pcd
(tests/golden/ref_seed.npz) and against the plain-torch restatement (tests/seed_refs.py) run on the device.

Bars.  Bit for bit: n, zval, rayo, rayd, points, features_dc, features_rest, rotation, max_radii2D, sparse_depths, masks, and the
equality of the three scale columns.  opacity: rtol 1e-6.  scaling: at most 2 ulp from log(sqrt(clamp_min(d, 1e-7))) formed by
torch on the device from the project's distCUDA2 on the same points; and exp(2 * scaling[:, 0]) within rtol 2e-5, atol 1e-7 of
the fp64 kNN reference clamped at 1e-7 (the kNN tests' own rtol 1e-5, atol 1e-7, the relative part doubled for the log / sqrt /
exp round trip at |2 * scale| <= 16)."""
import math
import os

import numpy as np
import pytest
import torch

import loss_refs as LR
import seed_refs as S
from scgaussian_amd import _lib, optim as O, render as rmod, seed, synthetic as syn
from scgaussian_amd.init_stage import InitStage
from simple_knn._C import distCUDA2

pytestmark = pytest.mark.gpu
DEV = "cuda"
FX = S.fixture()
BIT_EXACT = ("zval", "rayo", "rayd", "points", "features_dc", "features_rest", "rotation", "max_radii2D", "sparse_depths", "masks")
GROUP = 256                                      # matches per workgroup of csrc/seed.hip


def to_dev(arena):
    return {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in arena.items()}


def inputs_of(arena, views=None):
    return seed.SeedInputs.from_flat(arena["rays_o"], arena["rays_d"], arena["z"], arena["color"], arena["uv"], arena["cam_z"],
                                     arena["counts"], arena["seg_view"], arena["V"], arena["H"], arena["W"], views)


def run(arena):
    return seed.seed_arrays(inputs_of(arena), arena["min_loss"])


def check_scaling(got):
    sc, pts, n = got["scaling"], got["points"], got["n"]
    assert sc.shape == (n, 3)
    assert torch.equal(sc[:, 0], sc[:, 1]) and torch.equal(sc[:, 0], sc[:, 2])
    if n == 0:
        return
    want = torch.log(torch.sqrt(torch.clamp_min(distCUDA2(pts), 0.0000001)))
    ulps = int(S.ulp_distance(sc[:, 0], want).max())
    print(f"scaling: n = {n}, worst distance from torch's log(sqrt(clamp_min(distCUDA2))) {ulps} ulp")
    assert ulps <= 2
    ref = np.maximum(LR.knn_ref64(pts.cpu().numpy()), 1e-7)
    np.testing.assert_allclose(torch.exp(2 * sc[:, 0]).double().cpu().numpy(), ref, rtol=2e-5, atol=1e-7)


def check_against(got, want):
    """got: seed_arrays' dict; want: the restatement's (or the golden arrays), on any device."""
    assert got["n"] == int(want["n"])
    for k in BIT_EXACT:
        w = want[k].to(DEV)
        assert got[k].dtype == w.dtype and got[k].shape == w.shape, (k, got[k].shape, w.shape)
        assert got[k].is_contiguous() and torch.equal(got[k], w), k
    torch.testing.assert_close(got["opacity"], want["opacity"].to(DEV), rtol=1e-6, atol=0)
    check_scaling(got)


def check(arena):
    got = run(arena)
    check_against(got, S.seed(arena, distCUDA2))
    return got


# ---- golden ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", S.SCENES)
def test_golden_scene_equals_the_reference(tag):
    arena = to_dev(S.load_arena(FX, tag))
    want = {k: torch.from_numpy(FX[f"{tag}_out_{k}"]) for k in BIT_EXACT + ("opacity",)}
    want["n"] = int(FX[f"{tag}_n"])
    check_against(run(arena), want)


# ---- compaction edges -------------------------------------------------------------------------------------------------------------
def random_arena(N, counts, seg_view, V, H=12, W=16, seed_=0):
    g = torch.Generator().manual_seed(seed_)
    r = lambda *s: torch.rand(*s, generator=g)                                             # noqa: E731
    assert sum(counts) == N and len(counts) == len(seg_view)
    d = torch.nn.functional.normalize(r(N, 3) - 0.5, dim=1)
    return to_dev(dict(rays_o=r(N, 3) * 2 - 1, rays_d=d, color=r(N, 3), z=r(N) * 6 + 2, cam_z=r(N) * 0.5 + 0.5,
                       uv=torch.stack([r(N) * (W + 4) - 2, r(N) * (H + 4) - 2], 1), min_loss=r(N) * 0.2,
                       counts=list(counts), seg_view=list(seg_view), V=V, H=H, W=W))


def split(N, parts, seed_):
    """N split into `parts` segment sizes (some may be 0), a fixed pseudo-random way."""
    rng = np.random.default_rng(seed_)
    cuts = np.sort(rng.integers(0, N + 1, size=parts - 1))
    return [int(c) for c in np.diff(np.concatenate([[0], cuts, [N]]))]


PATTERNS = ("none", "all", "half", "first_of_run", "last_of_run", "empty_middle")


def pattern(name, N, min_loss):
    i = torch.arange(N, device=DEV)
    if name == "half":
        return min_loss
    keep = {"none": i < 0, "all": i >= 0, "first_of_run": i % GROUP == 0, "last_of_run": (i % GROUP == GROUP - 1) | (i == N - 1),
            "empty_middle": i // GROUP != 1}[name]
    return torch.where(keep, torch.full_like(min_loss, 0.01), torch.full_like(min_loss, 0.5))


@pytest.mark.parametrize("N", [1, 2, 3, 4, 63, 64, 65, 255, 256, 257, 1025, 65537])
def test_compaction_edges_against_the_restatement(N):
    parts = min(N, 6)
    counts = split(N, parts, N)
    arena = random_arena(N, counts, [s % 3 for s in range(parts)], 3, seed_=N)
    base = arena["min_loss"]
    for name in PATTERNS:
        arena["min_loss"] = pattern(name, N, base)
        got = check(arena)
        if name == "none":
            assert got["n"] == 0 and not bool(got["masks"].any())
        if name == "all":
            assert got["n"] == N
        if name == "empty_middle" and N > 2 * GROUP:
            assert got["n"] == N - GROUP
    arena["min_loss"] = None                                                               # the reference's min_loss_state is None
    assert check(arena)["n"] == N


def test_many_short_segments_and_a_segment_across_a_workgroup_boundary():
    counts = [(1, 2, 3, 5, 4)[s % 5] for s in range(42)]
    check(random_arena(sum(counts), counts, [s // 6 for s in range(42)], 7, seed_=42))
    counts = [250, 12, 300]                                                                # [250, 262) lies across element 256
    check(random_arena(sum(counts), counts, [2, 0, 1], 3, seed_=43))
    counts = [254] + [(1, 2, 3, 5, 4)[s % 5] for s in range(42)] + [0, 200]                # short ones around 256, an empty one
    check(random_arena(sum(counts), counts, [s % 7 for s in range(len(counts))], 7, seed_=44))


# ---- sparse depth ---------------------------------------------------------------------------------------------------------------
def test_sparse_depth_duplicates_non_finite_uv_and_an_untouched_view():
    counts, seg_view = [8, 8, 8, 8], [0, 3, 0, 1]                                          # view 2 receives no match at all
    arena = random_arena(32, counts, seg_view, 4, H=12, W=16, seed_=5)
    uv, ml = arena["uv"], arena["min_loss"]
    ml[:] = 0.01
    uv[:, 0] = torch.arange(32, device=DEV) % 16 + 0.5                                     # distinct pixels to start from
    uv[:, 1] = torch.arange(32, device=DEV) // 16 + 0.5
    # within one pair: three kept matches on pixel (row 5, column 7) and a dropped one later in the arena that must not win
    for i in (1, 3, 6, 7):
        uv[i] = torch.tensor([7.25, 5.75], device=DEV)
    ml[7] = 0.5
    # across pairs of view 0: match 2 (pair 0) and match 20 (pair 2) on pixel (row 9, column 2); the later pair wins
    uv[2] = torch.tensor([2.5, 9.5], device=DEV)
    uv[20] = torch.tensor([2.9, 9.1], device=DEV)
    # the same pixel coordinates in another view do not collide
    uv[9] = torch.tensor([2.5, 9.5], device=DEV)
    # non-finite uv: seeded, no depth
    uv[4, 0], uv[5, 1], uv[10, 0] = float("nan"), float("inf"), float("-inf")
    got = check(arena)
    assert got["n"] == 31
    depth = arena["z"] * arena["cam_z"]
    sd = got["sparse_depths"]
    assert float(sd[0, 5, 7]) == float(depth[6]) and float(sd[0, 9, 2]) == float(depth[20]) and float(sd[3, 9, 2]) == float(depth[9])
    assert not bool(got["masks"][2].any()) and not bool(sd[2].any())
    finite = torch.isfinite(uv).all(1) & (ml < 0.1)
    assert int(got["masks"].sum()) == int(finite.sum()) - 2 - 1                            # two lose pixel (5, 7), one pixel (9, 2)
    assert torch.equal(got["zval"][:, 0], arena["z"][ml < 0.1])                            # the non-finite ones are seeded


# ---- kNN hand-over --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3, 4])
def test_knn_hand_over_at_fewer_than_four_points(n):
    check(random_arena(n, [n], [0], 1, seed_=n))
    arena = random_arena(300, [100, 200], [0, 1], 2, seed_=10 + n)                         # n kept out of 300, in two workgroups
    arena["min_loss"][:] = 0.5
    arena["min_loss"][torch.tensor([5, 255, 256, 299][:n], device=DEV)] = 0.0
    assert check(arena)["n"] == n


def test_four_identical_points_take_the_clamped_scale():
    arena = random_arena(4, [4], [0], 1, seed_=3)
    for k in ("rays_o", "rays_d"):
        arena[k][:] = arena[k][0]
    arena["z"][:] = 3.0
    got = check(arena)
    assert bool((got["dist2"] == 0).all())
    want = math.log(math.sqrt(1e-7))                                                       # -8.06: fp32 values there lie 2^-20 apart
    assert float((got["scaling"].double() - want).abs().max()) <= 2 * 2.0 ** -20            # a rounded sqrt, a log good to an ulp


# ---- determinism ----------------------------------------------------------------------------------------------------------------
def test_two_calls_agree_bit_for_bit():
    counts = split(5000, 12, 9)
    arena = random_arena(5000, counts, [s % 3 for s in range(12)], 3, H=12, W=16, seed_=9)          # 576 pixels: many duplicates
    a, b = run(arena), run(arena)
    assert a["n"] == b["n"] > 0
    for k in S.OUT_KEYS + ("dist2",):
        assert torch.equal(a[k], b[k]), k
    check_against(a, S.seed(arena, distCUDA2))


# ---- drop-in --------------------------------------------------------------------------------------------------------------------
class Model:
    """The attribute names of the reference's GaussianModel that the render and optimizer paths read."""
    max_sh_degree = 3
    active_sh_degree = 0


def scene_a_view_gs():
    arena = to_dev(S.load_arena(FX, "A"))
    g = torch.Generator().manual_seed(1)
    extras = {v: dict(intr=torch.from_numpy(FX["A_intr"][v]).to(DEV), w2c=torch.from_numpy(FX["A_w2c"][v]).to(DEV),
                      image_color=torch.rand(arena["H"] * arena["W"], 3, generator=g).to(DEV),
                      near_far=torch.tensor([0.5 + v, 30.0 + v], device=DEV)) for v in range(arena["V"])}
    return arena, S.view_gs_of(arena, extras)


def test_install_makes_create_from_pcd_a_drop_in(capsys):
    arena, vg = scene_a_view_gs()
    gm = Model()
    gm.view_gs = vg
    stage = InitStage.from_view_gs(vg)
    seed.install(gm, stage)
    stage.run_schedule(8, halve_at=(4,))
    stage.load_best(vg)
    stage.min_loss[::2] = 0.01                                       # some matches are kept and some dropped, whatever eight
    stage.min_loss[1::4] = 0.5                                       # iterations reached
    state = stage.min_loss_state()
    inputs = seed.SeedInputs.from_view_gs(vg, stage)
    for name in ("rays_o", "rays_d", "z", "min_loss"):               # the stage's arena tensors are used in place
        assert getattr(inputs, name).data_ptr() == getattr(stage, name).data_ptr(), name
    assert seed._min_loss_flat(inputs, state, stage).data_ptr() == stage.min_loss.data_ptr()
    copies = {a: {b: t.clone() for b, t in d.items()} for a, d in state.items()}
    assert seed._min_loss_flat(inputs, copies, stage).data_ptr() != stage.min_loss.data_ptr()

    gm.create_from_pcd(state)
    n = gm._zval.shape[0]
    assert f"Number of points at initialisation :  {n}" in capsys.readouterr().out
    ref_arena = dict(arena, z=stage.z, min_loss=stage.min_loss)
    want = S.seed(ref_arena, distCUDA2)
    assert n == want["n"] and 0 < n < stage.N
    for attr, k in (("_zval", "zval"), ("_features_dc", "features_dc"), ("_features_rest", "features_rest"), ("_rotation", "rotation"),
                    ("_scaling", None), ("_opacity", None)):
        p = getattr(gm, attr)
        assert isinstance(p, torch.nn.Parameter) and p.requires_grad and p.is_cuda, attr
        if k is not None:
            assert torch.equal(p.detach(), want[k]), attr
    assert gm._zval.shape == (n, 1) and gm._features_dc.shape == (n, 1, 3) and gm._features_rest.shape == (n, 15, 3)
    assert gm._scaling.shape == (n, 3) and gm._rotation.shape == (n, 4) and gm._opacity.shape == (n, 1)
    for attr, k in (("_rayo", "rayo"), ("_rayd", "rayd"), ("max_radii2D", "max_radii2D"), ("sparse_depths", "sparse_depths"),
                    ("masks", "masks")):
        t = getattr(gm, attr)
        assert not isinstance(t, torch.nn.Parameter) and not t.requires_grad and torch.equal(t, want[k]), attr
    for name in ("bg_xyz", "bg_features_dc", "bg_features_rest", "bg_scaling", "bg_rotation", "bg_opacity"):
        p = getattr(gm, name)
        assert isinstance(p, torch.nn.Parameter) and tuple(p.shape) == (0,) and p.is_cuda, name
    names = list(vg)
    H, W = arena["H"], arena["W"]
    assert torch.equal(gm.img_colors, torch.stack([vg[k]["image_color"].reshape(H, W, 3).permute(2, 0, 1) for k in names]))
    assert gm.img_colors.shape == (3, 3, H, W) and gm.img_colors.is_contiguous()
    assert torch.equal(gm.intrs, torch.stack([vg[k]["intr"] for k in names])) and gm.w2cs.shape == (3, 4, 4)
    assert torch.equal(gm.near_fars, torch.stack([vg[k]["near_far"] for k in names]))
    assert gm.curr_scale == 1 and gm.curr_patch_size == 5
    # the copies give the same model (one concatenation instead of the arena)
    other = Model()
    other.view_gs = vg
    seed.create_from_pcd(other, copies, stage=stage)
    assert torch.equal(other._zval, gm._zval) and torch.equal(other.sparse_depths, gm.sparse_depths)

    # the seeded model renders and takes an optimizer step
    opt = O.ArenaAdam([{"params": [getattr(gm, a)], "lr": 1e-3, "name": a.lstrip("_")}
                       for a in ("_zval", "_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation")], lr=0.0, eps=1e-15)
    cam = syn.orbit_camera(W, H, 2.0, 1.0, 7.0).to(DEV)
    pipe = rmod.PipelineParams()
    assert rmod.model_fast_path_available(gm, pipe)
    out = rmod.render(cam, gm, pipe, torch.zeros(3, device=DEV))
    (out["render"].sum() + out["rendered_depth"].sum()).backward()
    before = gm._zval.detach().clone()
    opt.step()
    torch.cuda.synchronize()
    assert opt.fallback_steps == 0
    for k in ("render", "rendered_depth", "rendered_alpha"):
        assert bool(torch.isfinite(out[k]).all()), k
    for a in ("_zval", "_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation"):
        assert bool(torch.isfinite(getattr(gm, a)).all()), a
    assert gm._zval.grad is not None and gm._zval.shape == before.shape


def test_no_match_kept_gives_an_empty_model_without_a_knn_launch():
    arena, vg = scene_a_view_gs()
    gm = Model()
    gm.view_gs = vg
    state = S.nested_state(vg, torch.full_like(arena["min_loss"], 0.5))
    seed.create_from_pcd(gm, state)
    assert gm._zval.shape == (0, 1) and gm._features_rest.shape == (0, 15, 3) and gm._scaling.shape == (0, 3)
    assert gm.max_radii2D.shape == (0,) and gm.sparse_depths.shape == (3, arena["H"], arena["W"])
    assert not bool(gm.sparse_depths.any()) and not bool(gm.masks.any()) and gm._zval.requires_grad
    with pytest.raises(_lib.ScgError, match="contradicts"):
        seed.seed_arrays(inputs_of(arena), arena["min_loss"], n_out=arena["z"].numel())

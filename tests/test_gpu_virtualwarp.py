"""The virtual-view warp loss and the depth smoothness on the GPU (scgaussian_amd/virtual.py, csrc/virtualwarp.hip), forward and
backward, against the fp64 restatement of tests/virtualwarp_refs.py.

Bars.  winner and in_bounds equal fp64's outside the near-tie set; floats lie within max(4 e_ref, 1 fp32 ulp of the tensor's
largest magnitude) of fp64, e_ref being the deviation from fp64 of the reference's own fp32 arithmetic (the reference-shaped
expression in fp32 on the CPU, held to the reference's recorded results by tests/test_virtualwarp_cpu.py) on the same input.
Every comparison prints the kernel's deviation beside e_ref.  A near tie is a quantity within 16 e_ref of a decision's edge
(two views' s_v, a channel term and a clamp bound, a normalised coordinate and +-1, a tap coordinate and an integer); on every
small scene the set is asserted EMPTY before anything is compared (the seeds were chosen on the CPU from the reference's fp32 run
alone, with four times the margin: another CPU's fp32 run has another e_ref), on the 96 x 128 scene and the three one-view scenes
of 255 to 272 tiles it may hold 1 % of the pixels.

What fp64 is.  The kernels' input is the composed record of 12 fp32 numbers per view, so the truth they are held to is the fp64
restatement of the header's rule ON THOSE RECORDS; e_ref is the reference-shaped expression's fp32 run against its own fp64 run
on the raw matrices.  (Rounding the records moves a loss by up to 2e-7 on its own, measured on the CPU: the reference's chain of
four fp32 matrix products has the same size of error, but per pixel and with both signs.)  Coordinates PLANTED on edges
(test_planted_coordinates...) are dyadic, so both sides compute the same bits up to the division by Z + 1e-8; the decisions are
asserted against hand-made expectations as well."""
import numpy as np
import pytest
import torch

import parity_utils as pu
import virtualwarp_refs as VR
from scgaussian_amd import _lib_vw, virtual
from scgaussian_amd import render as rmod
from scgaussian_amd import synthetic as syn

pytestmark = pytest.mark.gpu
DEV = "cuda"
T = _lib_vw.VW_TILE
NVMAX = _lib_vw.VW_MAX_VIEWS
# (H, W, nv): seed.  The lowest seed whose fp32 reference run has no near tie at FOUR times the margin (64 e_ref; three times for
# 16 x 33), sees 30 % of the frame, agrees with fp64 on every winner and (nv <= 3) lets every view win somewhere.
SEEDS = {(3, 3, 3): 2, (3, 40, 3): 2, (40, 3, 3): 1, (4, 5, 3): 1, (T - 1, T + 1, 3): 6, (T, T, 3): 51, (T + 1, T - 1, 3): 28,
         (2 * T + 1, T, 3): 1, (T, 2 * T + 1, 3): 425, (T - 1, 2 * T + 1, 2): 5, (2 * T + 1, T + 1, 1): 3, (7, 9, 1): 1, (7, 9, 2): 2,
         (6, 7, NVMAX): 76, (12, 20, 3): 29}
SPECIAL_SEED = 1             # of the special-depths scene, chosen the same way with the depths planted
_REFS = {}


def refs_of(key, scene, upstream=1.0, eps=1e-8):
    """(truth, r64, r32, near ties) of a scene, computed once.  r64, r32: the reference-shaped expression in fp64 and fp32, whose
    difference is e_ref.  truth: the fp64 restatement of the header's rule on the kernels' own input, the composed fp32 records."""
    if key not in _REFS:
        r64, r32 = VR.warp_reference(scene, upstream=upstream), VR.warp_reference(scene, torch.float32, upstream=upstream)
        truth = VR.warp_reference(scene, upstream=upstream, eps=eps,
                                  records=virtual.compose_records(scene["intrs"], scene["w2cs"], scene["vir_c2w"]))
        _REFS[key] = (truth, r64, r32, VR.near_ties(r64, r32, truth))
    return _REFS[key]


def run_kernels(scene, upstream=1.0, warp=None, mask=None):
    """mask: the bytes handed to the kernels in place of the scene's bool mask (uint8, any values)."""
    t = VR.tensors(scene, device=DEV)
    if mask is not None:
        t["vir_mask"] = torch.from_numpy(np.ascontiguousarray(mask)).to(DEV)
    if warp is None:
        warp = virtual.VirtualWarp(t["intrs"], t["w2cs"], t["img_colors"])
        warp.set_pose(scene["vir_c2w"])
    img, depth = t["virtual_img"].requires_grad_(True), t["virtual_depth"].requires_grad_(True)
    loss = warp.loss(img, depth, t["vir_mask"])
    (loss * upstream).backward()
    torch.cuda.synchronize()
    return {"loss": loss.detach().cpu().numpy(), "loss_map": warp.loss_map.cpu().numpy(), "winner": warp.winner.cpu().numpy(),
            "in_bounds": warp.in_bounds.cpu().numpy().astype(bool), "d_img": img.grad.cpu().numpy(), "d_depth": depth.grad.cpu().numpy()}


def check(name, scene, upstream=1.0, max_share=0.0, planted=False):
    """Forward and backward of the kernels against fp64 under the bars.  planted: the scene's coordinates lie ON edges or within
    the division's 1e-8 of them; its set is not asserted empty, and the decisions must equal fp64's everywhere all the same (the
    kernels form the coordinates in fp64, operation by operation as the restatement does)."""
    truth, r64, r32, ties = refs_of(name, scene, upstream)
    print(name, "near-tie share", ties["share"], "e_ref of s / raw / norm / tap", ties["e"])
    if not planted:
        assert ties["share"] <= max_share, (name, ties["share"])
    got = run_kernels(scene, upstream)
    decide = np.ones_like(ties["decision"]) if planted else ~ties["decision"]
    assert np.array_equal(got["winner"][decide], truth["winner"][decide]), name
    assert np.array_equal(got["in_bounds"][:, decide], truth["in_bounds"][:, decide]), name
    keep = np.ones_like(ties["block"]) if planted else ~ties["block"]
    for k, where in (("loss", None), ("loss_map", decide), ("d_img", keep), ("d_depth", keep & ~ties["tap"])):
        if k == "loss" and ties["share"] > 0 and not planted:
            continue
        dev, e_ref, bound = VR.compare(k, got[k], r64, r32, keep if planted and k == "d_depth" else where, truth)
        print(f"  {name} {k}: kernel deviation {dev:.3e}  e_ref {e_ref:.3e}  bound {bound:.3e}")
        assert dev <= bound, (name, k, dev, e_ref, bound)
    return got, truth


# ---- shapes ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,nv", [k for k in SEEDS if k != (12, 20, 3)])
def test_shapes_forward_and_backward(H, W, nv):
    """3x3, 3x40, 40x3, 4x5; heights and widths one under, at, one over and twice-plus-one the tile side, both ways; 1, 2, 3 and the
    most views."""
    got, r64 = check(f"{H}x{W}x{nv}", VR.make_scene(H, W, nv, SEEDS[(H, W, nv)]), upstream=0.75 if nv == 2 else 1.0)
    assert (got["winner"] == -1).any() and (got["winner"] >= 0).any()


@pytest.mark.parametrize("tag", [str(t) for t in np.load(VR.GOLDEN)["scenes"]])
def test_fixture_scenes(tag):
    fx = np.load(VR.GOLDEN)
    check("fixture " + tag, {k: fx[f"{tag}_{k}"] for k in VR.KEYS})


def test_larger_scene_near_tie_share():
    sc = VR.make_scene(96, 128, 3, 8)
    check("96x128x3", sc, max_share=0.01)


# ---- planted cases --------------------------------------------------------------------------------------------------------------
def test_unseen_pixels_and_masked_pixels():
    sc = VR.make_scene(12, 20, 3, SEEDS[(12, 20, 3)])
    got, r64 = check("unseen", sc)
    unseen = ~r64["in_bounds"].any(axis=0)
    assert unseen.any() and (~sc["vir_mask"] & ~unseen).any()                 # a pixel no view sees; a visible one the mask removes
    assert (got["winner"][unseen] == -1).all() and (got["loss_map"][unseen] == 0).all()
    assert (got["winner"][~sc["vir_mask"]] == -1).all() and (got["loss_map"][~sc["vir_mask"]] == 0).all()


def test_a_frame_no_view_sees_is_exactly_zero():
    sc = VR.make_scene(T + 1, T + 3, 3, 5)
    sc["w2cs"][:, 0, 3] += 100.0
    got = run_kernels(sc)
    assert not got["in_bounds"].any() and (got["winner"] == -1).all()
    assert float(got["loss"]) == 0.0 and not got["loss_map"].any() and not got["d_img"].any() and not got["d_depth"].any()
    sc = VR.make_scene(T + 1, T + 3, 3, 5)
    sc["vir_mask"][:] = False                                                 # ... and one the mask removes
    got = run_kernels(sc)
    assert got["in_bounds"].any() and (got["winner"] == -1).all()
    assert float(got["loss"]) == 0.0 and not got["d_img"].any() and not got["d_depth"].any()


def identical_views_scene():
    sc = VR.make_scene(T - 1, T + 1, 3, SEEDS[(T - 1, T + 1, 3)])
    for k in ("intrs", "w2cs", "img_colors"):
        sc[k] = sc[k][[0, 0, 2]].copy()                                        # views 0 and 1 bit-identical
    return sc


def test_two_bit_identical_views_the_lowest_index_wins():
    sc = identical_views_scene()
    got, r64 = check("identical views", sc)
    assert (got["winner"] != 1).all() and (got["winner"] == 0).any()
    assert np.array_equal(got["in_bounds"][0], got["in_bounds"][1])
    two = {k: (v[[0, 2]].copy() if k in ("intrs", "w2cs", "img_colors") else v) for k, v in sc.items()}
    alone = run_kernels(two)                                                   # view 0 carries the whole y-side gradient: as if 1 were absent
    assert np.array_equal(alone["d_img"], got["d_img"]) and np.array_equal(alone["d_depth"], got["d_depth"])
    assert np.array_equal(alone["winner"] * 2, np.where(got["winner"] > 0, got["winner"] * 2 - 2, got["winner"] * 2))


def behind_camera_scene():
    sc = VR.make_scene(T + 1, T - 1, 3, SEEDS[(T + 1, T - 1, 3)])
    flip = np.diag([-1.0, -1.0, -1.0]).astype(np.float32)                      # view 0's camera frame negated: Z < 0, x and y unchanged
    sc["w2cs"][0, :3, :3] = flip @ sc["w2cs"][0, :3, :3]
    sc["w2cs"][0, :3, 3] = flip @ sc["w2cs"][0, :3, 3]
    return sc


def test_a_point_behind_a_camera_that_lands_in_bounds():
    sc = behind_camera_scene()
    rec = virtual.compose_records(sc["intrs"], sc["w2cs"], sc["vir_c2w"]).astype(np.float64)
    yy, xx = np.mgrid[0:T + 1, 0:T - 1]
    Z = sc["virtual_depth"] * (rec[0, 6] * xx + rec[0, 7] * yy + rec[0, 8]) + rec[0, 11]
    got, r64 = check("behind the camera", sc)
    assert (Z < 0).all() and got["in_bounds"][0].mean() > 0.5 and (got["winner"] == 0).any()


def special_depths_scene():
    sc = VR.make_scene(T + 1, T + 3, 3, SPECIAL_SEED)
    d = sc["virtual_depth"]
    d[2, 3], d[5, 9], d[8, 4], d[11, 12], d[14, 15] = 0.0, -3.0, np.nan, np.inf, -np.inf
    return sc


def test_depth_zero_negative_nan_and_inf():
    """A NaN or infinite depth is out of bounds in every view, samples zero, and its depth gradient is NaN, as torch's chain gives
    it (0 / NaN); its neighbours are finite.  (The projection 2^33 px away is the fourth view of the planted coordinates.)"""
    sc = special_depths_scene()
    got, r64 = check("special depths", sc)
    bad = ~np.isfinite(sc["virtual_depth"])
    assert bad.sum() == 3 and np.isnan(got["d_depth"][bad]).all() and np.isfinite(got["d_depth"][~bad]).all()
    assert not got["in_bounds"][:, bad].any() and np.isfinite(got["d_img"]).all() and np.isfinite(got["loss"])


def test_planted_coordinates_on_0_on_the_last_column_on_minus_a_half_and_on_integers():
    H, W = 6, 9
    sc = VR.exact_scene(H, W, nv=4, depth=2.0)
    for v, shift in enumerate((0.0, -0.5, 2.0)):                               # pixel px lands on px + shift exactly
        sc["w2cs"][v, 0, 3] = np.float32(shift * 2.0 / 4.0)
    sc["w2cs"][3, :3, 3] = (32768.0, 0.0, -2.0 + 2.0 ** -20)                   # Z = 2^-20 exactly: x ~ 1.4e11 > 2^33, its floor beyond int32
    got, r64 = check("planted coordinates", sc, planted=True)
    assert r64["tap"][3, 0].min() > 2.0 ** 33 and not got["in_bounds"][3].any()
    px = np.arange(W)[None, :].repeat(H, axis=0)
    assert got["in_bounds"][0].all()                                           # 0 and W - 1 themselves are inside
    assert np.array_equal(got["in_bounds"][1], px >= 1)                        # -0.5 is outside, 0.5 inside
    assert np.array_equal(got["in_bounds"][2], px <= W - 3)                    # W - 1 inside, W outside
    tap = r64["tap"][0]
    assert np.abs(r64["d_depth"]).max() > 0 and (np.abs(tap - np.round(tap)) < 1e-7).any()      # taps 1e-8 short of an integer: one side, both


def test_points_in_the_camera_plane_are_divided_by_1e_minus_8():
    """x = X / (Z + 1e-8): at depths around 3 the 1e-8 is below fp32's resolution of every output, so it shows only where Z = 0
    EXACTLY.  View 1 of a dyadic pair is moved back by the depth: Z = 0 at every pixel, X = 2 (px - cx), Y = 2 (py - cy).  By the
    rule the centre pixel is 0 / 1e-8 = 0, in bounds on the corner (nx = ny = -1, tap -0.5), every other pixel 2e8 px and more
    away, out of bounds and outside every image, and the depth gradient is finite everywhere.  (Without the 1e-8: 0 / 0 and
    x / 0, the centre out of bounds and dy/ddepth not finite at every pixel.)"""
    H, W = 6, 9
    sc = VR.exact_scene(H, W, nv=2, depth=2.0)
    sc["w2cs"][1, 2, 3] = -2.0
    rec = virtual.compose_records(sc["intrs"], sc["w2cs"], sc["vir_c2w"])
    assert np.array_equal(rec[1], np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, -2 * (W // 2), -2 * (H // 2), -2], dtype=np.float32))
    got, truth = check("camera plane", sc, planted=True)
    centre = np.zeros((H, W), dtype=bool)
    centre[H // 2, W // 2] = True
    assert np.array_equal(got["in_bounds"][1], centre) and got["in_bounds"][0].all()
    assert np.abs(truth["tap"][1][:, ~centre]).max(axis=0).min() > 2e8 and np.array_equal(truth["tap"][1][:, centre].ravel(), [-0.5, -0.5])
    assert np.isfinite(got["d_depth"]).all() and np.isfinite(got["d_img"]).all() and np.isfinite(got["loss"])


def test_identical_virtual_image_and_warped_image_sit_on_the_clamp():
    """The warp of the identity pose is not the photograph (normalised with W - 1, sampled with W), so the warped image is taken
    from where the forward leaves it: the head of the scratch, (nv,3,H,W) fp64 (the header's layout), rounded to fp32.  With it as
    virtual_img every term is within 1e-7 of 0, the clamp's lower bound, on either side of it: the fp64 restatement of the same
    input decides each clamp, and the kernels must follow it (planted: nothing is excluded).
    Exactly ON the bound: black photographs and a black virtual image.  mx = my = 0, n = d = C1 C2 bit for bit, every term is
    (1 - 1) / 2 = 0, where torch's clamp lets the gradient through; B = 1 / C2 and C = -1 / C2 multiply zeros: both gradients
    are zeros, and the depth's 0 * dy/dd is 0."""
    H, W = T + 1, T - 1
    sc = VR.make_scene(H, W, 1, 3)
    sc["vir_mask"][:] = True
    t = VR.tensors(sc, device=DEV)
    warp = virtual.VirtualWarp(t["intrs"], t["w2cs"], t["img_colors"])
    warp.set_pose(sc["vir_c2w"])
    warp.loss(t["virtual_img"], t["virtual_depth"], t["vir_mask"])
    y = warp.scratch.view(torch.float64)[:3 * H * W].reshape(3, H, W).cpu().numpy()
    sc["virtual_img"] = y.astype(np.float32)
    assert np.abs(y).max() > 0.1
    got, truth = check("image = its own warp", sc, planted=True)
    seen = got["in_bounds"][0]
    assert seen.mean() > 0.5 and np.array_equal(got["winner"], np.where(seen, 0, -1)) and float(got["loss"]) < 1e-6
    assert ((truth["raw"] < 0) & seen).any() and ((truth["raw"] > 0) & seen).any()      # both sides of the bound
    sc["virtual_img"][:] = 0
    sc["img_colors"][:] = 0
    got = run_kernels(sc)
    assert np.array_equal(got["winner"], np.where(seen, 0, -1))
    assert float(got["loss"]) == 0.0 and not got["loss_map"].any()
    assert not got["d_img"].any() and not got["d_depth"].any()


# ---- rules of the header no scene above reaches ------------------------------------------------------------------------------------
def test_mask_bytes_other_than_one_are_true():
    """vir_mask: "non-zero = true".  The same scene with its true pixels written as 1, 2, 0x80 and 0xFF: every output bit for bit
    the bool mask's."""
    sc = VR.make_scene(12, 20, 3, SEEDS[(12, 20, 3)])
    values = np.array([1, 2, 0x80, 0xFF], dtype=np.uint8)
    draw = values[np.random.default_rng(3).integers(0, 4, sc["vir_mask"].shape)]
    mask = np.where(sc["vir_mask"], draw, 0).astype(np.uint8)
    assert all((mask == b).any() for b in values) and (mask == 0).any() and np.array_equal(mask != 0, sc["vir_mask"])
    want, got = run_kernels(sc), run_kernels(sc, mask=mask)
    assert (want["winner"] >= 0).any() and (want["winner"][~sc["vir_mask"]] == -1).all()
    for k in want:
        assert np.array_equal(got[k], want[k]), k


@pytest.mark.parametrize("variant", ["inside", "masked_out"])
@pytest.mark.parametrize("case", list(VR.NONFINITE_CASES))
def test_nonfinite_image_values(case, variant):
    """One element of virtual_img set to NaN, +inf or -inf, or one texel of img_colors[1] to NaN or +inf, with every affected
    window inside the mask and with all of them masked out.

    Forward, against the restatement (whose winner is torch.min's: the first NaN view): the windows that hold the value have a
    NaN s_v (an infinity gives inf - inf in the variance), loss_map's NaN pattern is exact, the winner there is the first view
    with a NaN, the loss is NaN inside the mask and finite and within the bar masked out.

    Gradients, against the header's gather rule in fp64 (virtualwarp_refs.gather_gradients: window_gradients per view on the
    windows that view won, the y side times the sampler's own fp64 derivative), NOT against autograd.  Where they differ (printed):
    autograd of the expression sends the clamp's zero through n / dd, 0 / NaN, and marks the whole 9 x 9 block of pixels whose
    windows hold the value — 81 elements of d_img's channel and of d_depth for the image cases, 90 for the texel (it lies under
    two pixels' taps) — masked out or not.  The header's rule (its paragraph on non-finite values) marks only the element itself:
    d_img and d_depth at the one pixel (the two pixels under the texel) inside the mask; masked out d_img is all finite, d_depth
    all finite for the image cases and NaN at the two pixels whose dy/ddepth holds the texel (0 * NaN over every view).  The
    finite values are held under the suite's bar everywhere, the 9 x 9 block included; e_ref is autograd's own fp32 deviation
    where autograd is finite."""
    H, W, nv, seed = VR.NONFINITE_SCENE
    assert SEEDS[(H, W, nv)] == seed and (H, W) == (T + 1, T - 1)
    clean = VR.make_scene(H, W, nv, seed)
    rec = virtual.compose_records(clean["intrs"], clean["w2cs"], clean["vir_c2w"])
    sc, affected = VR.nonfinite_scene(case, variant, rec)
    with np.errstate(invalid="ignore"):
        r64, r32 = VR.warp_reference(sc), VR.warp_reference(sc, torch.float32)
        truth = VR.warp_reference(sc, records=rec, sampler=True)
        ties = VR.near_ties(r64, r32, truth)
        truth["d_img"], truth["d_depth"] = VR.gather_gradients(sc["virtual_img"], truth)
    assert ties["share"] == 0 and affected.sum() >= 25
    got = run_kernels(sc)
    name = f"{case} {variant}"
    assert np.array_equal(got["winner"], truth["winner"]) and np.array_equal(got["in_bounds"], truth["in_bounds"]), name
    first = np.where((np.isnan(truth["s"]) & truth["in_bounds"]), np.arange(nv).reshape(nv, 1, 1), nv).min(axis=0)
    if variant == "inside":
        assert np.isnan(got["loss"]) and np.array_equal(np.isnan(got["loss_map"]), affected), name
        assert np.array_equal(got["winner"][affected], first[affected]), name
    else:
        assert np.isfinite(got["loss"]) and np.isfinite(got["loss_map"]).all() and (got["winner"][affected] == -1).all(), name
    for k in ("loss", "loss_map", "d_img", "d_depth"):
        dev, e_ref, bound = VR.compare(k, got[k], r64, r32, None, truth)      # asserts the NaN pattern against truth's, everywhere
        ok = np.isfinite(truth[k])
        dev = max(dev, float(np.abs(got[k][ok] - truth[k][ok]).max()) if ok.any() else 0.0)      # ... and where autograd is NaN
        print(f"  {name} {k}: kernel deviation {dev:.3e}  e_ref {e_ref:.3e}  bound {bound:.3e}")
        assert dev <= bound, (name, k, dev, e_ref, bound)
    for k in ("d_img", "d_depth"):
        print(f"  {name} {k}: NaN in the kernel's at {np.argwhere(np.isnan(got[k])).tolist()}; autograd's has {int(np.isnan(r64[k]).sum())}"
              f" in rows {np.unique(np.argwhere(np.isnan(r64[k]))[:, -2]).tolist()}")
        assert (np.isnan(r64[k]) | ~np.isnan(got[k])).all()                   # the rule's NaNs are among autograd's
    key, at, _ = VR.NONFINITE_CASES[case]
    under = np.argwhere(~np.isfinite(truth["warp"]).all(axis=(0, 1))).tolist() if key == "img_colors" else [list(at[1:])]
    want_img = [[at[-3]] + q for q in under] if variant == "inside" else []
    want_depth = under if variant == "inside" or key == "img_colors" else []
    assert np.argwhere(np.isnan(got["d_img"])).tolist() == want_img and np.argwhere(np.isnan(got["d_depth"])).tolist() == want_depth


def loss_is_the_mean_of_its_map(name, got):
    """The header's identity, loss = sum of loss_map / (H W), on what the kernels returned: |loss - mean64(loss_map)| <=
    2^-25 max(loss_map) + ulp32(loss) / 2, mean64 the fp64 mean of the fp32 map; the first term for the rounding of the map's
    elements (the kernel sums them before they are rounded), the second for the rounding of the scalar."""
    m, loss = got["loss_map"].astype(np.float64), float(got["loss"])
    dev, bound = abs(loss - m.mean()), 2.0 ** -25 * m.max() + VR.ulp32(loss) / 2
    print(f"  {name} loss against the fp64 mean of its map: deviation {dev:.3e}  bound {bound:.3e}")
    assert m.max() > 0 and dev <= bound, (name, dev, bound)


def test_loss_is_the_mean_of_its_map_on_a_small_scene():
    """12 x 20 is two tiles: a failure of the identity HERE is not the fold's second trip."""
    loss_is_the_mean_of_its_map("12x20x3", run_kernels(VR.make_scene(12, 20, 3, SEEDS[(12, 20, 3)])))


@pytest.mark.parametrize("H,W", list(VR.LARGE_SCENES))
def test_more_tiles_than_the_fold_has_threads(H, W):
    """255, 256 and 272 tiles (the last with a partial tile row) of one view: above 256 a thread of vw_fold_kernel adds a second
    partial sum.  Everything against fp64 as on the 96 x 128 scene (near-tie share at most 1 %: check() then leaves the scalar out),
    and the scalar by the identity above."""
    tiles = -(-H // T) * -(-W // T)
    assert tiles == {(240, 272): 255, (256, 256): 256, (241, 272): 272}[(H, W)] and T * T == 256
    got, truth = check(f"{H}x{W}x1", VR.make_scene(H, W, 1, VR.LARGE_SCENES[(H, W)]), max_share=0.01)
    assert (got["winner"] == 0).mean() > 0.5
    loss_is_the_mean_of_its_map(f"{H}x{W}x1", got)


# ---- determinism, graphs, host reads --------------------------------------------------------------------------------------------
def test_two_runs_are_bitwise_equal():
    sc = VR.make_scene(2 * T + 1, 2 * T + 3, 3, 4)
    a, b = run_kernels(sc), run_kernels(sc)
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=a[k].dtype.kind == "f"), k
    d = torch.from_numpy(sc["virtual_depth"]).to(DEV)
    g = torch.from_numpy(sc["virtual_img"]).to(DEV)
    outs = []
    for _ in range(2):
        dd = d.clone().requires_grad_(True)
        loss = virtual.smooth_loss(dd, g)
        loss.backward()
        outs.append((loss.detach().cpu().numpy(), dd.grad.cpu().numpy()))
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])


def test_forward_and_backward_in_a_graph_replayed_on_rewritten_inputs_and_pose():
    H, W, nv = T + 1, 2 * T + 1, 3
    a, b = VR.make_scene(H, W, nv, 1), VR.make_scene(H, W, nv, 2)
    b["intrs"], b["w2cs"], b["img_colors"] = a["intrs"], a["w2cs"], a["img_colors"]      # the photographs stay; image, depth, mask, pose change
    t = VR.tensors(a, device=DEV)
    warp = virtual.VirtualWarp(t["intrs"], t["w2cs"], t["img_colors"])
    warp.set_pose(a["vir_c2w"])
    img, depth, mask = t["virtual_img"].clone().requires_grad_(True), t["virtual_depth"].clone().requires_grad_(True), t["vir_mask"].clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                              # warm up on the capture's stream
        gi, gd = torch.autograd.grad(warp.loss(img, depth, mask) + virtual.smooth_loss(depth, img.detach()), (img, depth))
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss = warp.loss(img, depth, mask) + virtual.smooth_loss(depth, img.detach())
        gi, gd = torch.autograd.grad(loss, (img, depth))
    tb = VR.tensors(b, device=DEV)
    with torch.no_grad():
        img.copy_(tb["virtual_img"]); depth.copy_(tb["virtual_depth"]); mask.copy_(tb["vir_mask"])
    warp.set_pose(b["vir_c2w"])
    graph.replay()
    torch.cuda.synchronize()
    replayed = [x.clone() for x in (loss, gi, gd, warp.winner, warp.loss_map)]
    img2, depth2 = tb["virtual_img"].clone().requires_grad_(True), tb["virtual_depth"].clone().requires_grad_(True)
    eager = warp.loss(img2, depth2, tb["vir_mask"]) + virtual.smooth_loss(depth2, img2.detach())
    ei, ed = torch.autograd.grad(eager, (img2, depth2))
    for x, y in zip(replayed, (eager, ei, ed, warp.winner, warp.loss_map)):
        assert torch.equal(x, y)
    assert not torch.equal(replayed[3].cpu(), torch.from_numpy(run_kernels(a)["winner"]))


def test_no_host_read(monkeypatch):
    sc = VR.make_scene(T, T + 1, 2, 3)
    t = VR.tensors(sc, device=DEV)
    warp = virtual.VirtualWarp(t["intrs"], t["w2cs"], t["img_colors"])         # reads the 2 x 25 matrix floats once, here
    warp.set_pose(sc["vir_c2w"])
    img, depth = t["virtual_img"].requires_grad_(True), t["virtual_depth"].requires_grad_(True)
    (warp.loss(img, depth, t["vir_mask"]) + virtual.smooth_loss(depth, img.detach())).backward()      # warm
    torch.cuda.synchronize()
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
    warp.set_pose(sc["vir_c2w"] * np.float32(1.001))
    loss = warp.loss(img, depth, t["vir_mask"]) + virtual.smooth_loss(depth, img.detach())
    loss.backward()
    monkeypatch.undo()
    assert reads == [], reads
    torch.cuda.synchronize()
    assert torch.isfinite(loss).item()


def test_backward_after_another_forward_is_refused():
    sc = VR.make_scene(7, 9, 1, 1)
    t = VR.tensors(sc, device=DEV)
    warp = virtual.VirtualWarp(t["intrs"], t["w2cs"], t["img_colors"])
    warp.set_pose(sc["vir_c2w"])
    img = t["virtual_img"].requires_grad_(True)
    first = warp.loss(img, t["virtual_depth"], t["vir_mask"])
    warp.loss(img, t["virtual_depth"], t["vir_mask"])
    with pytest.raises(Exception, match="another forward"):
        first.backward()


def test_reference_signature_on_device_tensors():
    fx = np.load(VR.GOLDEN)
    sc = {k: fx[f"a_{k}"] for k in VR.KEYS}
    t = VR.tensors(sc, device=DEV)
    H, W = sc["virtual_depth"].shape
    depth = t["virtual_depth"].reshape(1, H, W).requires_grad_(True)
    loss = virtual.virtual_warp_loss(t["virtual_img"], depth, sc["vir_c2w"], t["intrs"], t["w2cs"], t["img_colors"], t["vir_mask"].reshape(1, H, W))
    loss.backward()
    again = run_kernels(sc)
    assert depth.grad.shape == (1, H, W) and np.array_equal(depth.grad[0].cpu().numpy(), again["d_depth"])
    assert np.array_equal(loss.detach().cpu().numpy(), again["loss"])


# ---- the smoothness loss --------------------------------------------------------------------------------------------------------
B = _lib_vw.VW_SMOOTH_PIXELS
SMOOTH_SHAPES = [(1, 1), (1, 7), (7, 1), (2, 2), (1, B - 1), (1, B), (1, B + 1), (B + 1, 1), (3, (2 * B + 1) // 3 + 1), (T - 1, T + 1), (37, 29)]


def _smooth(depth, guide, upstream=1.0):
    d = torch.from_numpy(depth).to(DEV).requires_grad_(True)
    g = None if guide is None else torch.from_numpy(guide).to(DEV)
    loss = virtual.smooth_loss(d, g)
    if torch.isnan(loss.detach()).item():
        grad = torch.autograd.grad(loss, d, torch.tensor(upstream, device=DEV))[0]
    else:
        (loss * upstream).backward()
        grad = d.grad
    return loss.detach().cpu().numpy(), grad.cpu().numpy()


def check_smooth(name, depth, guide, upstream=0.5):
    """Loss and gradient of the kernels against fp64 under max(4 e_ref, 1 ulp); the empty means' NaN and the gradient's pattern."""
    H, W = depth.shape
    loss, grad = _smooth(depth, guide, upstream=upstream)
    l64, g64 = VR.smooth_reference(depth, guide, upstream=upstream)
    l32, g32 = VR.smooth_reference(depth, guide, torch.float32, upstream=upstream)
    if H == 1 or W == 1:
        assert np.isnan(loss) and np.isnan(l64)                                # an empty mean, as torch's
        if H == 1 and W == 1:
            assert not grad.any()
    else:
        e = abs(float(l32) - float(l64))
        print(f"smooth {name}: loss deviation {abs(float(loss) - float(l64)):.3e} e_ref {e:.3e} bound {VR.bar(e, l64):.3e}")
        assert abs(float(loss) - float(l64)) <= VR.bar(e, l64)
    fin = np.isfinite(g64)
    assert np.array_equal(np.isfinite(grad), fin)
    if fin.any():
        e = np.abs(g32[fin] - g64[fin]).max()
        dev = np.abs(grad[fin] - g64[fin]).max()
        print(f"smooth {name}: gradient deviation {dev:.3e} e_ref {e:.3e} bound {VR.bar(e, g64[fin]):.3e}")
        assert dev <= VR.bar(e, g64[fin])


@pytest.mark.parametrize("H,W", SMOOTH_SHAPES)
@pytest.mark.parametrize("form", ["none", "hw", "chw", "1hw"])
def test_smooth_loss_shapes_and_guides(H, W, form):
    rng = np.random.default_rng(H * 1000 + W)
    depth = (3 + rng.uniform(-1, 1, (H, W))).astype(np.float32)
    guide = {"none": None, "hw": rng.uniform(0, 1, (H, W)), "chw": rng.uniform(0, 1, (3, H, W)), "1hw": rng.uniform(0, 1, (1, H, W))}[form]
    check_smooth(f"{H}x{W} {form}", depth, None if guide is None else guide.astype(np.float32))


# 255, 256, 257 and 514 workgroups of B pixels: 65 280, 65 536, 65 538 and 131 330 pixels.  (As 2 x 32640 ... 2 x 65665 the widths
# would pass SCG_VW_MAX_DIM = 16384 and the library would refuse them — test_virtualwarp_cpu.py asserts that — so the same pixel
# counts are laid out 4, 4, 6 and 10 rows high; the second is as wide as the library takes.)
SMOOTH_MANY_GROUPS = {(4, 16320): 255, (4, 16384): 256, (6, 10923): 257, (10, 13133): 514}


@pytest.mark.parametrize("H,W", list(SMOOTH_MANY_GROUPS))
@pytest.mark.parametrize("form", ["none", "chw"])
def test_smooth_loss_more_workgroups_than_the_fold_has_threads(H, W, form):
    """Above 256 workgroups a thread of vw_smooth_fold_kernel adds a second pair of partial sums."""
    assert -(-H * W // B) == SMOOTH_MANY_GROUPS[(H, W)] and B == 256
    rng = np.random.default_rng(H * 1000 + W)
    depth = (3 + rng.uniform(-1, 1, (H, W))).astype(np.float32)
    check_smooth(f"{H}x{W} {form}", depth, None if form == "none" else rng.uniform(0, 1, (3, H, W)).astype(np.float32))


@pytest.mark.parametrize("C", [2, 4, 5, 64])
def test_smooth_loss_guide_channels(C):
    """The guide's mean is the sum over C in channel order and ONE division by C, C up to 64."""
    H, W = T - 1, T + 1
    rng = np.random.default_rng(C)
    depth = (3 + rng.uniform(-1, 1, (H, W))).astype(np.float32)
    check_smooth(f"{H}x{W} C={C}", depth, rng.uniform(0, 1, (C, H, W)).astype(np.float32))


def test_smooth_loss_refuses_65_guide_channels_before_any_launch():
    H, W, C = T - 1, T + 1, _lib_vw.VW_MAX_GUIDE_CHANNELS + 1
    depth, guide = torch.full((H, W), 3.0, device=DEV), torch.zeros((C, H, W), device=DEV)
    with pytest.raises(Exception, match="65 channels"):
        virtual.smooth_loss(depth, guide)
    lib = _lib_vw.load()
    out = torch.full((2, H, W), 7.0, device=DEV)                                # loss in out[0, 0, 0], d_depth in out[1]
    scratch = torch.full((4,), 7.0, device=DEV)
    up = torch.ones(1, device=DEV)
    assert lib.scg_vw_smooth_forward(H, W, C, depth.data_ptr(), guide.data_ptr(), out.data_ptr(), scratch.data_ptr(), 16, None) == -2
    assert b"C = 65" in lib.scg_vw_last_error()
    assert lib.scg_vw_smooth_backward(H, W, C, depth.data_ptr(), guide.data_ptr(), up.data_ptr(), out[1].data_ptr(), None) == -2
    torch.cuda.synchronize()
    assert (out == 7.0).all().item() and (scratch == 7.0).all().item()         # SCG_E_RANGE, and nothing was launched


@pytest.mark.parametrize("kind", ["spread", "deep"])
def test_smooth_loss_exp_far_from_zero(kind):
    """"exp is the accurate expf": every other guide lies in [0, 1], so the exponent never leaves [-1, 0].  spread: one channel
    drawn from [0, 20], neighbours' differences all over [0, 20], the exponent over [-20, 0].  deep: multiples of 1/64 (fp32
    forms their differences exactly, so e_ref is the fp32 exp's own error) alternating between [0, 2] and [18, 20] in a
    chequerboard, every exponent in [-20, -16]: there the weights are all of one size, and an exp whose relative error grows
    with |x| is measured against weights it is wrong about, not against the weights near 1 that set the bar of `spread`."""
    H, W = 37, 29
    rng = np.random.default_rng(20)
    depth = (3 + rng.uniform(-1, 1, (H, W))).astype(np.float32)
    if kind == "spread":
        guide = rng.uniform(0, 20, (H, W)).astype(np.float32)
    else:
        yy, xx = np.mgrid[0:H, 0:W]
        guide = (rng.integers(0, 129, (H, W)) / 64.0 + 18.0 * ((yy + xx) % 2)).astype(np.float32)
    gx, gy = np.abs(np.diff(guide.astype(np.float64), axis=1)), np.abs(np.diff(guide.astype(np.float64), axis=0))
    lo, hi = min(gx.min(), gy.min()), max(gx.max(), gy.max())
    assert (lo < 0.1 and hi > 19 and np.histogram(gx, 4, (0, 20))[0].min() > 20) if kind == "spread" else (lo >= 16 and hi <= 20)
    check_smooth(f"{H}x{W} exp {kind}", depth, guide)


def test_smooth_loss_equal_neighbours_have_sign_zero():
    depth = np.full((T, T + 1), 2.5, dtype=np.float32)
    depth[3, 4] = 3.0
    depth[9, :] = np.nan                                                       # sign(NaN) = 0 too: torch's abs backward
    d = torch.from_numpy(depth).to(DEV).requires_grad_(True)
    loss = virtual.smooth_loss(d)
    grad = torch.autograd.grad(loss, d)[0].cpu().numpy()
    nx, ny = T * T, (T - 1) * (T + 1)
    want = np.zeros_like(depth)
    want[3, 4] = 2 / nx + 2 / ny
    want[3, 3] = want[3, 5] = -1 / nx
    want[2, 4] = want[4, 4] = -1 / ny
    assert np.isnan(loss.item()) and np.allclose(grad, want, rtol=1e-6, atol=0) and (grad[want == 0] == 0).all()


def test_smooth_loss_fixture():
    fx = np.load(VR.GOLDEN)
    for tag in fx["scenes"]:
        for form, guide in (("g0", None), ("g2", fx[f"{tag}_guide"][0]), ("g3", fx[f"{tag}_guide"])):
            loss, grad = _smooth(fx[f"{tag}_virtual_depth"], guide)
            l64, g64 = VR.smooth_reference(fx[f"{tag}_virtual_depth"], guide)
            want_l, want_g = fx[f"{tag}_smooth_{form}"], fx[f"{tag}_smooth_d_depth_{form}"]
            assert abs(float(loss) - float(l64)) <= VR.bar(abs(float(want_l) - float(l64)), l64), (tag, form)
            assert np.abs(grad - g64).max() <= VR.bar(np.abs(want_g - g64).max(), g64), (tag, form)


# ---- the twin; end to end -------------------------------------------------------------------------------------------------------
def test_cpu_tensors_take_the_twin():
    sc = VR.make_scene(7, 9, 2, SEEDS[(7, 9, 2)])
    t = VR.tensors(sc)
    warp = virtual.VirtualWarp(t["intrs"], t["w2cs"], t["img_colors"])
    warp.set_pose(sc["vir_c2w"])
    img = t["virtual_img"].requires_grad_(True)
    loss = warp.loss(img, t["virtual_depth"], t["vir_mask"])
    loss.backward()
    got = run_kernels(sc)
    assert not loss.is_cuda and np.array_equal(warp.winner.numpy(), got["winner"])
    assert abs(float(loss) - float(got["loss"])) < 1e-6 and np.abs(img.grad.numpy() - got["d_img"]).max() < 1e-6


def test_end_to_end_through_render_against_the_torch_restatement_on_the_device():
    """A synthetic model, three training views' renders as photographs, a virtual camera between them: render, both losses,
    backward.  The model's parameter gradients against the same step with the plain-torch restatement (in fp64) on the device in
    place of the kernels, under the suite's gradient bar."""
    P, W, H = 4_000, 128, 96
    sc = syn.make_scene(P, W, H, seed=12)
    model = syn.make_raw_model(sc, ray_fraction=0.6, seed=15)
    cams = [syn.orbit_camera(W, H, yaw, 1.0, 7.0).to(DEV) for yaw in (-4.0, 0.0, 5.0)]
    bg, pipe = torch.zeros(3, device=DEV), rmod.PipelineParams()
    md = model.to(DEV)
    with torch.no_grad():
        colors = torch.stack([rmod.render(c, md, pipe, bg)["render"].clamp(0, 1) for c in cams])
    fx, fy = W / (2 * np.tan(cams[0].FoVx / 2)), H / (2 * np.tan(cams[0].FoVy / 2))
    intrs = torch.tensor([[fx, 0, W / 2], [0, fy, H / 2], [0, 0, 1]], dtype=torch.float32, device=DEV).expand(3, 3, 3).contiguous()
    w2cs = torch.stack([c.world_view_transform.T for c in cams]).contiguous()
    between = syn.orbit_camera(W, H, 2.0, 1.0, 7.0)
    c2w = np.linalg.inv(between.world_view_transform.T.numpy().astype(np.float64))[:3]
    vcam = virtual.virtual_camera(c2w, like=cams[0])
    warp = virtual.VirtualWarp(intrs, w2cs, colors)
    warp.set_pose(c2w)
    mask = torch.ones(H * W, dtype=torch.bool, device=DEV)

    def step(kernels):
        m = model.to(DEV)
        m.requires_grad_()
        out = rmod.render(vcam, m, pipe, bg)
        img, depth = out["render"], out["rendered_depth"]
        if kernels:
            loss = warp.loss(img, depth, mask) + 0.1 * virtual.smooth_loss(depth.reshape(H, W), img)
        else:                                                                  # in fp64, as the restatement everywhere in this file
            img, depth = img.double(), depth.double()
            loss = virtual.warp_loss_torch(img, depth, mask, colors, warp.records)[0] + \
                0.1 * virtual.smooth_loss_torch(depth.reshape(H, W), img)
        loss.backward()
        torch.cuda.synchronize()
        return loss.detach(), m
    l_k, m_k = step(True)
    l_t, m_t = step(False)
    assert (warp.winner >= 0).float().mean().item() > 0.5
    print("end to end: loss", float(l_k), float(l_t))
    assert abs(float(l_k) - float(l_t)) <= 1e-5 * abs(float(l_t))
    n = 0
    for k, (pk, pt) in enumerate(zip(m_k.parameters(), m_t.parameters())):
        if pt.grad is not None and pt.grad.numel() and float(pt.grad.abs().max()) > 0:
            pu.assert_close(pk.grad, pt.grad, ("virtual warp end to end", k))
            n += 1
    assert n >= 5

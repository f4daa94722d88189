"""The cross-view depth consistency kernels (csrc/geocheck.hip) on the GPU, through scgaussian_amd.geo_check.GeoCheck.

Two references (tests/geocheck_refs.py).  The fp64 oracle walks the reference's chain step by step; the kernel multiplies matrices
composed once per pair, so the two agree to rounding and a pixel ON a threshold may vote differently: the scene tests leave the
oracle's near-tie pixels out (at most 1 % of a scene, held by tests/test_geocheck_hip_cpu.py) and demand equal votes everywhere else
and depths within 1 fp32 ulp.  The restatement repeats the kernel's arithmetic operation by operation: planted pixels, odd shapes and
thresholds are held to it exactly.  Every scene has at most 8 views of at most 70 x 70 pixels."""
import numpy as np
import pytest
import torch

import geocheck_refs as G
from scgaussian_amd import _lib
from scgaussian_amd import geo_check as gc

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
ULP32 = 2.0 ** -23


def _run(intrs, exts, depths, num_src=15, **kw):
    """(votes, masks, filtered, pairs) as numpy, from one GeoCheck."""
    n, H, W = depths.shape
    chk = gc.GeoCheck(n, H, W, num_src=num_src, device=DEV)
    chk.setup(torch.from_numpy(np.asarray(intrs)).to(DEV), torch.from_numpy(np.asarray(exts)).to(DEV))
    fd, fm = chk.run(torch.from_numpy(np.asarray(depths, dtype=np.float32)).to(DEV), **kw)
    torch.cuda.synchronize()
    assert fd.shape == fm.shape == chk.votes.shape == (n, H, W)
    assert fd.dtype == fm.dtype == torch.float32 and chk.votes.dtype == torch.uint8 and chk.pairs.dtype == torch.int32
    return chk.votes.cpu().numpy(), fm.cpu().numpy(), fd.cpu().numpy(), chk.pairs.cpu().numpy()


def _hold(what, got, want_votes, want_depth, near, view_thresh):
    """The terms of every comparison: votes equal outside `near`, masks follow from the votes, depths within 1 fp32 ulp where the
    masks agree (0 or NaN where the pixel is dropped).  Prints the measured maximum and the pixels left out."""
    votes, masks, filtered, _ = got
    off = votes != want_votes
    assert not (off & ~near).any(), f"{what}: {int((off & ~near).sum())} votes differ outside the near-tie set"
    assert np.array_equal(masks, (votes > view_thresh).astype(np.float32))
    agree = masks == (want_votes > view_thresh)
    kept = agree & (masks > 0)
    worst = float(G.ulps32(filtered[kept], np.asarray(want_depth)[kept]).max()) if kept.any() else 0.0
    print(f"{what}: {votes.size} pixels, {int(near.sum())} left out as near ties, {int(off.sum())} votes differ among them, "
          f"{int(kept.sum())} kept depths, max {worst:.3f} fp32 ulp")
    assert worst <= 1.0
    dropped = filtered[masks == 0]
    assert np.all((dropped == 0) | np.isnan(dropped))
    return worst


# ---- the reference's own run ------------------------------------------------------------------------------------------------------
def test_reference_fixture():
    r = G.scene_refs("fixture")
    ref = np.load(G.GOLDEN)
    votes, masks, filtered, _ = _run(r["intrs"], r["exts"], r["depths"], **r["kw"])
    near = r["near"]
    assert near.mean() <= 0.01
    off = masks != ref["geo_masks"]
    assert not (off & ~near).any()
    # the yardstick: what the fp64 oracle itself deviates from the fixture (the reference sums in fp32)
    same_o = (r["o_mask"] == ref["geo_masks"]) & (ref["geo_masks"] > 0)
    want = ref["geo_filtered_depths"].astype(np.float64)
    e_oracle = float((np.abs(r["o_depth"][same_o] - want[same_o]) / np.abs(want[same_o])).max())
    same = ~off & (masks > 0)
    err = float((np.abs(filtered[same].astype(np.float64) - want[same]) / np.abs(want[same])).max())
    print(f"fixture: {int(off.sum())} masks differ (all near ties), depth deviation {err:.3e}, oracle's own {e_oracle:.3e}")
    assert err <= max(4 * e_oracle, ULP32)
    assert np.all(filtered[~off & (masks == 0)] == 0)


@pytest.mark.parametrize("name", ["arc", "small", "wide"])
def test_against_the_oracle(name):
    r = G.scene_refs(name)
    got = _run(r["intrs"], r["exts"], r["depths"], **r["kw"])
    _hold(name, got, r["o_votes"], r["o_depth"], r["near"], r["kw"]["view_thresh"])
    assert np.array_equal(got[3], r["r_pairs"])
    if name == "wide":                                   # more sources asked for than views: every view is one of its own
        assert all(i in got[3][i] for i in range(got[3].shape[0]))
    else:
        assert all(i not in got[3][i] for i in range(got[3].shape[0]))


def test_agrees_with_the_twin_on_the_device():
    r = G.scene_refs("small")
    ti, te, td = (torch.from_numpy(r[k]).to(DEV) for k in ("intrs", "exts", "depths"))
    td_, tm = gc.geocheck(ti, te, td, **r["kw"])
    hd, hm = gc.geocheck_hip(ti, te, td, **r["kw"])
    torch.cuda.synchronize()
    assert hd.shape == td_.shape and hm.shape == tm.shape and hd.dtype == hm.dtype == torch.float32
    assert (tm != hm).float().mean().item() < 0.005
    same = (tm == hm).cpu().numpy()
    assert np.allclose(hd.cpu().numpy()[same], td_.cpu().numpy()[same], rtol=1e-4, atol=0, equal_nan=True)


# ---- pairs -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which,num_src", [("tie", 1), ("tie", 2), ("tie", 3), ("tie", 64), ("beyond", 2), ("beyond", 3), ("beyond", 4),
                                          ("beyond", 15)])
def test_pairs_are_the_twins_get_pairs(which, num_src):
    exts = G.planted_cameras(which)
    n = len(exts)
    K = np.repeat(np.array([[32.0, 0, 2], [0, 32.0, 2], [0, 0, 1]])[None], n, 0)
    chk = gc.GeoCheck(n, 4, 4, num_src=num_src, device=DEV).setup(torch.from_numpy(K).to(DEV), torch.from_numpy(exts).float().to(DEV))
    want = gc.get_pairs(torch.from_numpy(exts), num_src)
    assert chk.pairs.shape == want.shape and torch.equal(chk.pairs.cpu().long(), want)
    assert np.array_equal(chk.pairs.cpu().numpy(), G.pair_table(exts, num_src))


# ---- shapes around the workgroup's pixel tile ------------------------------------------------------------------------------------
TW, TH = _lib.load().scg_geocheck_tile(0), _lib.load().scg_geocheck_tile(1)


def _close_scene(n, H, W, seed):
    """Cameras a tenth of a pixel of disparity apart in front of a slanted plane, every view with its own outliers and holes:
    round trips mostly agree even in an image of one row or column."""
    rng = np.random.default_rng(seed)
    f = 30.0
    K = np.array([[f, 0, W / 2], [0, f, H / 2], [0, 0, 1.0]])
    exts = np.zeros((n, 4, 4))
    depths = np.zeros((n, H, W), dtype=np.float32)
    nrm, d0 = np.array([0.1, -0.05, 1.0]), 6.0
    for i in range(n):
        ang = 0.002 * (i - n / 2)
        R = np.array([[np.cos(ang), 0, np.sin(ang)], [0, 1, 0], [-np.sin(ang), 0, np.cos(ang)]])
        t = np.array([0.02 * i + 0.003 * i * i, 0.007 * i, 0.0])
        exts[i] = np.eye(4)
        exts[i, :3, :3], exts[i, :3, 3] = R, t
        ys, xs = np.mgrid[0:H, 0:W]
        rays = np.linalg.inv(K) @ np.stack([xs.ravel(), ys.ravel(), np.ones(H * W)])
        depths[i] = ((d0 + nrm @ (R.T @ t)) / (nrm @ (R.T @ rays))).reshape(H, W)
    bad = rng.random(depths.shape) < 0.1
    depths[bad] *= rng.uniform(1.05, 1.6, size=int(bad.sum())).astype(np.float32)
    depths[rng.random(depths.shape) < 0.03] = 0.0
    return np.repeat(K[None], n, 0), exts, depths


@pytest.mark.parametrize("n,H,W", [(3, 1, 1), (3, 1, TW + 1), (3, TH + 1, 1), (3, TH - 1, TW - 1), (3, TH, TW), (3, TH + 1, TW + 1),
                                   (2, 2 * TH + 1, 2 * TW + 3), (3, 2, 3), (2, 2, 3)])
def test_shapes_around_the_tile(n, H, W):
    intrs, exts, depths = _close_scene(n, H, W, seed=100 + 7 * H + W)
    kw = dict(view_thresh=0, num_src=2)
    r_votes, r_masks, r_filtered, r_pairs = G.geocheck_ref(intrs, exts, depths, **kw)
    near = G.near_ties(intrs, exts, depths, num_src=kw["num_src"])
    got = _run(intrs, exts, depths, **kw)
    _hold(f"{n} x {H} x {W}", got, r_votes, r_filtered, near, kw["view_thresh"])
    assert np.array_equal(got[3], r_pairs)
    if H * W >= 64:
        assert r_votes.max() >= 1 and len(np.unique(depths.reshape(n, -1), axis=0)) == n          # views of unequal content


# ---- planted pixels --------------------------------------------------------------------------------------------------------------
PW = PH = 16


def _planted():
    """Four cameras with identity rotations and dyadic numbers, so that every matrix, product and coordinate below is exact: view 0
    looks at the plane Z = 8; views 1 and 2 stand 0.25 to its right and left (a pixel of depth d lands 8 / d pixels beside itself);
    view 3 stands 4 in front of it (k2 = d - 4) and sees the pixel (u, v) at (2 (u - 8) + 8, 2 (v - 8) + 8).  Their depth maps show
    the same plane, so an untouched pixel in the middle of view 0 collects all three votes.  Returns (intrs, exts, depths, the planted pixels of view 0 as {name: (v, u)})."""
    K = np.array([[32.0, 0, 8], [0, 32.0, 8], [0, 0, 1]])
    exts = np.repeat(np.eye(4)[None], 4, 0)
    exts[1, 0, 3], exts[2, 0, 3], exts[3, 2, 3] = 0.25, -0.25, -4.0
    depths = np.full((4, PH, PW), 8.0, dtype=np.float32)
    depths[3] = 4.0
    d0 = depths[0]
    at = {"zero": (1, 5), "negative": (1, 7), "nan": (1, 9), "inf": (1, 11),
          "on_integer": (5, 6),                       # d = 8, untouched: lands on u + 1 and u - 1 exactly, and inside view 3
          "between": (4, 6),                          # d = 16: lands on u + 0.5 and u - 0.5
          "in_minus1_0": (5, 0),                      # d = 16 at u = 0: view 2 sees it at -0.5
          "in_w1_w": (6, PW - 1),                     # d = 16 at u = W - 1: view 1 sees it at W - 0.5
          "at_minus1": (7, 0),                        # d = 8 at u = 0: view 2 sees it at -1
          "at_w": (8, PW - 1),                        # d = 8 at u = W - 1: view 1 sees it at W
          "k2_zero": (9, 6),                          # d = 4: on view 3's camera plane
          "behind": (10, 6),                          # d = 2: behind view 3
          "beyond_int32": (11, 6),                    # d = 2^-30: lands 2^33 pixels away
          "source_zero": (12, 4), "source_nan": (14, 4)}          # view 1 holds 0 / NaN where these land (u + 1)
    for name, val in (("zero", 0.0), ("negative", -8.0), ("nan", np.nan), ("inf", np.inf), ("between", 16.0), ("in_minus1_0", 16.0),
                      ("in_w1_w", 16.0), ("k2_zero", 4.0), ("behind", 2.0), ("beyond_int32", 2.0 ** -30)):
        d0[at[name]] = val
    depths[1, 12, 5], depths[1, 14, 5] = 0.0, np.nan
    return np.repeat(K[None], 4, 0), exts, depths, at


def test_planted_pixels():
    intrs, exts, depths, at = _planted()
    kw = dict(view_thresh=1, num_src=3)
    r_votes, r_masks, r_filtered, r_pairs = G.geocheck_ref(intrs, exts, depths, **kw)
    votes, masks, filtered, pairs = _run(intrs, exts, depths, **kw)
    assert np.array_equal(pairs, r_pairs) and pairs[0].tolist() == [1, 2, 3]
    assert np.array_equal(votes, r_votes), np.argwhere(votes != r_votes)[:8]
    assert np.array_equal(masks, r_masks)
    assert np.array_equal(filtered, r_filtered, equal_nan=True), float(np.nanmax(G.ulps32(filtered, r_filtered)))
    # ... and the restatement says what the rule says at each of them
    v0 = {k: int(r_votes[0][p]) for k, p in at.items()}
    assert v0["zero"] == v0["negative"] == v0["nan"] == v0["inf"] == v0["beyond_int32"] == v0["between"] == 0
    assert np.isnan(r_filtered[0][at["nan"]]) and r_masks[0][at["nan"]] == 0
    assert v0["on_integer"] == 3 and r_filtered[0][at["on_integer"]] == 8.0 and r_masks[0][at["on_integer"]] == 1.0
    assert int(r_votes[0, 2, 6]) == 2                                                 # view 3 sees rows and columns 4 ... 11 only
    assert v0["at_minus1"] == 1 and v0["at_w"] == 1                                   # view 2 / view 1 see nothing there, nor does view 3
    assert v0["k2_zero"] == 0 and v0["behind"] == 0
    assert int(r_votes[0, 12, 3]) == 2 and v0["source_zero"] == 1                     # a zero beside a landing point costs its neighbour nothing
    assert int(r_votes[0, 14, 3]) == 1 and v0["source_nan"] == 1                      # a NaN does: NaN * 0 through the zero weight


@pytest.mark.parametrize("view_thresh", [0, 1, 2, 3, -1])
def test_vote_thresholds(view_thresh):
    intrs, exts, depths, _ = _planted()
    r_votes, r_masks, r_filtered, _ = G.geocheck_ref(intrs, exts, depths, view_thresh=view_thresh, num_src=3)
    votes, masks, filtered, _ = _run(intrs, exts, depths, view_thresh=view_thresh, num_src=3)
    assert np.array_equal(votes, r_votes) and np.array_equal(masks, r_masks) and np.array_equal(filtered, r_filtered, equal_nan=True)
    assert np.array_equal(masks, (votes > view_thresh).astype(np.float32))
    if 0 <= view_thresh < 3:                               # pixels exactly on the threshold are dropped, one vote more is kept
        assert (votes == view_thresh).any() and (votes == view_thresh + 1).any()
        assert not masks[votes == view_thresh].any() and masks[votes == view_thresh + 1].all()
    if view_thresh == 3:                                   # view_thresh = J: nothing can be kept
        assert votes.max() == 3 and not masks.any()
    if view_thresh == -1:
        assert masks.all()


# ---- the remaining cases ---------------------------------------------------------------------------------------------------------
def test_singular_intrinsic_gives_no_votes_and_no_fault():
    r = G.scene_refs("small")
    intrs = r["intrs"].copy()
    intrs[2] = np.array([[0.0, 0, 16], [0, 0.0, 12], [0, 0, 1]])          # focal length 0: no inverse
    r_votes, r_masks, r_filtered, _ = G.geocheck_ref(intrs, r["exts"], r["depths"], **r["kw"])
    got = _run(intrs, r["exts"], r["depths"], **r["kw"])
    # pairs without view 2 are those of the scene itself; the others vote in neither: the scene's near ties cover this one's
    _hold("singular K_2", got, r_votes, r_filtered, r["near"], r["kw"]["view_thresh"])
    assert not got[0][2].any() and not got[1][2].any()
    assert got[1].any() and (got[0] < r["o_votes"]).any()                 # ... and view 2 votes for nobody else either


def test_two_runs_are_bit_identical():
    r = G.scene_refs("arc")
    a = _run(r["intrs"], r["exts"], r["depths"], **r["kw"])
    b = _run(r["intrs"], r["exts"], r["depths"], **r["kw"])
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()


def test_run_is_captured_and_replayed_on_new_depths():
    """The capture itself proves that GeoCheck.run reads nothing on the host."""
    r = G.scene_refs("small")
    _, _, other = _close_scene(*r["depths"].shape, seed=5)
    n, H, W = r["depths"].shape
    kw = dict(view_thresh=r["kw"]["view_thresh"])
    chk = gc.GeoCheck(n, H, W, num_src=r["kw"]["num_src"], device=DEV)
    chk.setup(torch.from_numpy(r["intrs"]).to(DEV), torch.from_numpy(r["exts"]).to(DEV))
    static = torch.from_numpy(other).to(DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        chk.run(static, **kw)                                  # warm: library loaded
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fd, fm = chk.run(static, **kw)
    static.copy_(torch.from_numpy(r["depths"]).to(DEV))        # new depths, written in place
    graph.replay()
    torch.cuda.synchronize()
    eager = _run(r["intrs"], r["exts"], r["depths"], **r["kw"])
    assert np.array_equal(chk.votes.cpu().numpy(), eager[0]) and np.array_equal(fm.cpu().numpy(), eager[1])
    assert fd.cpu().numpy().tobytes() == eager[2].tobytes()
    assert eager[1].any() and not np.array_equal(other, r["depths"])

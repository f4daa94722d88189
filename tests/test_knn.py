"""distCUDA2 replacement: oracle self-consistency on CPU, HIP kernel vs oracle on GPU."""
import numpy as np
import pytest
import torch

import loss_refs as lr
from oracle import knn_oracle as ko


def _cloud(n, seed, dup=False):
    rng = np.random.default_rng(seed)
    p = rng.normal(size=(n, 3)).astype(np.float32) * np.array([3.0, 1.0, 0.3], dtype=np.float32)
    if dup and n > 10:
        p[n // 2: n // 2 + n // 10] = p[: n // 10]        # exact duplicates -> zero distances
    return p


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 64, 1000, 5000])
def test_oracle_bruteforce_matches_kdtree(n):
    p = _cloud(n, n, dup=n >= 1000)
    a = ko.mean_dist2_bruteforce(p)
    b = ko.mean_dist2_kdtree(p)
    np.testing.assert_allclose(a, b, rtol=2e-4, atol=1e-6)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 255, 256, 257, 1025, 12000, 60000])
def test_distcuda2_matches_oracle(n):
    from simple_knn._C import distCUDA2
    p = _cloud(n, 7 * n + 1, dup=n >= 1000)
    out = distCUDA2(torch.from_numpy(p).cuda()).cpu().numpy()
    ref = ko.mean_dist2_bruteforce(p)
    assert out.shape == (n,) and out.dtype == np.float32
    np.testing.assert_allclose(out, ref, rtol=1e-5, atol=1e-7)
    if n >= 1000:      # duplicated points have a zero-distance neighbour: their mean is at most 2/3 of an undup'd one
        dup = np.r_[np.arange(n // 10), np.arange(n // 2, n // 2 + n // 10)]
        assert np.median(out[dup]) < np.median(np.delete(out, dup))
    # the reference's use of it: scales = log(sqrt(clamp_min(dist2, 1e-7)))  (scene/gaussian_model.py:444-445)
    scales = torch.log(torch.sqrt(torch.clamp_min(torch.from_numpy(out), 1e-7)))
    assert torch.isfinite(scales).all()


@pytest.mark.gpu
def test_distcuda2_refuses_cpu_tensors():
    from simple_knn._C import distCUDA2
    from scgaussian_amd._lib import ScgError
    with pytest.raises(ScgError):
        distCUDA2(torch.zeros(10, 3))


# --------------------------------------------------------------------------------------------------------------------------------
# fp64 edge parity.  Reference: loss_refs.knn_ref64 (scipy kd-tree, fp64) on the fp32 points the kernel gets; bar rtol 1e-5 /
# atol 1e-7 as above, except the cloud offset by 1e3, whose bar is 4 * e32 of the fp32 brute force against fp64.
#
# The kernel splits the candidate range over splits = min(64, ceil(524288 / n)) slices of per = ceil(n / splits) candidates, each
# streamed through LDS in tiles of 1 024:
#   n          splits  per     what it exercises
#   4, 5       64      1       60 / 59 empty slices; 3 / 4 neighbours exist
#   1023..1025 64      16..17  uneven slices, the last ones empty or short
#   8191       64      128     last slice one short
#   8192       64      128     the last n where the cap of 64 binds exactly
#   8193       64      129     uneven, last slice short
#   8322       64      131     the last n with 64 slices
#   8323       63      133     the first n with 63
#   16385      32      513
#   23529      23      1023    one less than the LDS tile
#   23552      23      1024    exactly one tile per slice
#   23553      23      1025    one candidate in a second tile
#   65537      8       8193    eight tiles + 1
#   262145     2       131073
#   524288     1       524288  a single slice (kd-tree reference only; the GPU needs well under a second)
KNN_SIZES = [4, 5, 1023, 1024, 1025, 8191, 8192, 8193, 8322, 8323, 16385, 23529, 23552, 23553, 65537, 262145]
KNN_BIG = 524288
BRUTE_MAX = 20000                      # no fp32 brute force on the CPU above this
# cloud kind -> largest n it runs at (identical points make a kd-tree one quadratic leaf; the offset cloud needs the brute force)
KNN_CLOUDS = {"lattice": 262145, "identical": 8323, "collinear": 262145, "clusters": 262145, "offset1e3": 16385, "aniso": 262145}
KNN_CASES = [(kind, n) for kind, nmax in KNN_CLOUDS.items() for n in KNN_SIZES if n <= nmax] + [("aniso", KNN_BIG)]


def _expected_split(n):
    splits = min(64, -(-524288 // n))
    return splits, -(-n // splits)


def test_knn_case_table_hits_the_split_and_tile_boundaries():
    """The sizes above sit on the boundaries the table claims (pure arithmetic: the kernel's own formula restated)."""
    assert [_expected_split(n) for n in (8192, 8322, 8323, 262145, 524288)] == [(64, 128), (64, 131), (63, 133), (2, 131073), (1, 524288)]
    assert [_expected_split(n)[1] for n in (23529, 23552, 23553)] == [1023, 1024, 1025]
    assert _expected_split(524287)[0] == 2


def _dist(points):
    from simple_knn._C import distCUDA2
    out = distCUDA2(points)
    assert out.dtype == torch.float32 and out.shape == (points.shape[0],)
    return out.cpu().numpy()


def _hold(tag, out, p, kind):
    assert np.isfinite(out).all()
    if kind == "identical":                                   # exactly 0 (a kd-tree of identical points is one quadratic leaf: no call)
        assert not out.any()
        return
    ref = lr.knn_ref64(p)
    err = np.abs(out.astype(np.float64) - ref)
    if kind == "offset1e3":                                   # fp32 cancellation in q - c: the plain fp32 evaluation sets the bar
        e32 = float(np.abs(ko.mean_dist2_bruteforce(p).astype(np.float64) - ref).max())
        lr.held_to(f"knn {tag}", float(err.max()), e32, 1e-7, out.size)
        return
    bound = 1e-5 * np.abs(ref) + 1e-7
    print(f"CENSUS knn {tag}: worst |out - ref64| / (1e-5 |ref| + 1e-7) = {float((err / bound).max()):.3f}")
    np.testing.assert_allclose(out, ref, rtol=1e-5, atol=1e-7)


@pytest.mark.gpu
@pytest.mark.parametrize("kind,n", KNN_CASES)
def test_distcuda2_adversarial_clouds_against_fp64(kind, n):
    p = lr.CLOUDS[kind](n, 13 * n + 5)
    out = _dist(torch.from_numpy(p).cuda())
    _hold(f"{kind} n={n}", out, p, kind)
    if kind == "lattice" and n >= 1023:                       # massive exact ties: three neighbours at exactly one spacing
        assert np.median(out) == np.float32(0.25)


@pytest.mark.gpu
@pytest.mark.parametrize("kind,n", [("lattice", 8323), ("aniso", 8323), ("aniso", 23553), ("clusters", 1025)])
def test_distcuda2_is_invariant_under_a_permutation_of_the_rows(kind, n):
    """Each distance is the same fp32 expression of the same two points wherever they sit in the slices, and the three smallest are
    added in sorted order: the output of a permuted cloud, un-permuted, is EXACTLY the original's."""
    p = lr.CLOUDS[kind](n, 3 * n + 1)
    perm = np.random.default_rng(n).permutation(n)
    a = _dist(torch.from_numpy(p).cuda())
    b = _dist(torch.from_numpy(p[perm]).cuda())
    back = np.empty_like(b)
    back[perm] = b
    assert np.array_equal(back, a)


@pytest.mark.gpu
@pytest.mark.parametrize("kind,n", [("aniso", 4097), ("collinear", 1025), ("lattice", 4162)])
def test_distcuda2_of_a_cloud_stacked_on_itself(kind, n):
    """Every point gains a zero-distance neighbour (its copy), and so does its nearest neighbour: the three nearest of the stacked
    cloud are the copy, the original's nearest point and THAT point's copy.  The expected value is (0 + d1^2 + d1^2) / 3 with d1 the
    nearest distance in the ORIGINAL cloud, identical for a point and its copy.
    (2 n = 8 194 / 8 324 rows: just past the 64- and 63-slice boundaries.)"""
    p = lr.CLOUDS[kind](n, 5 * n + 2)
    out = _dist(torch.from_numpy(np.concatenate([p, p])).cuda())
    assert np.array_equal(out[:n], out[n:])
    d = ((p.astype(np.float64)[:, None, :] - p.astype(np.float64)[None, :, :]) ** 2).sum(-1)
    np.fill_diagonal(d, np.inf)
    d1sq = d.min(axis=1)
    want = (0.0 + d1sq + d1sq) / 3.0
    np.testing.assert_allclose(lr.knn_ref64(np.concatenate([p, p]))[:n], want, rtol=1e-12, atol=1e-15)     # the reference agrees
    np.testing.assert_allclose(out[:n], want, rtol=1e-5, atol=1e-7)


@pytest.mark.gpu
def test_distcuda2_non_contiguous_and_fp64_input():
    n = 8193
    p = lr.aniso_cloud(n, 99)
    four = torch.from_numpy(np.concatenate([p, np.full((n, 1), 7.0, np.float32)], 1)).cuda()
    view = four[:, :3]
    assert not view.is_contiguous()
    want = _dist(torch.from_numpy(p).cuda())
    assert np.array_equal(_dist(view), want)
    assert np.array_equal(_dist(torch.from_numpy(p).double().cuda()), want)          # fp64 holding fp32 values: the same numbers
    _hold("non-contiguous", want, p, "aniso")

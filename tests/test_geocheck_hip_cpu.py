"""CPU-side checks of the cross-view depth consistency kernels (csrc/geocheck.hip, include/scg_geocheck.h): the ABI, the argument
validation, and the references the GPU tests lean on.  No kernel runs here.

What anchors what: geocheck_refs.geocheck_ref restates the kernel's rule; it is held here to oracle/geo_check_oracle.py on every
scene the GPU tests use (votes equal, kept depths within 1 fp32 ulp), and its pair table to the twin's and the oracle's get_pairs."""
import numpy as np
import pytest
import torch

import abi_text
import geocheck_refs as G
from oracle import geo_check_oracle as orc
from scgaussian_amd import _lib
from scgaussian_amd import geo_check as gc

NEW_SYMBOLS = ("scg_geocheck_workspace_bytes", "scg_geocheck_tile", "scg_geocheck_setup", "scg_geocheck")
NULL, RANGE, SCRATCH, ALIGN = -1, -2, -4, -5


def test_new_symbols_are_declared_exported_and_bound():
    lib = _lib.load()
    declared = abi_text.declared_by("scg_geocheck.h")
    assert declared == sorted(NEW_SYMBOLS)
    for name in declared:
        assert name in _lib.SYMBOLS, f"ctypes binding lacks {name}"
        assert hasattr(lib, name), f"libscg_raster.so does not export {name}"
    assert lib.scg_abi_version() == _lib.ABI_VERSION == 10
    tw, th = lib.scg_geocheck_tile(0), lib.scg_geocheck_tile(1)
    assert tw >= 4 and th >= 2 and tw * th % 64 == 0 and lib.scg_geocheck_tile(2) == 0
    # the source is built without contraction: numpy's float64 products and sums
    from scgaussian_amd import build
    assert "-ffp-contract=off" in build.SOURCES["geocheck.hip"]
    assert any(h.endswith("scg_geocheck.h") for h in build.HEADERS)
    assert all(hasattr(gc, n) for n in ("GeoCheck", "geocheck_hip", "geocheck", "reproject_with_depth", "get_pairs"))


def test_workspace_bytes_is_monotone():
    lib = _lib.load()
    ws = lib.scg_geocheck_workspace_bytes
    assert ws(1, 1) >= 4 + 9 * 8 + 24 * 8
    sizes = [ws(n, 15) for n in (1, 2, 3, 8, 15, 16, 49, 300, 1024)]
    assert sizes == sorted(sizes) and sizes[0] < sizes[-1]
    sizes = [ws(49, j) for j in (1, 2, 5, 15, 48, 49, 64)]
    assert sizes == sorted(sizes) and sizes[0] < sizes[4] < sizes[5] == sizes[6]          # J = min(num_src, N)
    assert ws(49, 15) >= 49 * 15 * (4 + 24 * 8 + 4) + 49 * 9 * 8
    for n, j in ((0, 15), (1025, 15), (8, 0), (8, 65), (-1, 15), (8, -1)):
        assert ws(n, j) == 0


def test_argument_validation_returns_codes_without_a_gpu():
    lib = _lib.load()
    fake = 0x10000            # never dereferenced: validation fails first
    big = 1 << 30

    def setup(intrs=fake, exts=fake, N=8, num_src=15, ws=fake, nbytes=big):
        return lib.scg_geocheck_setup(intrs, exts, N, num_src, ws, nbytes, None)

    def run(depths=fake, N=8, H=20, W=28, num_src=15, ws=fake, nbytes=big, votes=fake, masks=fake, filtered=fake):
        return lib.scg_geocheck(depths, N, H, W, num_src, 1.0, 0.01, 5, ws, nbytes, votes, masks, filtered, None)

    for call in (setup, run):
        for k in ("intrs", "exts", "ws") if call is setup else ("depths", "ws", "votes", "masks", "filtered"):
            assert call(**{k: None}) == NULL, k
        for N in (0, 1025, -3):
            assert call(N=N) == RANGE
        for num_src in (0, 65, -1):
            assert call(num_src=num_src) == RANGE
        assert b"out of range" in lib.scg_last_error()
        need = lib.scg_geocheck_workspace_bytes(8, 15)
        assert call(nbytes=need - 1) == SCRATCH and call(nbytes=16) == SCRATCH
        assert b"workspace" in lib.scg_last_error()
        assert call(ws=fake + 4) == ALIGN
    for H, W in ((0, 28), (20, 0), (-1, 28), (65536, 32768), (1 << 16, 1 << 16)):          # H * W >= 2^31
        assert run(H=H, W=W) == RANGE
    # range comes before NULL, NULL before the workspace's size, its size before its alignment
    assert run(N=0, depths=None) == RANGE and run(depths=None, nbytes=16) == NULL and run(nbytes=16, ws=fake + 4) == SCRATCH


def test_cpu_tensors_are_refused():
    intrs, exts, depths, kw = G.scene("small")
    ti, te, td = (torch.from_numpy(a) for a in (intrs, exts, depths))
    with pytest.raises(_lib.ScgError, match="no CPU path"):
        gc.geocheck_hip(ti, te, td, **kw)
    with pytest.raises(_lib.ScgError, match="no CPU path"):
        gc.GeoCheck(6, 24, 32, num_src=4, device="cpu")


@pytest.mark.parametrize("name", G.SCENES)
def test_restatement_is_the_oracle_on_every_scene(name):
    r = G.scene_refs(name)
    assert np.array_equal(r["r_votes"], r["o_votes"])
    assert np.array_equal(r["r_masks"], r["o_mask"]) and np.array_equal(r["r_masks"], (r["r_votes"] > r["kw"]["view_thresh"]))
    kept = r["o_mask"] > 0
    assert 0.3 < kept.mean() < 0.9                             # the check does its job on the scene: both outcomes are common
    worst = G.ulps32(r["r_filtered"][kept], r["o_depth"][kept]).max()
    print(f"{name}: restatement vs oracle, {int(kept.sum())} kept depths, max {worst:.3f} fp32 ulp")
    assert worst <= 1.0
    dropped = r["r_filtered"][~kept]
    assert np.all((dropped == 0) | np.isnan(dropped))          # a product with the mask: a hole's NaN stays NaN
    # the copy of the oracle's loop that exposes the votes is the oracle
    od, om = orc.geocheck(r["intrs"], r["exts"], r["depths"], **r["kw"])
    assert np.array_equal(om, r["o_mask"]) and np.array_equal(od, r["o_depth"], equal_nan=True)


@pytest.mark.parametrize("name", G.SCENES)
def test_near_tie_share_is_at_most_one_percent(name):
    r = G.scene_refs(name)
    share = float(r["near"].mean())
    print(f"{name}: near-tie share {share:.5f}")
    assert share <= 0.01
    assert np.array_equal(r["near"], G.near_ties(r["intrs"], r["exts"], r["depths"], num_src=r["kw"]["num_src"]))


def test_fixture_is_the_references_own_run():
    """tests/golden/ref_model.npz geo_*: masks and depths the reference's geocheck produced.  The fp64 oracle's own deviation from
    it is the yardstick of the GPU test's depth bound; it is the rounding of the reference's fp32 sum and nothing more."""
    r = G.scene_refs("fixture")
    ref = np.load(G.GOLDEN)
    same = (r["o_mask"] == ref["geo_masks"]) & (ref["geo_masks"] > 0)
    e_oracle = float((np.abs(r["o_depth"][same] - ref["geo_filtered_depths"][same]) / np.abs(ref["geo_filtered_depths"][same])).max())
    print(f"e_oracle = {e_oracle:.3e}")
    assert 0 < e_oracle < 1e-6
    off = (r["o_mask"] != ref["geo_masks"])
    assert not (off & ~r["near"]).any()


@pytest.mark.parametrize("which,num_src", [("tie", 1), ("tie", 2), ("tie", 3), ("tie", 15), ("beyond", 2), ("beyond", 3), ("beyond", 4),
                                          ("beyond", 64)])
def test_pair_table_is_get_pairs_on_planted_cameras(which, num_src):
    exts = G.planted_cameras(which)
    want = gc.get_pairs(torch.from_numpy(exts), num_src).numpy()
    got = G.pair_table(exts, num_src)
    assert got.dtype == np.int32 and got.shape == (len(exts), min(num_src, len(exts)))
    assert np.array_equal(got, want) and np.array_equal(got, orc.get_pairs(exts, num_src))
    if which == "tie":
        assert got[1, 0] == 0 and (num_src < 2 or got[1, 1] == 2)                    # the exact tie: the lower index first
        if num_src >= 3:
            assert got[:, -1].tolist() == [0, 1, 2]                                   # every view is its own last source
    elif num_src >= 4:
        assert got[0].tolist()[-2:] == [0, 3] and got[3].tolist()[0] == 3             # 1e3 sorts in front of 2000


@pytest.mark.parametrize("name", G.SCENES)
def test_pair_table_is_get_pairs_on_the_scenes(name):
    r = G.scene_refs(name)
    n_src = r["kw"]["num_src"]
    assert np.array_equal(r["r_pairs"], orc.get_pairs(r["exts"], n_src))
    assert np.array_equal(r["r_pairs"], gc.get_pairs(torch.from_numpy(r["exts"]), n_src).numpy())


def test_composed_matrices_are_the_step_by_step_transforms():
    """M1, t1, M2, t2 against numpy's own inverses and products: the composition is the reference's chain, to rounding."""
    r = G.scene_refs("small")
    K, E = r["intrs"], r["exts"]
    pairs, M1, t1, M2, t2 = G.compose(K, E, 4)
    for i in range(len(K)):
        for s, j in enumerate(pairs[i]):
            A, B = E[j] @ np.linalg.inv(E[i]), E[i] @ np.linalg.inv(E[j])
            assert np.allclose(M1[i, s], K[j] @ A[:3, :3] @ np.linalg.inv(K[i]), rtol=1e-12, atol=1e-12)
            assert np.allclose(t1[i, s], K[j] @ A[:3, 3], rtol=1e-12, atol=1e-12)
            assert np.allclose(M2[i, s], B[:3, :3] @ np.linalg.inv(K[j]), rtol=1e-12, atol=1e-12)
            assert np.allclose(t2[i, s], B[:3, 3], rtol=1e-12, atol=1e-12)
    # a singular matrix gives non-finite entries, not an exception
    assert not np.isfinite(G.inv3(np.zeros((3, 3)))).any() and not np.isfinite(G.inv4(np.zeros((4, 4)))).any()

"""CPU checks of the seeding step: the plain-torch restatement (tests/seed_refs.py) against the arrays the reference's own
create_from_pcd produced (tests/golden/ref_seed.npz), the new C-ABI entry points and their argument validation without a GPU, and the
Python binding's refusals."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import abi_text
import seed_refs as S
from scgaussian_amd import _lib, seed

FX = S.fixture()
BIT_EXACT = ("zval", "rayo", "rayd", "points", "features_dc", "features_rest", "rotation", "max_radii2D", "sparse_depths", "masks")


def _want(tag, k):
    return torch.from_numpy(FX[f"{tag}_out_{k}"])


@pytest.mark.parametrize("form", ["flat", "per_pair"])
@pytest.mark.parametrize("tag", S.SCENES)
def test_restatement_matches_the_reference_create_from_pcd(tag, form):
    arena = S.load_arena(FX, tag)
    dist2 = lambda pts: _want(tag, "dist2")                                                # noqa: E731
    if form == "flat":
        got = S.seed(arena, dist2)
    else:
        vg = S.view_gs_of(arena)
        got = S.seed_per_pair(vg, S.nested_state(vg, arena["min_loss"]), dist2)
    assert got["n"] == int(FX[f"{tag}_n"]) == _want(tag, "zval").shape[0]
    for k in BIT_EXACT:
        assert got[k].dtype == _want(tag, k).dtype and got[k].shape == _want(tag, k).shape, k
        assert torch.equal(got[k], _want(tag, k)), k
    assert torch.equal(got["opacity"], _want(tag, "opacity"))
    torch.testing.assert_close(got["scaling"], _want(tag, "scaling"), rtol=1e-6, atol=0)
    # the fp32 brute-force kNN of the oracle on the restated points is the dist2 the generator bound distCUDA2 to
    assert torch.equal(S.knn_cpu(got["points"]), _want(tag, "dist2"))


def test_fixture_holds_the_planted_rows():
    a = S.load_arena(FX, "A")
    ml, keep = a["min_loss"], S.keep_mask(a)
    tenth = torch.tensor(0.1, dtype=torch.float32)
    exact = (ml == tenth).nonzero()[:, 0]
    below = (ml == torch.nextafter(tenth, torch.tensor(0.0))).nonzero()[:, 0]
    assert exact.numel() >= 1 and not bool(keep[exact].any()) and below.numel() >= 1 and bool(keep[below].all())
    assert int(ml.isnan().sum()) == 1 and not bool(keep[ml.isnan()].any())
    assert int(ml.isneginf().sum()) == 1 and bool(keep[ml.isneginf()].all())
    offs = np.concatenate([[0], np.cumsum(a["counts"])])
    whole = [s for s in range(len(a["counts"])) if a["counts"][s] > 1 and not bool(keep[offs[s]:offs[s + 1]].any())]
    assert whole, "no whole pair is dropped"
    H, W = a["H"], a["W"]
    uv = a["uv"][keep]
    assert bool((uv[:, 0] < 0).any()) and bool((uv[:, 0] >= W).any()) and bool((uv[:, 1] == H - 0.5).any())
    # the determinism guard: distinct pixels among the kept matches of every single pair; one pixel shared by two pairs of a view
    view = np.repeat(a["seg_view"], a["counts"])
    seg = np.repeat(np.arange(len(a["counts"])), a["counts"])
    row, col = S.pixel_of(a["uv"], H, W)
    pix = {}
    for i in keep.nonzero()[:, 0].tolist():
        pix.setdefault((int(view[i]), int(row[i]), int(col[i])), []).append(int(seg[i]))
    assert all(len(set(s)) == len(s) for s in pix.values())
    assert any(len(s) == 2 for s in pix.values())
    for tag in S.SCENES:
        d2 = _want(tag, "dist2")
        assert bool(((d2 == 0) | (d2 >= 1e-3)).all())
    d = S.load_arena(FX, "D")
    assert len(d["counts"]) == 42 and set(d["counts"]) == {1, 2, 3, 5} and d["V"] == 7
    assert os.path.getsize(S.GOLDEN) < os.path.getsize(os.path.join(os.path.dirname(S.GOLDEN), "ref_densify.npz"))


def test_abi_has_the_seed_entry_points():
    lib = _lib.load()
    for name in ("scg_seed_workspace_bytes", "scg_seed_classify", "scg_seed_scatter", "scg_seed_finish"):
        assert hasattr(lib, name) and name in _lib.SYMBOLS, name
        assert abi_text.header_of(name) == "scg_raster.h", f"{name} is not declared in include/scg_raster.h"
    assert lib.scg_abi_version() == _lib.ABI_VERSION == 10
    w = lib.scg_seed_workspace_bytes
    assert w(0, 0) == 32 + 4 and w(1, 0) == 32 + 4 + 4 and w(256, 10) == 32 + 4 + 40 + 256 and w(257, 10) == 32 + 8 + 40 + 260
    assert w(-1, 0) == 0 and w(4, -1) == 0 and w(4, (1 << 31) + 1) == 0


def _segments(rows):
    t = (_lib.ScgSeedSegment * len(rows))()
    for s, (off, cnt, view) in zip(t, rows):
        s.offset, s.count, s.view = off, cnt, view
    return t


def _scatter_args(N=10, n_out=4, V=2, H=8, W=6, rows=((0, 4, 0), (4, 6, 1))):
    fake = 0x1000                                   # never dereferenced: validation fails first
    a = _lib.ScgSeedScatter()
    a.struct_bytes = C.sizeof(_lib.ScgSeedScatter)
    a.N, a.n_out, a.V, a.H, a.W, a.nseg = N, n_out, V, H, W, len(rows)
    table = _segments(rows)
    a.segments, a.segments_dev = C.addressof(table), fake
    for f in ("rays_o", "rays_d", "z", "color", "uv", "zval", "rayo", "rayd", "points", "features_dc", "features_rest", "rotation",
              "opacity_out", "max_radii2D"):
        setattr(a, f, fake)
    a._keep = table                                 # the host table lives as long as the struct
    return a


def test_seed_validation_returns_codes_without_a_gpu():
    lib = _lib.load()
    fake, big = 0x1000, 1 << 20
    cl = lambda ml=fake, N=10, px=96, ws=fake, nbytes=big: lib.scg_seed_classify(ml, N, 0.1, px, ws, nbytes, None)      # noqa: E731
    assert cl(N=-1) == -2 and b"N" in lib.scg_last_error()
    assert cl(px=-1) == -2
    assert cl(ws=None) == -1 and b"workspace" in lib.scg_last_error()
    assert cl(nbytes=lib.scg_seed_workspace_bytes(10, 96) - 1) == -4 and b"workspace" in lib.scg_last_error()
    assert cl(ws=fake + 2) == -5 and cl(ml=fake + 1) == -5

    sc = lambda a, ws=fake, nbytes=big: lib.scg_seed_scatter(a, ws, nbytes, None)          # noqa: E731
    assert sc(None) == -1
    a = _scatter_args()
    a.struct_bytes -= 8
    assert sc(C.byref(a)) == -2 and b"struct_bytes" in lib.scg_last_error()
    assert sc(C.byref(_scatter_args(N=-1))) == -2
    assert sc(C.byref(_scatter_args(H=0))) == -2 and sc(C.byref(_scatter_args(W=0))) == -2 and sc(C.byref(_scatter_args(W=-3))) == -2
    assert sc(C.byref(_scatter_args(n_out=-1))) == -2 and sc(C.byref(_scatter_args(n_out=11))) == -2
    assert sc(C.byref(_scatter_args(rows=((0, 4, 0), (4, 6, 2))))) == -2 and b"view" in lib.scg_last_error()      # view == V
    assert sc(C.byref(_scatter_args(rows=((0, 4, -1), (4, 6, 1))))) == -2 and b"view" in lib.scg_last_error()
    assert sc(C.byref(_scatter_args(rows=((0, 4, 0), (4, 7, 1))))) == -2 and b"past N" in lib.scg_last_error()
    assert sc(C.byref(_scatter_args(rows=((0, 4, 0), (5, 5, 1))))) == -2                   # a hole
    assert sc(C.byref(_scatter_args(rows=((0, 4, 0), (4, 5, 1))))) == -2 and b"cover" in lib.scg_last_error()
    assert sc(C.byref(_scatter_args(rows=()))) == -2                                        # matches but no segment
    a = _scatter_args()
    a.segments = None
    assert sc(C.byref(a)) == -1
    a = _scatter_args()
    a.segments_dev = None
    assert sc(C.byref(a)) == -1
    assert sc(C.byref(_scatter_args()), ws=None) == -1
    assert sc(C.byref(_scatter_args()), nbytes=lib.scg_seed_workspace_bytes(10, 96) - 1) == -4
    for f in ("rays_o", "uv", "zval", "features_rest", "max_radii2D"):
        a = _scatter_args()
        setattr(a, f, None)
        assert sc(C.byref(a)) == -1, f

    fin = lambda n=4, d2=fake, scl=fake, N=10, z=fake, cz=fake, V=2, H=8, W=6, sd=fake, mk=fake, ws=fake, nbytes=big: \
        lib.scg_seed_finish(n, d2, scl, N, z, cz, V, H, W, sd, mk, ws, nbytes, None)       # noqa: E731
    assert fin(N=-1) == -2 and fin(H=0) == -2 and fin(W=0) == -2 and fin(V=-1) == -2
    assert fin(n=-1) == -2 and fin(n=11) == -2
    assert fin(ws=None) == -1 and fin(nbytes=lib.scg_seed_workspace_bytes(10, 96) - 1) == -4
    assert fin(d2=None) == -1 and fin(scl=None) == -1 and fin(z=None) == -1 and fin(cz=None) == -1
    assert fin(sd=None) == -1 and fin(mk=None) == -1


def test_the_wrapper_refuses_contradicting_rows_and_cpu_tensors():
    seed.check_rows(7, 7)
    with pytest.raises(_lib.ScgError, match="contradicts"):
        seed.check_rows(6, 7)
    assert seed.raw_opacity() == float(S.raw_opacity(1, "cpu")[0, 0])

    arena = S.load_arena(FX, "A")
    vg = S.view_gs_of(arena)

    class Model:
        pass
    g = Model()
    g.view_gs = vg
    assert "create_from_pcd" not in vars(g)
    seed.install(g)
    assert g.create_from_pcd.func is seed.create_from_pcd
    with pytest.raises(_lib.ScgError, match="no CPU path"):          # never a silent torch fall-back
        g.create_from_pcd(S.nested_state(vg, arena["min_loss"]))
    with pytest.raises(_lib.ScgError, match="no CPU path"):
        g.create_from_pcd(None)
    assert not hasattr(g, "_zval")                                   # nothing was touched
    vg["view1"]["width"] = 80
    with pytest.raises(_lib.ScgError, match="unequal"):
        seed.SeedInputs.from_view_gs(vg)

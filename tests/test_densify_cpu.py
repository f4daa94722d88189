"""CPU checks of the densification path: the plain-torch restatement (tests/densify_refs.py) against the arrays the reference's own
densify_and_prune / reset_opacity produced (tests/golden/ref_densify.npz), the new C-ABI entry points and their argument
validation without a GPU, and the Python binding's refusals."""
import ctypes as C

import pytest
import torch

import densify_refs as D
from scgaussian_amd import _lib, densify

FX = D.fixture()


@pytest.mark.parametrize("tag", D.CASES)
def test_restatement_matches_the_reference_densify(tag):
    before = D.load_case(FX, tag, "in")
    got = D.load_case(FX, tag, "in")
    info = D.densify_and_prune(got, *D.case_args(FX, tag), torch.from_numpy(FX[f"{tag}_noise"]))
    want = D.load_case(FX, tag, "out")
    D.assert_same_model(got, want, before, tag)
    kept, clones, children = info["sections"]
    assert kept + clones + 2 * children == want.bg_xyz.shape[0] and clones > 0 and children > 0
    assert torch.equal(info["origin"], D.origins(before, want))


def test_fixture_holds_the_planted_rows():
    """Both exact ties are selected, the 0/0 row is not, the x/0 row is; the world-size term removes rows only with max_screen_size;
    max_radii2D (>= 100 everywhere, 1.5 * 20 = 30) removes nothing."""
    before = D.load_case(FX, "mss20", "in")
    max_grad = D.case_args(FX, "mss20")[0]
    g = (before.xyz_gradient_accum / before.denom)[:, 0]
    ties = (g == torch.tensor(max_grad, dtype=torch.float32)).nonzero()[:, 0]
    assert ties.numel() == 2 and int(g.isnan().sum()) == 1 and int(g.isinf().sum()) == 1
    nr = before._zval.shape[0]
    for tag in ("mss20", "mssnone"):
        after = D.load_case(FX, tag, "out")
        # a ray-bound source shows up among the new background rows only as a clone or as children; a background source shows
        # up once when it is merely kept and twice when it was cloned or split
        times = torch.bincount(D.origins(before, after), minlength=before.P)
        selected = torch.where(torch.arange(before.P) < nr, times >= 1, times >= 2)
        for row in list(ties) + list(g.isinf().nonzero()[:, 0]):
            assert bool(selected[row]), (tag, "row", int(row), "was not selected")
        assert not bool(selected[g.isnan().nonzero()[0, 0]])
    assert float(before.max_radii2D.min()) >= 100
    assert D.load_case(FX, "mssnone", "out").bg_xyz.shape[0] > D.load_case(FX, "mss20", "out").bg_xyz.shape[0]
    assert D.load_case(FX, "nobg", "in").bg_xyz.shape[0] == 0 and D.load_case(FX, "nobg", "in").group_state("bg_xyz") is None


def test_restatement_matches_the_reference_reset_opacity():
    before = D.load_case(FX, "reset", "in")
    got = D.load_case(FX, "reset", "in")
    D.reset_opacity(got)
    D.assert_same_model(got, D.load_case(FX, "reset", "out"), before, "reset", reset=True)
    assert float(torch.sigmoid(got._opacity.detach()).max()) <= 0.0100001


def test_abi_has_the_densify_entry_points():
    lib = _lib.load()
    for name in ("scg_densify_workspace_bytes", "scg_densify_classify", "scg_densify_scatter", "scg_reset_opacity"):
        assert hasattr(lib, name) and name in _lib.SYMBOLS, name
    assert lib.scg_struct_bytes(7) == C.sizeof(_lib.ScgDensifyScatter) > 0
    w = lib.scg_densify_workspace_bytes
    assert w(0) == 32 and w(1) == 32 + 12 + 4 and w(256) == 32 + 12 + 256 and w(257) == 32 + 24 + 260 and w(-1) == 0


def _model(nr=4, nb=3):
    fake = 0x1000                                   # never dereferenced: validation fails first
    m = _lib.ScgModel()
    m.ray.count, m.bg.count = nr, nb
    for f in ("zval", "rayo", "rayd", "features_dc", "features_rest", "opacity", "scaling", "rotation"):
        setattr(m.ray, f, fake)
    for f in ("xyz", "features_dc", "features_rest", "opacity", "scaling", "rotation"):
        setattr(m.bg, f, fake)
    return m


def test_densify_validation_returns_codes_without_a_gpu():
    lib = _lib.load()
    fake = 0x1000
    big = 1 << 20
    m = _model()
    cl = lambda model, acc=fake, den=fake, mg=4e-4, ws=fake, nbytes=big: lib.scg_densify_classify(         # noqa: E731
        model, acc, den, mg, 0.005, 0.05, 1.0, ws, nbytes, None)
    assert cl(None) == -1 and b"model" in lib.scg_last_error()
    assert cl(C.byref(_model(nr=-1))) == -2 and cl(C.byref(_model(nb=-5))) == -2
    assert cl(C.byref(m), mg=0.0) == -2 and b"max_grad" in lib.scg_last_error()
    assert cl(C.byref(m), mg=-1.0) == -2 and cl(C.byref(m), mg=float("nan")) == -2
    assert cl(C.byref(m), ws=None) == -1
    assert cl(C.byref(m), nbytes=lib.scg_densify_workspace_bytes(7) - 1) == -4 and b"workspace" in lib.scg_last_error()
    assert cl(C.byref(m), ws=fake + 2) == -5
    assert cl(C.byref(m), acc=None) == -1 and cl(C.byref(m), den=None) == -1
    hole = _model()
    hole.bg.scaling = None
    assert cl(C.byref(hole)) == -1

    a = _lib.ScgDensifyScatter()
    sc = lambda model, args, ws=fake, nbytes=big: lib.scg_densify_scatter(model, args, ws, nbytes, None)   # noqa: E731
    assert sc(None, C.byref(a)) == -1 and sc(C.byref(m), None) == -1
    a.out_rows = -1
    assert sc(C.byref(m), C.byref(a)) == -2
    a.out_rows = 3 * 7 + 1
    assert sc(C.byref(m), C.byref(a)) == -2
    a.out_rows = 5
    assert sc(C.byref(m), C.byref(a), ws=None) == -1 and sc(C.byref(m), C.byref(a), nbytes=16) == -4
    assert sc(C.byref(m), C.byref(a)) == -1 and b"output tensor" in lib.scg_last_error()
    for f in ("xyz", "features_dc", "features_rest", "opacity", "scaling", "rotation"):
        setattr(a.out, f, fake)
    a.out_exp_avg.xyz = fake                        # one moment without the other
    assert sc(C.byref(m), C.byref(a)) == -1
    a.out_exp_avg_sq.xyz = fake                     # output moments without input moments
    assert sc(C.byref(m), C.byref(a)) == -1 and b"input moments" in lib.scg_last_error()
    a.in_exp_avg.xyz = a.in_exp_avg_sq.xyz = fake
    assert sc(C.byref(m), C.byref(a)) == -2 and b"ray_scaling" in lib.scg_last_error()
    a.ray_scaling = fake
    assert sc(C.byref(m), C.byref(a)) == -1 and b"statistics" in lib.scg_last_error()
    a.accum = a.denom = a.max_radii2D = fake
    assert sc(C.byref(m), C.byref(a)) == -1 and b"noise" in lib.scg_last_error()

    assert lib.scg_reset_opacity(-1, fake, None, None, 0, None, None, None, None) == -2
    assert lib.scg_reset_opacity(4, None, None, None, 0, None, None, None, None) == -1
    assert lib.scg_reset_opacity(0, None, None, None, 3, None, None, None, None) == -1
    assert lib.scg_reset_opacity(0, None, None, None, 0, None, None, None, None) == 0


def test_install_binds_both_names_and_cpu_models_are_refused():
    g = D.load_case(FX, "mss20", "in")
    assert "densify_and_prune" not in vars(g) and "reset_opacity" not in vars(g)
    densify.install(g)
    assert callable(g.densify_and_prune) and callable(g.reset_opacity)
    assert g.densify_and_prune.func is densify.densify_and_prune and g.reset_opacity.func is densify.reset_opacity
    args = D.case_args(FX, "mss20")
    with pytest.raises(_lib.ScgError, match="no CPU path"):          # never a silent torch fall-back
        g.densify_and_prune(*args)
    with pytest.raises(_lib.ScgError, match="no CPU path"):
        g.reset_opacity()
    with pytest.raises(_lib.ScgError, match="max_grad"):
        g.densify_and_prune(0.0, *args[1:])
    assert g.bg_xyz.shape[0] == 64                                   # nothing was touched

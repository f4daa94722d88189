"""CPU-only checks of the LPIPS metric (scgaussian_amd/lpips.py, libscg_lp.so, include/lp/scg_lpips.h): the restatement the GPU
tests compare against (tests/lpips_refs.py) is held to a literal module list of vgg16().features and to the recorded fixture
(tests/golden/ref_lpips.npz); the sixth library and its binding to the header's text; the library's validation to its codes; the
scratch size to its stated arithmetic; the key mapping; the plain-torch twin (the path CPU tensors take) to the fp64 restatement
under the GPU tests' bar."""
import numpy as np
import pytest
import torch

import lpips_refs as LR
from abi_compare import VOID, check_side_library
from scgaussian_amd import _lib_lp, lpips

FX = np.load(LR.GOLDEN)
WEIGHTS = LR.make_weights()

# torchvision/models/vgg.py, vgg16().features as printed: index -> module
VGG16_FEATURES = """0 Conv2d(3,64) 1 ReLU 2 Conv2d(64,64) 3 ReLU 4 MaxPool2d 5 Conv2d(64,128) 6 ReLU 7 Conv2d(128,128) 8 ReLU 9 MaxPool2d
10 Conv2d(128,256) 11 ReLU 12 Conv2d(256,256) 13 ReLU 14 Conv2d(256,256) 15 ReLU 16 MaxPool2d 17 Conv2d(256,512) 18 ReLU
19 Conv2d(512,512) 20 ReLU 21 Conv2d(512,512) 22 ReLU 23 MaxPool2d 24 Conv2d(512,512) 25 ReLU 26 Conv2d(512,512) 27 ReLU
28 Conv2d(512,512) 29 ReLU 30 MaxPool2d""".split()


# ---- the restatement ------------------------------------------------------------------------------------------------------------
def test_tap_indices_against_the_module_list_of_vgg16_features():
    mods = dict(zip(map(int, VGG16_FEATURES[0::2]), VGG16_FEATURES[1::2]))
    assert sorted(mods) == list(range(31)) and len(LR.MODULES) == 31
    cin, convs = 3, []
    for i, m in enumerate(LR.MODULES):
        if isinstance(m, tuple):
            assert mods[i] == f"Conv2d({cin},{m[1]})", i
            convs.append(i)
            cin = m[1]
        else:
            assert mods[i] == {"relu": "ReLU", "pool": "MaxPool2d"}[m], i
    assert tuple(convs) == lpips.VGG_CONV_INDICES and len(convs) == _lib_lp.LP_LAYERS
    # target_layers counts from 1: layer i is module i - 1, the ReLU behind a block's last convolution; 30 stops before module 30
    assert [mods[i - 1] for i in LR.TARGET_LAYERS] == ["ReLU"] * 5
    assert tuple(convs.index(i - 2) for i in LR.TARGET_LAYERS) == lpips.TAP_AFTER
    assert tuple(convs.index(i + 1) for i, m in mods.items() if m == "MaxPool2d" and i < 30) == lpips.POOL_BEFORE
    assert tuple(LR.MODULES[i - 2][1] for i in LR.TARGET_LAYERS) == LR.N_CHANNELS == lpips.TAP_CHANNELS
    assert tuple((w.shape[1], w.shape[0]) for w, _ in WEIGHTS[0]) == lpips.CHANNELS
    assert (lpips.MEAN, lpips.STD, lpips.EPS) == (LR.MEAN, LR.STD, 1e-10)


def test_chain32_against_fp64_on_a_16x16_scene():
    H, W, seed = LR.SCENES[0]
    x, y = LR.make_images(H, W, seed)
    r64, rch = LR.rule(x, y, WEIGHTS), LR.chain32(x, y, WEIGHTS)
    assert rch["value"].dtype == np.float32 and all(f.dtype == np.float32 for f in rch["fx"])
    dev = LR.deviations(r64, rch)
    t = LR.tag(H, W)
    rec = dict(zip(FX[f"{t}_names"], np.maximum(FX[f"{t}_dev_torch32"], FX[f"{t}_dev_chain32"])))
    for k, wide in LR.tensors_of(r64).items():
        print(k, "chain32 deviation", dev[k], "recorded e_ref", rec[k])
        assert dev[k] <= LR.bar(rec[k], wide), k
    # a sequential fp32 sum of K <= 4608 products: far inside 1e-5 of the value, far outside fp64's agreement
    assert 1e-12 < dev["value"] < 1e-5 * float(r64["value"])
    assert all(v > 1e-4 for v in r64["terms"]), "every tap is alive at these weights"


@pytest.mark.parametrize("scene", LR.SCENES, ids=lambda s: LR.tag(s[0], s[1]))
def test_fixture_against_the_restatement(scene):
    H, W, seed = scene
    t = LR.tag(H, W)
    assert int(FX["weight_seed"]) == LR.WEIGHT_SEED and tuple(map(tuple, FX["scenes"])) == LR.SCENES
    r64 = LR.rule(*LR.make_images(H, W, seed), WEIGHTS)
    assert abs(float(r64["value"]) - float(FX[f"{t}_value"])) <= 1e-11 * float(r64["value"])
    assert np.abs(r64["terms"] - FX[f"{t}_terms"]).max() <= 1e-11 * r64["terms"].max()
    names = sorted(LR.tensors_of(r64))
    assert list(FX[f"{t}_names"]) == names and len(names) == 12
    assert np.allclose(FX[f"{t}_max"], [np.abs(LR.tensors_of(r64)[k]).max() for k in names], rtol=1e-9)
    for k in ("dev_torch32", "dev_chain32"):
        d = FX[f"{t}_{k}"]
        assert d.shape == (12,) and np.isfinite(d).all() and (d > 0).all() and (d < 1e-4 * FX[f"{t}_max"]).all(), k
    shapes = [f.shape for f in r64["fx"]]
    assert shapes == [(c, H >> l, W >> l) for l, c in enumerate(LR.N_CHANNELS)]


# ---- the sixth library against its header ---------------------------------------------------------------------------------------
def test_sixth_library_exports_and_binds_exactly_its_header():
    abi = check_side_library(_lib_lp, "lp", "scg_lpips.h", VOID)
    assert len(abi.functions) == 7 and not abi.structs
    assert {d.base for fn in abi.functions for d in fn.params if not d.pointer} <= {"int", "int32_t", "size_t"}
    assert sorted(abi.defines) == sorted("SCG_" + n for n in (
        "LP_ABI_VERSION", "LP_LAYERS", "LP_TAPS", "LP_TILE_M", "LP_HEAD_PIXELS", "LP_SMALL_GRID", "LP_MIN_DIM", "LP_MAX_DIM", "LP_MAX_PIXELS",
        "LP_MAX_BATCH", "LP_PARAM_FLOATS", "LP_RELU", "LP_POOL", "LP_ZSCORE"))
    assert _lib_lp.LP_PARAM_FLOATS == sum(9 * a * b + b for a, b in lpips.CHANNELS) + sum(lpips.TAP_CHANNELS)


# ---- scratch sizes and validation, without a GPU ----------------------------------------------------------------------------------
def _stated_scratch(H, W):
    h, w, P = H, W, []
    for _ in range(5):
        P.append(h * w)
        h, w = h // 2, w // 2
    floats = 2 * (64 * P[0] + 64 * P[0] + 128 * P[1] + 256 * P[2] + 256 * P[2] + 512 * P[3] + 512 * P[4])
    return 4 * floats + 8 * 5 * -(-P[0] // _lib_lp.LP_HEAD_PIXELS), 2 * sum(p * c for p, c in zip(P, lpips.TAP_CHANNELS))


def test_scratch_and_feature_sizes():
    lib = _lib_lp.load()
    for H, W in ((16, 16), (17, 19), (33, 47), (48, 80), (378, 504), (1200, 1600), (4096, 4096)):
        nbytes, floats = _stated_scratch(H, W)
        assert lib.scg_lp_scratch_bytes(H, W) == nbytes and lib.scg_lp_feature_floats(H, W) == floats, (H, W)
    assert 0.30e9 < lib.scg_lp_scratch_bytes(378, 504) < 0.32e9 and 3.0e9 < lib.scg_lp_scratch_bytes(1200, 1600) < 3.2e9      # as stated
    for bad in ((15, 16), (16, 15), (0, 16), (-1, 16), (16385, 16), (16, 16385), (4096, 4097)):
        assert lib.scg_lp_scratch_bytes(*bad) == 0 and lib.scg_lp_feature_floats(*bad) == 0, bad


def test_validation_returns_codes_without_a_gpu():
    """Every call below fails its validation before anything touches a device: the device pointers are never dereferenced."""
    lib = _lib_lp.load()
    err = lib.scg_lp_last_error
    fake, big = 0x1000, 1 << 40
    fwd = dict(H=17, W=19, x=fake, y=fake, params=fake, value=fake, terms=fake, features=None, scratch=fake, nbytes=big)
    call_f = lambda **k: lib.scg_lp_forward(*{**fwd, **k}.values(), None)      # noqa: E731
    need = lib.scg_lp_scratch_bytes(17, 19)
    for k in ("x", "y", "params", "value", "terms", "scratch"):
        assert call_f(**{k: None}) == -1 and b"NULL" in err(), k
    for k, off in (("x", 2), ("y", 1), ("params", 4), ("value", 2), ("terms", 2), ("features", 8), ("scratch", 8)):
        assert call_f(**{k: fake + off}) == -5 and b"aligned" in err(), k
    assert call_f(x=fake + 4, y=fake + 4, nbytes=need - 1) == -4 and b"scratch of" in err()      # images need 4-byte alignment only
    for bad in (dict(H=15, W=16), dict(H=16, W=15), dict(H=0), dict(W=-3), dict(H=16385), dict(H=4096, W=4097)):
        assert call_f(**bad) == -2, bad
    assert b"H * W" in err()
    head = dict(H=17, W=19, params=fake, value=fake, terms=fake, features=None, scratch=fake, nbytes=big)
    call_h = lambda **k: lib.scg_lp_head(*{**head, **k}.values(), None)      # noqa: E731
    assert [call_h(params=None), call_h(scratch=None), call_h(value=fake + 1), call_h(features=fake + 4), call_h(nbytes=need - 1),
            call_h(H=15), call_h(scratch=fake + 4)] == [-1, -1, -5, -5, -4, -2, -5]
    conv = dict(n=2, cin=64, cout=128, h=5, w=7, inp=fake, weights=fake, bias=fake, out=fake, flags=_lib_lp.LP_RELU)
    call_c = lambda **k: lib.scg_lp_conv3x3(*{**conv, **k}.values(), None)      # noqa: E731
    for k in ("inp", "weights", "bias", "out"):
        assert call_c(**{k: None}) == -1, k
        assert call_c(**{k: fake + 4}) == -5, k
    for bad in (dict(cin=64, cout=256), dict(cin=3, cout=128), dict(cin=128, cout=64), dict(cin=0), dict(n=0), dict(n=3), dict(h=0),
                dict(w=16385), dict(flags=8), dict(flags=-1), dict(h=1, flags=_lib_lp.LP_POOL), dict(w=1, flags=_lib_lp.LP_POOL)):
        assert call_c(**bad) == -2, bad
    assert call_c(flags=_lib_lp.LP_ZSCORE) == -3 and call_c(cin=3, cout=64, flags=_lib_lp.LP_POOL) == -3 and b"z-score" in err()
    for cin, cout in sorted(set(lpips.CHANNELS)):
        assert call_c(cin=cin, cout=cout, flags=0, out=None) == -1, (cin, cout)           # the pair itself is accepted
    assert len(set(lpips.CHANNELS)) == 8


# ---- the key mapping ------------------------------------------------------------------------------------------------------------
def test_key_mapping():
    vgg, lin = LR.state_dicts(WEIGHTS)
    bare, renamed = LR.state_dicts(WEIGHTS, vgg_prefix="", published=False)
    assert sorted(vgg)[:2] == ["features.0.bias", "features.0.weight"] and "lin0.model.1.weight" in lin and "0.1.weight" in renamed
    for v, l in ((vgg, lin), (bare, renamed), (vgg, renamed)):
        convs, lins = lpips.map_vgg_keys({**v, "classifier.0.weight": torch.zeros(1)}), lpips.map_lin_keys(l)
        assert all(a is b and c is d for (a, c), (b, d) in zip(convs, WEIGHTS[0])) and all(a is b for a, b in zip(lins, WEIGHTS[1]))
    missing = {k: t for k, t in vgg.items() if k != "features.17.bias"}
    with pytest.raises(ValueError, match=r"features\.17\.bias"):
        lpips.map_vgg_keys(missing)
    with pytest.raises(ValueError, match=r"features\.5\.weight"):
        lpips.map_vgg_keys({**vgg, "features.5.weight": torch.zeros(128, 64, 3, 2)})
    with pytest.raises(ValueError, match=r"lin3\.model\.1\.weight"):
        lpips.map_lin_keys({k: t for k, t in lin.items() if not k.startswith("lin3")})
    with pytest.raises(ValueError, match=r"2\.1\.weight"):
        lpips.map_lin_keys({**renamed, "2.1.weight": torch.zeros(1, 128, 1, 1)})
    with pytest.raises(ValueError, match="missing"):
        lpips.Lpips.from_state_dicts({}, lin, device="cpu")


def test_from_files_reads_plain_state_dicts(tmp_path):
    vgg, lin = LR.state_dicts(WEIGHTS)
    torch.save(vgg, tmp_path / "vgg16.pth")
    torch.save(lin, tmp_path / "vgg.pth")
    lp = lpips.Lpips.from_files(str(tmp_path / "vgg16.pth"), str(tmp_path / "vgg.pth"), device="cpu")
    assert all(torch.equal(a, b) for (a, _), (b, _) in zip(lp.convs, WEIGHTS[0])) and torch.equal(lp.lins[4], WEIGHTS[1][4])


# ---- the twin: the path CPU tensors take ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene", LR.SCENES[:4], ids=lambda s: LR.tag(s[0], s[1]))
def test_twin_on_cpu_tensors_meets_the_bar(scene):
    H, W, seed = scene
    t = LR.tag(H, W)
    x, y = LR.make_images(H, W, seed)
    lp = lpips.Lpips.from_state_dicts(*LR.state_dicts(WEIGHTS), device="cpu")
    value = lp(torch.from_numpy(x), torch.from_numpy(y)[None])
    assert value.shape == (1, 1, 1, 1) and value.dtype == torch.float32 and lp.terms.shape == (5,)
    r64 = LR.rule(x, y, WEIGHTS)
    e_ref = dict(zip(FX[f"{t}_names"], np.maximum(FX[f"{t}_dev_torch32"], FX[f"{t}_dev_chain32"])))
    fx, fy = lp.features(torch.from_numpy(x), torch.from_numpy(y))
    got = {"value": value.reshape(()).numpy(), "terms": lp.terms.numpy(), **{f"fx{l}": f[0].numpy() for l, f in enumerate(fx)},
           **{f"fy{l}": f[0].numpy() for l, f in enumerate(fy)}}
    for k, wide in LR.tensors_of(r64).items():
        dev = float(np.abs(got[k].astype(np.float64) - wide).max())
        print(t, k, "twin deviation", dev, "e_ref", e_ref[k], "bar", LR.bar(e_ref[k], wide))
        assert dev <= LR.bar(e_ref[k], wide), k
    with pytest.raises(ValueError, match="H, W >= 16"):
        lp(torch.zeros(3, 15, 16), torch.zeros(3, 15, 16))
    with pytest.raises(ValueError, match="one shape"):
        lp(torch.zeros(3, 16, 16), torch.zeros(3, 16, 17))

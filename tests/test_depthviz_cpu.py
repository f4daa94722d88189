"""CPU-side checks of the depth colour maps and video frames (csrc/depthviz.hip, include/scg_viz.h, scgaussian_amd/video.py): the
ABI, the argument validation, and the restatement the GPU tests lean on.  No kernel runs here.

What anchors what: depthviz_refs restates the rule; it is held here, bit for bit, to np.percentile on a few thousand random planes, to
matplotlib's own mapper where matplotlib is installed, and to tests/golden/ref_depthviz.npz, which was recorded from both."""
import inspect
import os
import types
import warnings

import numpy as np
import pytest
import torch

import abi_text
import depthviz_refs as D
from scgaussian_amd import _lib, evaluate, video

NEW_SYMBOLS = ("scg_viz_select_block", "scg_viz_select_scratch_bytes", "scg_viz_select", "scg_viz_frame")
NULL, RANGE, SCRATCH, ALIGN = -1, -2, -4, -5
f32 = np.float32


def _plane(rng, n, kind):
    x = rng.random(n, dtype=f32)
    if kind == 1:
        x = (np.floor(x * 8) / 8).astype(f32)                 # ties
    elif kind == 2:
        x = ((x - f32(0.5)) * f32(100)).astype(f32)           # both signs, vmin != 0
    elif kind == 3 and n > 1:
        x = D.normalised(x * f32(5) + f32(1))                 # what both scripts colour
    return x


def test_new_symbols_are_declared_exported_and_bound():
    lib = _lib.load()
    declared = abi_text.declared_by("scg_viz.h")
    assert declared == sorted(NEW_SYMBOLS)
    for name in declared:
        assert name in _lib.SYMBOLS, f"ctypes binding lacks {name}"
        assert hasattr(lib, name), f"libscg_raster.so does not export {name}"
    assert lib.scg_abi_version() == _lib.ABI_VERSION
    block = lib.scg_viz_select_block()
    assert block >= 256 and block % 256 == 0
    from scgaussian_amd import build
    assert "-ffp-contract=off" in build.SOURCES["depthviz.hip"]
    assert any(h.endswith("scg_viz.h") for h in build.HEADERS)
    assert all(hasattr(video, n) for n in ("TURBO", "DepthColorizer", "colorize_depth", "render_video"))


def test_scratch_bytes():
    ws = _lib.load().scg_viz_select_scratch_bytes
    assert ws(1) > 0 and ws(1 << 24) >= ws(1)
    for n in (0, -1, (1 << 24) + 1, 1 << 31):
        assert ws(n) == 0


def test_argument_validation_returns_codes_without_a_gpu():
    lib = _lib.load()
    fake = 0x10000            # never dereferenced: validation fails first
    big = 1 << 30

    def select(depth=fake, rng=None, n=1000, p=98.0, stats=fake, nan=fake, ws=fake, nbytes=big):
        return lib.scg_viz_select(depth, rng, n, p, stats, nan, ws, nbytes, None)

    def frame(render=None, depth=fake, rng=None, stats=fake, nan=fake, lut=fake, H=20, W=28, rgb=fake, bgr=None, grey=None, r8=None, fb=None):
        return lib.scg_viz_frame(render, depth, rng, stats, nan, lut, H, W, rgb, bgr, grey, r8, fb, None)

    for k in ("depth", "stats", "nan", "ws"):
        assert select(**{k: None}) == NULL, k
    for n in (0, -5, (1 << 24) + 1, 1 << 40):
        assert select(n=n) == RANGE
    assert b"2^24" in lib.scg_last_error()
    for p in (-0.001, 100.001, float("nan"), float("inf")):
        assert select(p=p) == RANGE
    assert b"percentile" in lib.scg_last_error()
    need = lib.scg_viz_select_scratch_bytes(1000)
    assert select(nbytes=need - 1) == SCRATCH and select(nbytes=0) == SCRATCH
    assert select(ws=fake + 2) == ALIGN
    # range comes before NULL, NULL before the scratch's size, its size before its alignment
    assert select(n=0, depth=None) == RANGE and select(depth=None, nbytes=16) == NULL and select(nbytes=16, ws=fake + 2) == SCRATCH

    for k in ("depth", "stats", "nan", "lut", "rgb"):
        assert frame(**{k: None}) == NULL, k
    assert frame(r8=fake) == NULL and frame(fb=fake) == NULL            # they need a render
    assert b"render" in lib.scg_last_error()
    for H, W in ((0, 28), (20, 0), (-1, 28), (65536, 32768)):
        assert frame(H=H, W=W) == RANGE
    assert frame(H=0, depth=None) == RANGE


def test_cpu_tensors_and_bad_arguments_are_refused():
    with pytest.raises(_lib.ScgError, match="no CPU path"):
        video.DepthColorizer(8, 8, device="cpu")
    with pytest.raises(_lib.ScgError, match="no CPU path"):
        video.colorize_depth(torch.rand(8, 8))
    with pytest.raises(ValueError, match="256x3"):
        video._as_lut(np.zeros((255, 3), np.uint8))
    with pytest.raises(ValueError, match="256x3"):
        video._as_lut(np.zeros((256, 3), np.float32))
    views = [types.SimpleNamespace(image_height=40, image_width=56), types.SimpleNamespace(image_height=40, image_width=57)]
    with pytest.raises(ValueError, match="one size"):
        video.render_video(views, None, None, torch.zeros(3))
    with pytest.raises(ValueError, match="at least one view"):
        video.render_video([], None, None, torch.zeros(3))


def test_ranks_at_known_sizes():
    assert D.ranks(1) == (0, 0, f32(0)) and D.ranks(2, 100) == (1, 1, f32(0)) and D.ranks(2, 0) == (0, 1, f32(0))
    lo, hi, g = D.ranks(101, 50)
    assert (lo, hi, g) == (50, 51, f32(0))
    lo, hi, g = D.ranks(1 << 24, 100)
    assert lo == hi == (1 << 24) - 1 and g == 0
    for n in (3, 64, 4097, 1080 * 1920):
        lo, hi, g = D.ranks(n)
        assert 0 <= lo <= hi <= n - 1 and hi - lo <= 1 and 0 <= g < 1


def test_percentile_restatement_is_numpy_on_random_planes():
    """2 000 planes of 1 .. 20 000 values and 40 of up to 1080 x 1920, every kind of content, four percentiles in turn."""
    rng = np.random.default_rng(1)
    sizes = [int(np.exp(rng.uniform(0, np.log(20000)))) for _ in range(2000)]
    sizes += [int(rng.integers(1, 1081)) * int(rng.integers(1, 1921)) for _ in range(40)]
    sizes[:6] = [1, 2, 3, 4, 1080 * 1920, 1079 * 1919]
    ps = (98, 0, 50, 100, 98, 37.5, 99.9)
    for i, n in enumerate(sizes):
        x = _plane(rng, n, i % 4)
        p = ps[i % len(ps)]
        want = np.percentile(x, p)
        vmin, vmax, a, b = D.stats(x, p)
        assert want.dtype == np.float32
        assert vmax.view(np.uint32) == want.view(np.uint32), (n, p, vmax, want)
        assert vmin == x.min() and a <= vmax <= b


def test_percentile_restatement_with_nan_and_inf():
    rng = np.random.default_rng(2)
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        for n in (1, 2, 25, 200, 4097):
            for where in (0, n // 2, n - 1):
                x = _plane(rng, n, 0)
                x[where] = np.nan
                vmin, vmax, _, _ = D.stats(x)
                assert np.isnan(vmin) and np.isnan(vmax) and np.isnan(np.percentile(x, 98)) and np.isnan(x.min())
        x = _plane(rng, 25, 0)
        x[7] = np.inf                                         # rank hi = 24: inf - inf * (1 - g)
        assert np.isnan(D.stats(x)[1]) and np.isnan(np.percentile(x, 98)) and D.stats(x)[0] == x.min()
        x[7] = -np.inf
        assert D.stats(x)[0] == -np.inf and D.stats(x)[1].view(np.uint32) == np.percentile(x, 98).view(np.uint32)


def test_colour_restatement_is_matplotlibs_mapper():
    mpl = pytest.importorskip("matplotlib")
    import matplotlib.cm as cm
    rng = np.random.default_rng(3)
    shapes = [(int(rng.integers(1, 48)), int(rng.integers(1, 48))) for _ in range(400)] + [(270, 480), (301, 397), (1080, 1920)]
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        for i, (H, W) in enumerate(shapes):
            x = _plane(rng, H * W, i % 4).reshape(H, W)
            if i % 23 == 5:
                x[0, 0] = np.nan
            if i % 29 == 7:
                x[-1, -1] = np.inf
            mapper = cm.ScalarMappable(norm=mpl.colors.Normalize(vmin=x.min(), vmax=np.percentile(x, 98)), cmap="turbo")
            want = (mapper.to_rgba(x)[:, :, :3] * 255).astype(np.uint8)
            assert np.array_equal(D.colorize(x, video.TURBO), want), (H, W, i % 4)


def test_turbo_table_is_matplotlibs():
    mpl = pytest.importorskip("matplotlib")
    cmap = mpl.colormaps["turbo"]
    assert cmap.N == 256
    want = (cmap(np.arange(256))[:, :3] * 255).astype(np.uint8)
    assert video.TURBO.shape == (256, 3) and video.TURBO.dtype == np.uint8 and np.array_equal(video.TURBO, want)
    # the table's under and over colours are its ends, and its bad colour is black
    assert np.array_equal((np.array(cmap(-1.0)[:3]) * 255).astype(np.uint8), want[0])
    assert np.array_equal((np.array(cmap(2.0)[:3]) * 255).astype(np.uint8), want[255])
    assert tuple(cmap(np.nan)) == (0.0, 0.0, 0.0, 0.0)
    assert not video.TURBO.flags.writeable


def test_restatement_against_the_fixture():
    z = np.load(D.GOLDEN)
    names = [str(n) for n in z["names"]]
    assert len(names) >= 20
    for p in (0, 50, 98, 100):
        assert any(float(z[f"{n}_p"]) == p for n in names)
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        for n in names:
            x, p = z[f"{n}_x"], float(z[f"{n}_p"])
            vmin, vmax, a, b = D.stats(x, p)
            assert D.same_stats([vmin, vmax], [z[f"{n}_vmin"], z[f"{n}_vmax"]]), n
            assert np.array_equal(D.colorize(x, video.TURBO, p), z[f"{n}_rgb"]), n
    assert np.array_equal(D.video_frame(z["frame_render"]), z["frame_bgr"])
    assert np.isnan(z["one_nan_vmax"]) and np.isnan(z["pos_inf_at_hi_vmax"]) and np.isfinite(z["pos_inf_above_vmax"])
    assert not z["pos_inf_at_hi_rgb"].any() and not z["all_nan_rgb"].any() and not z["neg_inf_min_rgb"].any()
    assert (z["constant_rgb"] == video.TURBO[0]).all() and float(z["zero_one_vmax"]) == 1.0


def test_keys_are_ordered_as_the_values():
    rng = np.random.default_rng(4)
    x = np.concatenate([((rng.random(2000, dtype=f32) - f32(0.5)) * f32(1e3)).astype(f32),
                        np.array([0.0, -0.0, np.inf, -np.inf, 1e-45, -1e-45, 1e-39, 3.4e38, -3.4e38], f32)])
    k = D.key_of(x)
    order = np.argsort(k, kind="stable")
    assert np.all(np.diff(x[order]) >= 0)
    assert np.array_equal(D.value_of(k).view(np.uint32), x.view(np.uint32))
    assert D.key_of(f32(-0.0)) + 1 == D.key_of(f32(0.0))


def test_render_set_default_path_is_untouched(tmp_path, monkeypatch):
    """With a stand-in for the GPU work: the default writes the five directories and keys of before; color_depth adds one key and
    one file per view."""
    assert inspect.signature(evaluate.render_set).parameters["color_depth"].default is False
    assert "matplotlib depth visualisation" not in evaluate.render_set.__doc__ and "color_depth" in evaluate.render_set.__doc__
    H, W = 6, 8
    u8 = lambda *s: torch.zeros(s, dtype=torch.uint8)          # noqa: E731

    class FakeSet:
        def __init__(self, n, lpips_fn=None, device=None):
            self.n = 0

        def add(self, name, rendering, gt, depth, dtumask=None):
            self.n += 1
            return {"renders": u8(H, W, 3), "gt": u8(H, W, 3), "depth": u8(H, W), "error_map": u8(H, W), "dtumask": None,
                    "renders_masked": None, "record": None}

        def results(self):
            return {"SSIM": 1.0, "PSNR": 30.0}, {"SSIM": {}, "PSNR": {}}

    class FakeColorizer:
        def __init__(self, H, W, device=None):
            self.shape = (H, W, 3)

        def colorize_depth(self, depth):
            return torch.full(self.shape, 7, dtype=torch.uint8)

    monkeypatch.setattr(evaluate, "EvalSet", FakeSet)
    monkeypatch.setattr(video, "DepthColorizer", FakeColorizer)
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: None)
    render = lambda v, g, p, b: {"render": torch.zeros(3, H, W), "rendered_depth": torch.zeros(1, H, W)}          # noqa: E731
    views = [types.SimpleNamespace(original_image=torch.zeros(3, H, W)) for _ in range(2)]

    def tree(root):
        return sorted(os.path.relpath(os.path.join(d, f), root) for d, _, fs in os.walk(root) for f in fs)

    full, per_view, images = evaluate.render_set(views, None, None, torch.zeros(3), out_dir=str(tmp_path / "a"), iteration=3, render=render)
    assert [sorted(im) for im in images] == [sorted(("renders", "gt", "depth", "error_map", "dtumask"))] * 2
    want = sorted(os.path.join("test", "ours_3", sub, f"{i:05d}.png") for sub in ("renders", "gt", "depth", "error_map") for i in range(2))
    assert tree(tmp_path / "a") == want and list(full) == ["ours_3"]
    _, _, images = evaluate.render_set(views, None, None, torch.zeros(3), out_dir=str(tmp_path / "b"), iteration=3, render=render,
                                       color_depth=True)
    assert [sorted(im) for im in images] == [sorted(("renders", "gt", "depth", "error_map", "dtumask", "depth_color"))] * 2
    assert tree(tmp_path / "b") == sorted(want + [os.path.join("test", "ours_3", "depth", f"color_{i:05d}.png") for i in range(2)])

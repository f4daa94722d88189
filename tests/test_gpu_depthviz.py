"""The depth colour maps and video frames on the GPU (scgaussian_amd/video.py, csrc/depthviz.hip) against the numpy restatement of
tests/depthviz_refs.py and what numpy and matplotlib themselves produced (tests/golden/ref_depthviz.npz).

Every comparison is bit for bit: the feature is an integer selection plus a fixed chain of separately rounded operations, there is no
tolerance to measure.  The one exception: a zero among the stats is compared by value, since -0.0 and +0.0 tie in numpy's order.

Sizes come from the select kernel's block (scg_viz_select_block): one value, a partly filled wave, a partly filled workgroup, more
than one workgroup; the frame kernel's four pixels per thread: sizes that are no multiple of four, outputs at unaligned addresses."""
import types
import warnings

import numpy as np
import pytest
import torch

import depthviz_refs as D
from scgaussian_amd import _lib, evaluate, video
from scgaussian_amd import render as rmod
from scgaussian_amd import synthetic as syn

pytestmark = pytest.mark.gpu
DEV = "cuda"
f32 = np.float32
BLOCK = _lib.load().scg_viz_select_block()
PERCENTILES = (0.0, 50.0, 98.0, 100.0)
_VIZ = {}


def _viz(H, W, p=98.0, lut=None):
    key = (H, W, p, None if lut is None else lut.tobytes())
    if key not in _VIZ:
        _VIZ[key] = video.DepthColorizer(H, W, percentile=p, **({} if lut is None else {"lut": lut}))
    return _VIZ[key]


def _t(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=f32)).to(DEV)


def _select(x, p=98.0, rng=None):
    """(stats (4,) fp32, nan count) of the plane x on the GPU"""
    x = np.atleast_2d(x)
    viz = _viz(x.shape[0], x.shape[1], p)
    st = viz.stats(_t(x), None if rng is None else _t(rng)).cpu().numpy().copy()
    return st, int(viz.nan_count)


def _colorize(x, p=98.0, rng=None, lut=None, **kw):
    x = np.atleast_2d(x)
    return _viz(x.shape[0], x.shape[1], p, lut).colorize(_t(x), None if rng is None else _t(rng), **kw).cpu().numpy()


def _check_select(x, p=98.0, what=""):
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        want = D.stats(x, p)
    got, nans = _select(x, p)
    assert D.same_stats(got, want), (what, p, got, want)
    assert nans == int(np.isnan(x).sum()), what
    return got


def _plane(rng, n, kind):
    x = rng.random(n, dtype=f32)
    if kind == 1:
        x = (np.floor(x * 8) / 8).astype(f32)
    elif kind == 2:
        x = ((x - f32(0.5)) * f32(100)).astype(f32)
    elif kind == 3 and n > 1:
        x = D.normalised(x * f32(5) + f32(1))
    return x


SIZES = [1, 2, 3, 63, 64, 65, 255, 256, 257, BLOCK - 1, BLOCK, BLOCK + 1, 2 * BLOCK + 1]


@pytest.mark.parametrize("p", PERCENTILES)
def test_select_at_the_block_edges_and_small_shapes(p):
    rng = np.random.default_rng(int(p))
    for i, n in enumerate(SIZES):
        _check_select(_plane(rng, n, i % 4), p, f"n={n}")
    for i, (H, W) in enumerate(((3, 3), (5, 7), (9, 31), (17, 65), (300, 400))):
        _check_select(_plane(rng, H * W, (i + 1) % 4).reshape(H, W), p, f"{H}x{W}")


def test_select_interpolation_weights():
    """g = 0, g just below 0.5 and g just above it: the two branches of numpy's _lerp, on values far enough apart to tell them."""
    assert D.ranks(101, 50)[2] == 0
    gs = {(n, p): D.ranks(n, p)[2] for n in range(3, 2 * BLOCK + 100) for p in (98.0, 49.99, 50.01)}
    below = max((k for k in gs if gs[k] < 0.5), key=lambda k: (gs[k], k))
    above = min((k for k in gs if gs[k] >= 0.5), key=lambda k: (gs[k], -k[0]))
    assert 0.499 < gs[below] < 0.5 <= gs[above] < 0.501
    rng = np.random.default_rng(7)
    for n, p in ((101, 50.0), below, above, (26, 98.0)):
        x = (rng.permutation(n).astype(f32) * f32(1.7) + f32(0.3)).astype(f32)
        got = _check_select(x, p, f"n={n}")
        lo, hi, g = D.ranks(n, p)
        assert got[2] == np.sort(x)[lo] and got[3] == np.sort(x)[hi] and (g == 0) == (got[1] == got[2])


def test_select_runs_of_equal_values():
    const = np.full((7, 9), 0.625, f32)
    assert _check_select(const).tolist() == [0.625] * 4
    assert (_colorize(const) == video.TURBO[0]).all()
    n = 200
    lo, hi, _ = D.ranks(n)
    assert (lo, hi) == (195, 196)
    rng = np.random.default_rng(8)
    for first_one, want_ab in ((197, (0, 0)), (196, (0, 1)), (195, (1, 1))):
        x = np.zeros(n, f32)
        x[first_one:] = 1
        got = _check_select(rng.permutation(x).reshape(8, 25), 98.0, f"ones from rank {first_one}")
        assert (got[2], got[3]) == want_ab and got[0] == 0


@pytest.mark.parametrize("shift", [28, 21, 20, 12, 10, 9, 5, 0])
def test_select_ranks_whose_keys_part_at_every_byte_and_digit(shift):
    """Rank lo and rank hi hold keys that first differ at bit `shift`: in the top, second, third and lowest byte, and on both sides
    of the borders between the kernel's digits."""
    n = 200
    lo, hi, _ = D.ranks(n)
    rng = np.random.default_rng(shift)
    top = 0xC0100155 & ~((1 << (shift + 1)) - 1)             # the bits both keys share
    a_key = top | int(rng.integers(0, 1 << shift))
    b_key = top | (1 << shift) | int(rng.integers(0, 1 << shift))
    assert a_key < b_key and int(a_key ^ b_key).bit_length() - 1 == shift
    below = a_key - rng.integers(1, 1 << 30, lo)
    above = b_key + rng.integers(1, 1 << 28, n - hi - 1)
    x = D.value_of(rng.permutation(np.concatenate([below, [a_key, b_key], above])).astype(np.uint32))
    assert np.isfinite(x).all()
    got = _check_select(x.reshape(10, 20), 98.0, f"shift {shift}")
    assert got[2].view(np.uint32) == a_key ^ 0x80000000 and got[3].view(np.uint32) == b_key ^ 0x80000000          # positive floats


def test_select_signs_zeros_denormals():
    rng = np.random.default_rng(9)
    for p in PERCENTILES:
        _check_select(((rng.random((13, 17), dtype=f32) - f32(0.5)) * f32(8)).astype(f32), p, "mixed signs")
        _check_select((-rng.random((6, 11), dtype=f32) - f32(1)).astype(f32), p, "all negative")
        x = np.zeros((4, 6), f32)
        x[::2] = -0.0
        _check_select(x, p, "signed zeros only")
        x[1, 2], x[3, 3] = 0.5, -0.25
        _check_select(x, p, "signed zeros")
        d = (rng.random((5, 8), dtype=f32) * f32(1e-39)).astype(f32)
        d[0, 0], d[1, 1] = 0, -1e-42
        assert (np.abs(d[d != 0]) < np.finfo(f32).tiny).all()
        _check_select(d, p, "denormals")


def test_select_infinities():
    rng = np.random.default_rng(10)
    x = rng.random((5, 5), dtype=f32)
    x[1, 1] = np.inf                                          # n = 25: rank hi is the last one: inf - inf * (1 - g)
    got = _check_select(x, 98.0, "+inf at rank hi")
    assert np.isnan(got[1]) and np.isinf(got[3]) and np.isfinite(got[0])
    assert not _colorize(x).any()
    x = rng.random((10, 20), dtype=f32)
    x[4, 4] = np.inf                                          # above rank hi: vmax finite, the pixel takes the table's last entry
    got = _check_select(x, 98.0, "+inf above rank hi")
    img = _colorize(x)
    assert np.isfinite(got[1]) and (img[4, 4] == video.TURBO[255]).all() and np.array_equal(img, D.colorize(x, video.TURBO))
    x[0, 5] = -np.inf
    got = _check_select(x, 98.0, "-inf as the minimum")
    assert got[0] == -np.inf and not _colorize(x).any()


@pytest.mark.parametrize("n", [1, 65, BLOCK + 1])
def test_one_nan_makes_both_scalars_nan(n):
    rng = np.random.default_rng(n)
    for where in sorted({0, n // 2, n - 1}):
        x = rng.random(n, dtype=f32)
        x[where] = np.nan
        got = _check_select(x, 98.0, f"NaN at {where} of {n}")
        assert np.isnan(got[0]) and np.isnan(got[1])
        assert not _colorize(x).any()


def test_with_and_without_range():
    rng = np.random.default_rng(11)
    H, W = 37, 53
    depth = (2 + 30 * rng.random((H, W), dtype=f32) ** 2).astype(f32)
    x = D.normalised(depth)
    r = np.array([depth.min(), depth.max()], f32)
    got, _ = _select(depth, 98.0, r)
    assert D.same_stats(got, D.stats(x)) and got[0] == 0
    viz = _viz(H, W)
    assert np.array_equal(viz.depth_range(_t(depth)).cpu().numpy(), r)
    want = D.colorize(x, video.TURBO)
    assert np.array_equal(_colorize(depth, rng=r), want)
    assert np.array_equal(viz.colorize_depth(_t(depth)[None]).cpu().numpy(), want)
    assert np.array_equal(video.colorize_depth(_t(depth)).cpu().numpy(), want)
    assert np.array_equal(_colorize(depth), D.colorize(depth, video.TURBO))          # without: the raw plane
    assert float(viz.vmin) == float(depth.min()) and float(viz.vmax) == float(np.percentile(depth, 98))
    # a raw depth with max == min: the normalised plane is NaN throughout, the image zero
    flat = np.full((H, W), 2.5, f32)
    got, nans = _select(flat, 98.0, np.array([2.5, 2.5], f32))
    assert np.isnan(got).all() and nans == H * W
    assert not viz.colorize_depth(_t(flat)).cpu().numpy().any()


def _planted_plane():
    """4 096 values, vmin = 0, a run of exact ones across ranks lo and hi (vmax = 1), and for every k in 1..256 the value whose
    fl(t * 256) is exactly k and the one an ulp below it; t == 1 and values above 1 above rank hi."""
    n = 4096
    lo, hi, _ = D.ranks(n)
    ks = (np.arange(1, 257, dtype=f32) / f32(256)).astype(f32)
    planted = np.concatenate([ks, np.nextafter(ks, f32(0))])
    over = np.array([1.0000001, 1.5, 2.0, 255.0, 256.0, 1e30, np.inf, 1.25], f32)
    ones = np.ones(100, f32)
    rng = np.random.default_rng(12)
    rest = rng.random(n - len(planted) - len(over) - len(ones) - 1, dtype=f32)
    x = rng.permutation(np.concatenate([planted, over, ones, np.zeros(1, f32), rest]).astype(f32))
    s = np.sort(x)
    assert len(x) == n and s[lo] == 1 and s[hi] == 1 and s[0] == 0 and (x > 1).sum() == len(over)
    return x.reshape(64, 64)


def test_frame_index_at_every_table_boundary():
    x = _planted_plane()
    got, _ = _select(x)
    assert got.tolist() == [0.0, 1.0, 1.0, 1.0]
    idx, bad = D.index(x, 0, 1)
    assert not bad.any() and set(np.unique(idx)) == set(range(256))
    for k in range(1, 256):
        assert idx[x == f32(k) / f32(256)].tolist() == [k] * int((x == f32(k) / f32(256)).sum())
        assert (idx[x == np.nextafter(f32(k) / f32(256), f32(0))] == k - 1).all()
    assert (idx[x >= 1] == 255).all()
    img = _colorize(x)
    assert np.array_equal(img, video.TURBO[idx]) and np.array_equal(img, D.colorize(x, video.TURBO))
    assert np.array_equal(_colorize(x, bgr=True), img[..., ::-1])
    lut = np.random.default_rng(13).integers(0, 256, (256, 3)).astype(np.uint8)
    assert np.array_equal(_colorize(x, lut=lut), lut[idx])
    assert np.array_equal(_colorize(x, lut=lut, bgr=True), lut[idx][..., ::-1])


def test_frame_with_stats_of_another_plane():
    """s < 0 and s >= 256 through the C entry: stats the caller wrote, as a graph that colours several planes by one range would."""
    lib = _lib.load()
    H, W = 9, 21
    for st, scale in (((0.25, 0.75), 1), ((-49.99981, 48.014668), 40), ((0.3, 0.3), 1)):
        x = (np.linspace(-0.5, 1.5, H * W, dtype=f32) * f32(scale)).reshape(H, W)
        stats = _t(np.array([st[0], st[1], 0, 0], f32))
        nan = torch.zeros(1, dtype=torch.int32, device=DEV)
        lut, d = torch.from_numpy(video.TURBO.copy()).to(DEV), _t(x)
        out = torch.zeros((H, W, 3), dtype=torch.uint8, device=DEV)
        _lib.check(lib.scg_viz_frame(None, d.data_ptr(), None, stats.data_ptr(), nan.data_ptr(), lut.data_ptr(), H, W, out.data_ptr(),
                                     None, None, None, None, torch.cuda.current_stream().cuda_stream), "scg_viz_frame")
        want = D.colorize(x, video.TURBO, st=st)
        assert np.array_equal(out.cpu().numpy(), want), st
    assert (want == video.TURBO[0]).all()


def _render_with_planted_values(H, W):
    ks = (np.arange(0, 256, dtype=f32) / f32(255)).astype(f32)
    vals = np.concatenate([ks, np.nextafter(ks, f32(2)), np.nextafter(ks, f32(-1)),
                           np.array([-0.0, -0.3, -1e30, 1.0000001, 1.7, 1e30, np.inf, -np.inf, np.nan, 1e-40], f32)])
    rng = np.random.default_rng(14)
    assert len(vals) <= H * W
    planes = vals[rng.integers(0, len(vals), (3, H * W))]
    for c in range(3):
        planes[c, :len(vals)] = np.roll(vals, 37 * c)
    return planes.reshape(3, H, W).astype(f32)


def _all_outputs(viz, depth, rng, render, skip=()):
    H, W = viz.H, viz.W
    outs = {k: torch.full((H, W) if k == "depth_u8" else (H, W, 3), 77, dtype=torch.uint8, device=DEV)
            for k in ("depth_color", "depth_color_bgr", "depth_u8", "render_u8", "frame_bgr") if k not in skip}
    got = viz.frame(depth, rng, render=render, **outs)
    if "depth_color" in skip:
        outs["depth_color"] = got
    return {k: v.cpu().numpy() for k, v in outs.items()}


def test_frame_outputs_video_bytes_and_evaluate_views_images():
    H, W = 31, 29                                             # 899 pixels: no multiple of four, interleaved rows at odd addresses
    render = _render_with_planted_values(H, W)
    rng = np.random.default_rng(15)
    depth = (1 + 5 * rng.random((H, W), dtype=f32)).astype(f32)
    viz = _viz(H, W)
    r = viz.depth_range(_t(depth))
    full = _all_outputs(viz, _t(depth), r, _t(render))
    x = D.normalised(depth)
    with np.errstate(all="ignore"):
        assert np.array_equal(full["frame_bgr"], D.video_frame(render))
        assert np.array_equal(full["render_u8"], D.render_u8(render))
    assert np.array_equal(full["depth_color"], D.colorize(x, video.TURBO))
    assert np.array_equal(full["depth_color_bgr"], full["depth_color"][..., ::-1])
    assert np.array_equal(full["depth_u8"], D.quantise(x))
    # rule 7 is not save_image's quantiser: the two differ wherever the fraction of r * 255 is at least one half
    assert (full["frame_bgr"][..., ::-1] != full["render_u8"]).any()
    ev = evaluate.evaluate_view(_t(render), _t(np.zeros_like(render)), _t(depth))
    assert np.array_equal(ev["renders"].cpu().numpy(), full["render_u8"]) and np.array_equal(ev["depth"].cpu().numpy(), full["depth_u8"])
    z = np.load(D.GOLDEN)
    g = z["frame_render"]
    gv = _viz(g.shape[1], g.shape[2])
    got = _all_outputs(gv, _t(np.zeros(g.shape[1:], f32)), None, _t(g))
    assert np.array_equal(got["frame_bgr"], z["frame_bgr"])
    # every optional output absent in turn: the others are the same bytes
    for skip in ("depth_color_bgr", "depth_u8", "render_u8", "frame_bgr", ("render_u8", "frame_bgr"), "depth_color"):
        skip = (skip,) if isinstance(skip, str) else skip
        part = _all_outputs(viz, _t(depth), r, _t(render), skip=skip)
        assert all(np.array_equal(part[k], full[k]) for k in part), skip
    no_render = viz.frame(_t(depth), r).cpu().numpy()
    assert np.array_equal(no_render, full["depth_color"])
    with pytest.raises(ValueError, match="need a render"):
        viz.frame(_t(depth), r, frame_bgr=torch.zeros((H, W, 3), dtype=torch.uint8, device=DEV))


@pytest.mark.parametrize("H,W", [(1, 1), (1, 2), (1, 3), (3, 3), (5, 7), (1, 1023), (1, 1025), (17, 65)])
def test_frame_tails_and_unaligned_outputs(H, W):
    rng = np.random.default_rng(H * 2000 + W)
    x = rng.random((H, W), dtype=f32)
    want = D.colorize(x, video.TURBO)
    viz = _viz(H, W)
    assert np.array_equal(viz.colorize(_t(x)).cpu().numpy(), want)
    for off in (1, 2, 3):
        buf = torch.full((H * W * 3 + 8,), 99, dtype=torch.uint8, device=DEV)
        out = buf[off:off + H * W * 3].view(H, W, 3)
        assert viz.colorize(_t(x), bgr=bool(off % 2), out=out) is out
        host = buf.cpu().numpy()
        assert np.array_equal(host[off:off + H * W * 3].reshape(H, W, 3), want[..., ::-1] if off % 2 else want)
        assert (host[:off] == 99).all() and (host[off + H * W * 3:] == 99).all()          # nothing written outside


def test_golden_cases_of_numpy_and_matplotlib():
    z = np.load(D.GOLDEN)
    for n in [str(n) for n in z["names"]]:
        x, p = z[f"{n}_x"], float(z[f"{n}_p"])
        got, _ = _select(x, p)
        assert D.same_stats(got[:2], [z[f"{n}_vmin"], z[f"{n}_vmax"]]), (n, got)
        assert np.array_equal(_colorize(x, p), z[f"{n}_rgb"]), n


def test_two_runs_are_bitwise_equal():
    rng = np.random.default_rng(16)
    H, W = 61, 2 * BLOCK // 61 + 5
    x = (np.floor(rng.random((H, W), dtype=f32) * 50) / 50).astype(f32)          # many ties: every workgroup adds to the same bins
    a, b = video.DepthColorizer(H, W), video.DepthColorizer(H, W)
    ia, ib = a.colorize(_t(x)), b.colorize(_t(x))
    ia2 = a.colorize(_t(x))
    assert torch.equal(ia, ib) and torch.equal(ia, ia2)
    assert torch.equal(a._stats.view(torch.int32), b._stats.view(torch.int32))


def test_colorize_is_captured_and_replayed():
    """The capture itself proves that colorize reads nothing on the host: a synchronising call inside it would fail."""
    H, W = 45, 2 * BLOCK // 45 + 3
    rng = np.random.default_rng(17)
    d0 = _t((1 + 4 * rng.random((H, W), dtype=f32)).astype(f32))
    d1 = (3 + 9 * rng.random((H, W), dtype=f32) ** 3).astype(f32)
    viz = video.DepthColorizer(H, W)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        viz.colorize_depth(d0)                                # warm: library loaded, allocator primed
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = viz.colorize_depth(d0)
    d0.copy_(_t(d1))
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), D.colorize(D.normalised(d1), video.TURBO))
    assert float(viz.vmin) == 0.0 and D.same_stats([float(viz.vmax)], [D.stats(D.normalised(d1))[1]])


def _scene(W=56, H=40, n_views=3):
    sc = syn.make_scene(1500, W, H, seed=5)
    model = syn.make_raw_model(sc).to(DEV)
    model.active_sh_degree = 3
    bg = torch.zeros(3, device=DEV)
    pipe = rmod.PipelineParams()
    views = []
    for i, yaw in enumerate((0.0, 8.0, -6.0)[:n_views]):
        cam = syn.orbit_camera(W, H, yaw, -2.0, 7.0).to(DEV)
        gt = torch.rand(3, H, W, device=DEV, generator=torch.Generator(DEV).manual_seed(i))
        views.append(types.SimpleNamespace(**cam._asdict(), original_image=gt, idx=i))
    return views, model, pipe, bg


def test_render_video_end_to_end(tmp_path, monkeypatch):
    from PIL import Image
    views, model, pipe, bg = _scene()
    H, W = 40, 56
    with torch.no_grad():
        pkgs = [rmod.render(v, model, pipe, bg) for v in views]
    frames, depths = [], []
    out = video.render_video(views, model, pipe, bg, out_dir=str(tmp_path), name="video", iteration=7, frame_sink=frames.append,
                             depth_sink=depths.append)
    assert set(out) == set(video.VIDEO_KEYS)
    assert all(out[k].shape == ((3, H, W) if k == "depth" else (3, H, W, 3)) and out[k].dtype == np.uint8 for k in out)
    base = tmp_path / "video" / "ours_7"
    for i in range(3):
        render, depth = pkgs[i]["render"].cpu().numpy(), pkgs[i]["rendered_depth"].cpu().numpy()[0]
        x = D.normalised(depth)
        assert np.array_equal(out["renders"][i], D.render_u8(render)) and np.array_equal(out["frames_bgr"][i], D.video_frame(render))
        assert np.array_equal(out["depth"][i], D.quantise(x)) and np.array_equal(out["depth_color"][i], D.colorize(x, video.TURBO))
        assert np.array_equal(out["depth_frames_bgr"][i], out["depth_color"][i][..., ::-1])
        assert out["depth_color"][i].any() and len(np.unique(out["depth_color"][i].reshape(-1, 3), axis=0)) > 20
        assert np.array_equal(np.array(Image.open(base / "renders" / f"{i:05d}.png")), out["renders"][i])
        assert np.array_equal(np.array(Image.open(base / "depth" / f"{i:05d}.png")), np.repeat(out["depth"][i][:, :, None], 3, axis=2))
        assert np.array_equal(np.array(Image.open(base / "depth" / f"color_{i:05d}.png")), out["depth_color"][i])
        assert np.array_equal(frames[i], out["frames_bgr"][i]) and np.array_equal(depths[i], out["depth_frames_bgr"][i])
    assert len(frames) == len(depths) == 3
    assert sorted(p.name for p in (base / "depth").iterdir()) == sorted([f"{i:05d}.png" for i in range(3)] + [f"color_{i:05d}.png" for i in range(3)])
    # one host read for the whole video: with the rasteriser's own reads out of the way (the frames pre-rendered), every way a
    # tensor reaches the host is counted
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
    again = video.render_video(views, model, pipe, bg, render=lambda v, g, p, b: pkgs[v.idx])
    monkeypatch.undo()
    assert reads == ["cpu"], reads
    assert all(np.array_equal(again[k], out[k]) for k in out)
    views[1].image_width = W + 1
    with pytest.raises(ValueError, match="one size"):
        video.render_video(views, model, pipe, bg)


def test_render_set_color_depth(tmp_path):
    from PIL import Image
    views, model, pipe, bg = _scene(n_views=2)
    full, per_view, images = evaluate.render_set(views, model, pipe, bg, out_dir=str(tmp_path / "a"), iteration=7, color_depth=True)
    full_b, per_view_b, images_b = evaluate.render_set(views, model, pipe, bg, out_dir=str(tmp_path / "b"), iteration=7)
    assert full == full_b and per_view == per_view_b
    files = lambda root: sorted(str(p.relative_to(root)) for p in root.rglob("*.png"))          # noqa: E731
    extra = sorted(f"test/ours_7/depth/color_{i:05d}.png" for i in range(2))
    assert files(tmp_path / "a") == sorted(files(tmp_path / "b") + extra) and len(files(tmp_path / "b")) == 8
    for i, (im, im_b) in enumerate(zip(images, images_b)):
        assert set(im) == set(im_b) | {"depth_color"} and set(im_b) == {"renders", "gt", "depth", "error_map", "dtumask"}
        assert all(im_b[k] is None or torch.equal(im[k], im_b[k]) for k in im_b)
        with torch.no_grad():
            depth = rmod.render(views[i], model, pipe, bg)["rendered_depth"]
        want = video.colorize_depth(depth).cpu().numpy()
        assert np.array_equal(im["depth_color"].cpu().numpy(), want) and want.any()
        assert np.array_equal(want, D.colorize(D.normalised(depth.cpu().numpy()[0]), video.TURBO))
        assert np.array_equal(np.array(Image.open(tmp_path / "a" / "test" / "ours_7" / "depth" / f"color_{i:05d}.png")), want)

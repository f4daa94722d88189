"""The camera images' resize on the GPU (scgaussian_amd/images.py, csrc/resample.hip) against the numpy restatement of
tests/resize_refs.py (held to Pillow itself by tests/test_resize_cpu.py) and against the fixture recorded from the reference's
PILtoTorch.  Every comparison is bit for bit: output bytes, and the bit patterns of the float image.

Sizes come from the kernels' own tiles.  The horizontal pass gives a workgroup a strip of S = images.STRIP output columns over
R = images.STRIP_ROWS source rows and stages them a chunk of rows at a time (fewer than R when a row's span is long: near the
ksize limit); the vertical pass gives a workgroup V = images.VTILE bytes of ONE output row, 4 per lane, so its only tile is
along the row.  Source widths 1, 2, 3, 5, 17 and 403 over an odd number of rows put a row start and a row tail at every byte phase
on the source, the intermediate and the output."""
import os
import types

import numpy as np
import pytest
import torch

import mono_refs as MR
import resize_refs as R
from scgaussian_amd import _lib, images, mono

pytestmark = pytest.mark.gpu
DEV = "cuda"
S, ROWS, V = images.STRIP, images.STRIP_ROWS, images.VTILE
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_resize.npz")
_MAKE = {"random": R.random_image, "step": R.step_image, "checker": R.checker_image}
_CACHE = {}


def _case(kind, win, hin, c, size):
    """(source, resized bytes, float image) of a case: computed once, shared, read-only."""
    key = (kind, win, hin, c, tuple(size))
    if key not in _CACHE:
        src = _MAKE[kind](hin, win, c)
        want = R.resize(src, size)
        fl = R.float_image(want)
        for a in (src, want, fl):
            a.setflags(write=False)
        _CACHE[key] = (src, want, fl)
    return _CACHE[key]


def _bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


def _run(src, size, want, fl, device_source=False):
    given = torch.from_numpy(np.array(src)).to(DEV) if device_source else src
    c = 1 if src.ndim == 2 else src.shape[2]
    out_float = torch.full((c, size[1], size[0]), -1.0, dtype=torch.float32, device=DEV)
    got = images.resize_u8(given, size, out_float=out_float)
    assert got.is_cuda and got.dtype == torch.uint8 and tuple(got.shape) == want.shape
    g = got.cpu().numpy()
    assert np.array_equal(g, want), ("bytes", np.argwhere(g != want)[:5], g[g != want][:5], want[g != want][:5])
    assert np.array_equal(_bits(out_float), fl.view(np.uint32)), "float image"


def _check(kind, win, hin, c, size):
    src, want, fl = _case(kind, win, hin, c, size)
    _run(src, size, want, fl)
    _run(src, size, want, fl, device_source=True)


def _id(v):
    return "-".join(str(x) for x in v) if isinstance(v, tuple) else str(v)


# ---- 1. the tiles ---------------------------------------------------------------------------------------------------------------
# (win, hin, wout, hout): output widths S - 1, S, S + 1, 2 S + 1 and source rows R - 1, R, R + 1, 2 R + 1 of the horizontal pass,
# at a non-integer reduction; the width alone, and both axes
STRIPS = [(131, ROWS - 1, S - 1, ROWS - 1), (131, ROWS, S, 20), (131, ROWS + 1, S + 1, ROWS + 1), (150, 2 * ROWS + 1, 2 * S + 1, 40),
          (70, 9, S, 9), (75, 5, 2 * S + 1, 3)]


@pytest.mark.parametrize("c", [0, 3], ids=["L", "RGB"])
@pytest.mark.parametrize("sizes", STRIPS, ids=_id)
def test_horizontal_strips_and_row_blocks(sizes, c):
    win, hin, wout, hout = sizes
    _check("random", win, hin, c, (wout, hout))


# the vertical pass: output rows of V - 1, V, V + 1 and 2 V + 1 bytes (L), and of the nearest multiples of 3 (RGB: 1023, 1026, 2049
# bytes and 1020, the one that is whole dwords), the height alone changing; and with the width changing in front of it
@pytest.mark.parametrize("w, c", [(V - 1, 0), (V, 0), (V + 1, 0), (2 * V + 1, 0), (341, 3), (342, 3), (683, 3), (340, 3)], ids=_id)
def test_vertical_row_tiles(w, c):
    _check("random", w, 9, c, (w, 4))


def test_vertical_row_tiles_behind_the_horizontal_pass():
    _check("random", 2 * V + 40, 5, 0, (V + 1, 3))
    _check("random", 700, 5, 3, (342, 3))


# ---- 2. byte phases -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [0, 3], ids=["L", "RGB"])
@pytest.mark.parametrize("win, wout", [(1, 3), (2, 5), (3, 2), (5, 3), (17, 6), (403, 50)], ids=_id)
def test_source_widths_at_every_byte_phase(win, wout, c):
    _check("random", win, 7, c, (wout, 5))              # both passes
    _check("random", win, 7, c, (wout, 7))              # the width alone
    _check("random", win, 7, c, (win, 3))               # the height alone: the vertical pass reads the tight source


def test_device_source_at_an_odd_address():
    """A view that starts 1, 2 and 3 bytes into an allocation: the horizontal pass reads the aligned dwords around its rows, the
    vertical pass alone falls back to byte reads."""
    for shift in (1, 2, 3):
        for (win, hin, c, size) in ((40, 9, 3, (13, 4)), (40, 9, 3, (40, 4)), (37, 5, 0, (9, 5)), (36, 6, 0, (36, 6))):
            src, want, _fl = _case("random", win, hin, c, size)
            buf = torch.zeros(src.size + 8, dtype=torch.uint8, device=DEV)
            buf[shift:shift + src.size] = torch.from_numpy(np.array(src)).reshape(-1).to(DEV)
            view = buf[shift:shift + src.size].view(src.shape)
            assert view.data_ptr() % 4 == shift
            assert np.array_equal(images.resize_u8(view, size).cpu().numpy(), want), (shift, win, hin, c, size)


# ---- 3. size relations, clipped windows, both clamps ---------------------------------------------------------------------------
@pytest.mark.parametrize("c", [0, 3], ids=["L", "RGB"])
@pytest.mark.parametrize("sizes", [(40, 30, 40, 30), (7, 5, 20, 9), (1, 1, 3, 2), (5, 1, 2, 1), (1, 5, 1, 2), (2, 2, 5, 5),
                                   (32, 20, 1, 1), (21, 9, 8, 20), (64, 48, 16, 12)], ids=_id)
def test_copy_upscale_mixed_and_smallest(sizes, c):
    win, hin, wout, hout = sizes
    _check("random", win, hin, c, (wout, hout))


def test_windows_are_clipped_at_both_ends_of_both_axes():
    for in_size, out_size in ((64, 8), (48, 6), (7, 20), (5, 9)):
        bounds, _k = R.coefficients(in_size, out_size)
        full = R.ksize_of(in_size, out_size) - 2
        assert bounds[0, 0] == 0 and bounds[0, 1] < full and bounds[-1, 0] + bounds[-1, 1] == in_size and bounds[-1, 1] < full
    _check("random", 64, 48, 3, (8, 6))
    _check("random", 7, 5, 3, (20, 9))


@pytest.mark.parametrize("c", [0, 3], ids=["L", "RGB"])
@pytest.mark.parametrize("kind", ["step", "checker"])
def test_step_and_checkerboard_at_8x_hit_both_clamps(kind, c):
    src, want, _fl = _case(kind, 64, 48, c, (8, 6))
    assert (want == 0).any() and (want == 255).any()
    # a negative accumulator (shifted: -1 or below, stored: 0) and one above 255 << 22, in the first pass
    plane = (src if c == 0 else src[:, :, 0]).astype(np.int64)
    bounds, k = R.coefficients(64, 8)
    acc = np.array([[(1 << 21) + int((plane[y, f:f + n] * k[i, :n]).sum()) for i, (f, n) in enumerate(bounds)] for y in range(48)])
    assert (acc < 0).any() and ((acc >> 22) > 255).any()
    _check(kind, 64, 48, c, (8, 6))


def test_float_image_of_all_256_bytes():
    u8 = np.arange(256, dtype=np.uint8).reshape(16, 16)
    want = torch.from_numpy(u8) / 255.0
    for src in (u8, torch.from_numpy(u8).to(DEV)):
        fl = torch.empty((1, 16, 16), dtype=torch.float32, device=DEV)
        got = images.resize_u8(src, (16, 16), out_float=fl)
        assert np.array_equal(got.cpu().numpy(), u8) and np.array_equal(_bits(fl[0]), want.numpy().view(np.uint32))
    rgb = np.stack((u8, u8[::-1], u8.T), axis=2)
    got, fl = images.resize_batch(rgb[None], (16, 16), want_float=True)
    assert np.array_equal(got[0].cpu().numpy(), rgb)
    assert np.array_equal(_bits(fl[0]), (torch.from_numpy(rgb) / 255.0).permute(2, 0, 1).contiguous().numpy().view(np.uint32))


# ---- 4. ksize limits ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [0, 3], ids=["L", "RGB"])
def test_at_the_ksize_limit(c):
    """32x: ksize 129, the widest strip a workgroup stages: its 32 rows go through LDS in two chunks of 16 (L) and four of 8 (RGB),
    the lanes' four-row sweep partly idle; 65 rows are two workgroups and a row."""
    assert R.ksize_of(1280, 40) == images.MAX_KSIZE == R.ksize_of(64, 2)
    _check("random", 1280, 65, c, (40, 3))
    _check("random", 3, 64, c, (3, 2))


def test_beyond_the_ksize_limit_takes_the_host_route_and_gives_the_same_bytes():
    for (win, hin, size) in ((66, 3, (2, 3)), (3, 66, (3, 2))):
        plan = images.plan_of((win, hin), size, 3)
        assert not plan.device_route and max(plan.hksize, plan.vksize) == 133 and plan.tables.size == 0
        src, want, fl = _case("random", win, hin, 3, size)
        _run(src, size, want, fl)
        with pytest.raises(_lib.ScgError, match="beyond the kernels"):
            images.resize_u8(torch.from_numpy(np.array(src)).to(DEV), size)


# ---- 5. batches and the realistic size --------------------------------------------------------------------------------------------
def test_batch_of_three_in_one_call_and_in_two_chunks():
    size = (13, 9)
    srcs = [R.random_image(21, 37, 3, seed=s) for s in (1, 2, 3)]
    singles = [images.resize_u8(s, size) for s in srcs]
    for s, one in zip(srcs, singles):
        assert np.array_equal(one.cpu().numpy(), R.resize(s, size))
    plan = images.plan_of((37, 21), size, 3)
    whole, fl = images.resize_batch(srcs, size, want_float=True)
    two = images.resize_batch(srcs, size, max_staged_bytes=2 * plan.image_bytes + plan.tables.size + 10)
    stacked = images.resize_batch(torch.from_numpy(np.stack(srcs)).to(DEV), size)
    assert tuple(whole.shape) == (3, 9, 13, 3) and tuple(fl.shape) == (3, 3, 9, 13)
    for i, one in enumerate(singles):
        assert torch.equal(whole[i], one) and torch.equal(two[i], one) and torch.equal(stacked[i], one), i
        assert np.array_equal(_bits(fl[i]), R.float_image(one.cpu().numpy()).view(np.uint32))


def test_realistic_eighth():
    """378 x 504 -> 47 x 63, the benchmark's image at an eighth."""
    _check("random", 504, 378, 3, (63, 47))
    _check("step", 504, 378, 3, (63, 47))


# ---- 6. PILtoTorch ----------------------------------------------------------------------------------------------------------------
def _host_pil_to_torch(pil_image, resolution):
    """What PILtoTorch computes (utils/general_utils.py:22-28), stated here: Pillow's resize, / 255.0, channels first."""
    t = torch.from_numpy(np.array(pil_image.resize(resolution))) / 255.0
    return t.permute(2, 0, 1) if t.dim() == 3 else t.unsqueeze(-1).permute(2, 0, 1)


def test_pil_to_torch_against_the_reference_fixture():
    Image = pytest.importorskip("PIL.Image")
    z = np.load(GOLDEN)
    for name in (str(n) for n in z["names"]):
        src, res, want = z[name + "_src"], tuple(int(v) for v in z[name + "_res"]), z[name + "_out"]
        got = images.pil_to_torch(Image.fromarray(src), res)
        assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == want.shape, name
        assert np.array_equal(_bits(got), want.view(np.uint32)), name
        u8 = images.resize_u8(src, res).cpu().numpy()
        assert np.array_equal(R.float_image(u8).view(np.uint32), want.view(np.uint32)), name


def test_pil_to_torch_other_modes_take_the_host_route_and_install():
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(4)
    rgba = Image.fromarray(rng.integers(0, 256, (24, 32, 4), dtype=np.uint8), "RGBA")
    pal = Image.fromarray(rng.integers(0, 256, (24, 32, 3), dtype=np.uint8)).convert("P")
    rgb = Image.fromarray(rng.integers(0, 256, (24, 32, 3), dtype=np.uint8))
    assert (rgba.mode, pal.mode) == ("RGBA", "P")
    for img, channels in ((rgba, 4), (pal, 1), (rgb, 3)):
        got = images.pil_to_torch(img, (8, 6))
        want = _host_pil_to_torch(img, (8, 6))
        assert got.is_cuda and tuple(got.shape) == (channels, 6, 8) and torch.equal(got.cpu(), want.contiguous()), img.mode
    mod = types.SimpleNamespace(PILtoTorch=_host_pil_to_torch)
    assert images.install(mod) is _host_pil_to_torch and mod.PILtoTorch is images.pil_to_torch
    assert torch.equal(mod.PILtoTorch(rgb, (8, 6)).cpu(), _host_pil_to_torch(rgb, (8, 6)).contiguous())


# ---- 7. the hand-over to the scene setup -------------------------------------------------------------------------------------------
def test_resized_bytes_are_what_mono_setup_takes():
    rng = np.random.default_rng(9)
    H, W = 48, 64
    cams = MR.cameras([(H, W)] * 3, rng)
    big = [R.random_image(2 * H + 1, 2 * W + 3, 3, seed=20 + i) for i in range(3)]
    u8, fl = images.resize_batch(big, (W, H), want_float=True)
    for i, cam in enumerate(cams):
        cam.image = u8[i].cpu().numpy()
        assert np.array_equal(cam.image, R.resize(big[i], (W, H)))
    md = MR.match_data(cams, 5, rng, lo=0.1, hi=0.9)
    setup = mono.MonoSetup.build(cams, md, DEV, np.zeros(3 * 2 * 5, dtype=np.float32))
    for i, k in enumerate(setup.keys):
        got = setup.view_gs[k]["image_color"].reshape(H, W, 3)
        assert np.array_equal(_bits(got), _bits(fl[i].permute(1, 2, 0).contiguous())), k


# ---- 8. determinism, graph replay, host reads -----------------------------------------------------------------------------------
def test_two_runs_give_equal_bytes():
    src, want, _fl = _case("random", 403, 7, 3, (50, 5))
    a, b = images.resize_u8(src, (50, 5)), images.resize_u8(src, (50, 5))
    assert a.data_ptr() != b.data_ptr() and torch.equal(a, b) and np.array_equal(a.cpu().numpy(), want)


def test_launches_go_to_the_given_stream():
    src, want, fl = _case("random", 403, 7, 3, (50, 5))
    side = torch.cuda.Stream()
    for given in (src, torch.from_numpy(np.array(src)).to(DEV)):
        torch.cuda.synchronize()
        out_float = torch.empty((3, 5, 50), dtype=torch.float32, device=DEV)
        got = images.resize_u8(given, (50, 5), out_float=out_float, stream=side)
        side.synchronize()
        assert np.array_equal(got.cpu().numpy(), want) and np.array_equal(_bits(out_float), fl.view(np.uint32))


def test_device_source_in_a_graph_replays_on_rewritten_bytes():
    size = (S + 1, 20)
    src0, _w0, _f0 = _case("random", 131, ROWS + 1, 3, size)
    src1 = R.random_image(ROWS + 1, 131, 3, seed=5)
    dev_src = torch.from_numpy(np.array(src0)).to(DEV)
    images.resize_u8(dev_src, size)                                # the tables of this size are on the device from here on
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fl = torch.empty((3, size[1], size[0]), dtype=torch.float32, device=DEV)
        out = images.resize_u8(dev_src, size, out_float=fl)
    dev_src.copy_(torch.from_numpy(src1).to(DEV))
    graph.replay()
    torch.cuda.synchronize()
    want = R.resize(src1, size)
    assert np.array_equal(out.cpu().numpy(), want) and np.array_equal(_bits(fl), R.float_image(want).view(np.uint32))


def test_device_source_makes_no_host_read(monkeypatch):
    size = (50, 5)
    src, want, _fl = _case("random", 403, 7, 3, size)
    dev_src = torch.from_numpy(np.array(src)).to(DEV)
    images.resize_u8(dev_src, size)
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
    fl = torch.empty((3, 5, 50), dtype=torch.float32, device=DEV)
    got = images.resize_u8(dev_src, size, out_float=fl)
    batch = images.resize_batch(dev_src[None], size)
    monkeypatch.undo()
    assert reads == [], reads
    assert np.array_equal(got.cpu().numpy(), want) and np.array_equal(batch[0].cpu().numpy(), want)

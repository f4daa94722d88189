"""The test-set evaluation on the GPU (scgaussian_amd/evaluate.py, csrc/evalview.hip) against the plain-torch restatements of
tests/eval_refs.py and the numbers the reference's own get_pixel_loss / ssim / psnr produced (tests/golden/ref_eval.npz).

Bit for bit: everything that is a chain of separately rounded fp32 operations or an integer — the five quantised images, the masked
images, S and K.
error_f32: max |kernel - fp64| <= max(4 * e_ref, 1e-6), e_ref the deviation of the reference's own fp32 evaluation from its fp64 one
on the same input (from the golden for its cases, from the fp32 restatement otherwise); the 4 covers another summation order of the
25 taps at the same precision.  Measured on an MI355X: see the README section "Test-set evaluation".
PSNR: 1e-3 dB against the reference (fl(q / 255) carries 3e-8 per operand against a smallest difference of 1 / 255: at most 3e-5
relative in the mse, 1.3e-4 dB; the rest is margin).  SSIM: the 2e-6 at which tests/test_image_loss.py holds the same kernel.

Shapes come from the view kernel's tile (scg_eval_view_tile): reflection at both borders inside one tile, a halo that crosses a tile
edge, widths that are no multiple of 4 (unaligned byte stores).  The kernel refuses sides below 3, as ReflectionPad2d(2) does, so the
S / K sweep starts at 3 and sides 1 and 2 are checked to be refused."""
import math
import os
import types

import numpy as np
import pytest
import torch

import eval_refs as ER
from scgaussian_amd import _lib, evaluate
from scgaussian_amd import render as rmod
from scgaussian_amd import synthetic as syn

pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_eval.npz")
TW, TH = _lib.load().scg_eval_view_tile(0), _lib.load().scg_eval_view_tile(1)
HEIGHTS = sorted({3, 4, 5, TH - 1, TH, TH + 1, TH + 2, 2 * TH + 1})
WIDTHS = sorted({3, 4, 5, TW - 1, TW, TW + 1, TW + 2, 2 * TW + 1})
PSNR_TOL, SSIM_TOL, ERR_FLOOR, FACTOR = 1e-3, 2e-6, 1e-6, 4.0
U8_KEYS = ("renders", "gt", "depth", "dtumask")


def _mask(H, W, seed):
    """zeros, ones and values in between: about a third each"""
    m = torch.rand(H, W, generator=torch.Generator().manual_seed(seed))
    return torch.where(m < 0.3, torch.zeros(()), torch.where(m > 0.6, torch.ones(()), m))


def _run(render, gt, depth, mask=None, record=None):
    out = evaluate.evaluate_view(render.to(DEV), gt.to(DEV), depth.to(DEV), None if mask is None else mask.to(DEV), record)
    torch.cuda.synchronize()
    rec = out["record"].cpu()
    out["S"], out["K"] = int(rec[0]), int(rec[1])
    out["ssim"] = float(rec[2:3].view(torch.float32)[1]) / out["renders_masked"].numel()
    out["psnr"] = evaluate.psnr_from_sums(out["S"], out["K"])
    return out


def _check_exact(out, ref, what):
    for k in U8_KEYS:
        if ref[k] is None:
            assert out[k] is None, (what, k)
        else:
            assert out[k].dtype == torch.uint8 and torch.equal(out[k].cpu(), ref[k]), (what, k)
    assert torch.equal(out["error_map"], ER.quantise(out["error_map_f32"]).to(DEV)), (what, "error_u8 is q(error_f32)")
    assert torch.equal(out["renders_masked"].cpu(), ref["renders_masked"]) and torch.equal(out["gt_masked"].cpu(), ref["gt_masked"]), what
    assert (out["S"], out["K"]) == (ref["S"], ref["K"]), what


def _check_error(out, render, gt, what, e_ref=None, err64=None):
    if err64 is None:
        err64 = ER.pixel_loss_ref(render, gt, torch.float64)
    if e_ref is None:
        e_ref = float((ER.pixel_loss_ref(render, gt, torch.float32).double() - err64).abs().max())
    dev = float((out["error_map_f32"].cpu().double() - err64).abs().max())
    bar = max(FACTOR * e_ref, ERR_FLOOR)
    print(f"EVAL {what}: error map |kernel - fp64| {dev:.3e}  e_ref {e_ref:.3e}  bar {bar:.3e}")
    assert math.isfinite(dev) and dev <= bar, (what, dev, e_ref, bar)
    return dev


def _check_metrics(out, ref64, what):
    print(f"EVAL {what}: psnr {out['psnr']:.6f} ref {ref64['psnr']:.6f}  ssim {out['ssim']:.8f} ref {ref64['ssim']:.8f}")
    if math.isfinite(ref64["psnr"]):
        assert abs(out["psnr"] - ref64["psnr"]) <= PSNR_TOL, what
    assert abs(out["ssim"] - ref64["ssim"]) <= SSIM_TOL, what


@pytest.mark.parametrize("H", HEIGHTS)
def test_every_output_at_the_tile_edges(H):
    for W in WIDTHS:
        render, gt, depth = ER.images(H, W, seed=100 * H + W, outside=(W % 2 == 1))
        for mask in (None, _mask(H, W, 7 * H + W)):
            what = f"{H}x{W} {'masked' if mask is not None else 'plain'}"
            out = _run(render, gt, depth, mask)
            ref = ER.view_ref(render, gt, depth, mask, torch.float32)
            _check_exact(out, ref, what)
            _check_error(out, render, gt, what)
            ref64 = ER.view_ref(render, gt, depth, mask, torch.float64)
            if ref64["K"]:
                _check_metrics(out, ref64, what)
            else:
                assert math.isnan(out["psnr"])


@pytest.mark.parametrize("name", ["plain", "binary", "fractional", "outside"])
def test_golden_cases_of_the_reference(name):
    z = np.load(GOLDEN)
    t = lambda k: torch.from_numpy(z[f"{name}_{k}"])          # noqa: E731
    render, gt, depth = t("render"), t("gt"), t("depth")
    mask = t("mask") if f"{name}_mask" in z.files else None
    out = _run(render, gt, depth, mask)
    _check_exact(out, ER.view_ref(render, gt, depth, mask, torch.float32), name)
    _check_error(out, render, gt, f"golden {name}", e_ref=float(z[f"{name}_e_ref"]), err64=t("error_64"))
    assert (out["S"], out["K"]) == (int(z[f"{name}_S"]), int(z[f"{name}_K"]))
    _check_metrics(out, dict(psnr=float(z[f"{name}_psnr_64"]), ssim=float(z[f"{name}_ssim_64"])), f"golden {name}")


def test_quantiser_on_planted_values():
    f32 = np.float32
    base = np.array([(k + h) / 255 for k in range(256) for h in (0.0, 0.5)], dtype=f32)
    vals = np.concatenate([base, np.nextafter(base, f32(np.inf)), np.nextafter(base, f32(-np.inf)), -base, base + f32(1),
                           np.array([-0.0, np.inf, -np.inf, np.nan, 1e30, -1e30, 1e-40, -1e-40], dtype=f32)])
    H, W = 5 * TH + 1, 2 * TW + 1
    n = 3 * H * W
    assert len(vals) <= H * W
    g = torch.Generator().manual_seed(5)
    planes = torch.from_numpy(vals)[torch.randint(0, len(vals), (3, n), generator=g)]
    for p in planes:
        p[:len(vals)] = torch.from_numpy(vals)               # every planted value at least once in each input
    render, gt, mask = planes[0].reshape(3, H, W), planes[1].reshape(3, H, W), planes[2][:H * W].reshape(H, W)
    out = _run(render, gt, torch.rand(1, H, W), mask)
    ref = ER.view_ref(render, gt, torch.rand(1, H, W), mask, torch.float32)
    for k in ("renders", "gt", "dtumask"):
        assert torch.equal(out[k].cpu(), ref[k]), k
    assert int(ER.quantise(torch.tensor([float("nan")]))[0]) == 0 and bool(torch.isnan(render).any())
    assert torch.equal(out["renders_masked"].cpu(), ref["renders_masked"]) and (out["S"], out["K"]) == (ref["S"], ref["K"])


def test_depth_edge_cases():
    H, W = 2 * TH + 1, 2 * TW + 1
    render, gt, depth = ER.images(H, W, seed=9)
    const = _run(render, gt, torch.full((1, H, W), 2.5))
    assert int(const["depth"].max()) == 0                    # max == min: NaN, a zero image
    with_nan = depth.clone()
    with_nan[0, TH + 1, TW + 3] = float("nan")
    assert int(_run(render, gt, with_nan)["depth"].max()) == 0          # min and max are NaN, as torch's
    far = depth.clone()
    far[0, 0, 0], far[0, H - 1, W - 1] = 0.25, 9.0           # min and max in different tiles
    out = _run(render, gt, far)
    want = ER.quantise(ER.normalised_depth(far[0]))
    assert torch.equal(out["depth"].cpu(), want) and int(want[0, 0]) == 0 and int(want[-1, -1]) == 255
    # a larger plane: many workgroups of the range kernel, the extremes in its last partly filled chunk
    big = torch.rand(1, 131, 97, generator=torch.Generator().manual_seed(1)) * 3 + 1
    big[0, 130, 90], big[0, 130, 96] = -2.0, 11.0
    r2, g2, _ = ER.images(131, 97, seed=10)
    assert torch.equal(_run(r2, g2, big)["depth"].cpu(), ER.quantise(ER.normalised_depth(big[0])))


def test_error_map_planted_cases():
    H, W = TH + 2, TW + 2
    _, gt, depth = ER.images(H, W, seed=11)
    same = _run(gt, gt, depth)
    assert float(same["error_map_f32"].abs().max()) == 0.0 and int(same["error_map"].max()) == 0 and same["S"] == 0
    assert same["psnr"] == float("inf") and abs(same["ssim"] - 1.0) <= SSIM_TOL
    flat_r, flat_g = torch.full((3, H, W), 0.3), torch.full((3, H, W), 0.6)
    _check_error(_run(flat_r, flat_g, depth), flat_r, flat_g, "flat images")
    for corner in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)):
        spike = torch.zeros(3, H, W)
        spike[:, corner[0], corner[1]] = 1.0                 # the corner pixel: not duplicated; its neighbours are reflected twice
        out = _run(spike, torch.zeros(3, H, W), depth)
        _check_error(out, spike, torch.zeros(3, H, W), f"bright corner {corner}")
        assert float(out["error_map_f32"][corner]) > 0.5


def test_sums_under_the_psnr_are_exact():
    cases = [(h, w) for h in (3, TH, 2 * TH + 1) for w in (3, TW, 2 * TW + 1)] + [(300, 400)]
    for H, W in cases:
        render, gt, depth = ER.images(H, W, seed=H + W, spread=0.3, outside=True)
        q_r, q_g = ER.np_u8(ER.quantise(render)).astype(np.int64), ER.np_u8(ER.quantise(gt)).astype(np.int64)
        sq = ((q_r - q_g) ** 2).sum(axis=0)
        m = _mask(H, W, H * W)
        q_m = ER.np_u8(ER.quantise(m))
        masks = {"none": (None, np.ones((H, W), bool)), "mixed": (m, q_m == 255), "zeros": (torch.zeros(H, W), np.zeros((H, W), bool)),
                 "254": (torch.full((H, W), 254 / 255), np.zeros((H, W), bool))}
        assert int(ER.quantise(torch.tensor([254 / 255]))[0]) == 254
        for name, (mask, sel) in masks.items():
            out = _run(render, gt, depth, mask)
            assert (out["S"], out["K"]) == (int(sq[sel].sum()), 3 * int(sel.sum())), (H, W, name)
            if not sel.any():
                assert math.isnan(out["psnr"])
        same = _run(gt, gt, depth, m)
        assert same["S"] == 0 and same["K"] == 3 * int((q_m == 255).sum()) and same["psnr"] == float("inf")
    # ReflectionPad2d(2) refuses sides below 3, and so does the kernel
    for H, W in ((1, 8), (2, 8), (8, 1), (8, 2)):
        with pytest.raises(_lib.ScgError, match="3 x 3"):
            _run(*ER.images(H, W, seed=1))


def test_two_calls_are_bitwise_equal_and_a_set_equals_separate_calls():
    shapes = [(TH + 1, 2 * TW + 1), (2 * TH + 1, TW - 1), (5, 3)]
    views = [ER.images(H, W, seed=40 + i, outside=bool(i % 2)) + (_mask(H, W, i) if i != 1 else None,) for i, (H, W) in enumerate(shapes)]
    es = evaluate.EvalSet(3)
    for i, (r, g, d, m) in enumerate(views):
        a, b = _run(r, g, d, m), _run(r, g, d, m)
        for k, v in a.items():
            if isinstance(v, torch.Tensor):
                assert torch.equal(v.contiguous().view(torch.uint8), b[k].contiguous().view(torch.uint8)), k          # bits: a NaN equals itself
        c = es.add(f"{i:05d}.png", r.to(DEV), g.to(DEV), d.to(DEV), None if m is None else m.to(DEV))
        assert torch.equal(c["renders"], a["renders"]) and torch.equal(c["error_map_f32"], a["error_map_f32"])
        views[i] = a
    full, per_view = es.results()
    assert torch.equal(es.records.cpu(), torch.stack([v["record"].cpu() for v in views]))
    names = [f"{i:05d}.png" for i in range(3)]
    assert list(per_view["PSNR"]) == names == list(per_view["SSIM"]) and set(full) == {"SSIM", "PSNR"}
    for i, k in enumerate(names):
        assert per_view["PSNR"][k] == pytest.approx(views[i]["psnr"], abs=1e-5) and per_view["SSIM"][k] == pytest.approx(views[i]["ssim"], abs=1e-7)
    assert full["PSNR"] == torch.tensor([per_view["PSNR"][k] for k in names]).mean().item()
    # an lpips_fn is called per view on the masked images and its values join the one read
    es2 = evaluate.EvalSet(2, lpips_fn=lambda a, b: (a - b).abs().mean())
    for i in range(2):
        r, g, d = ER.images(*shapes[i], seed=40 + i, outside=bool(i % 2))
        es2.add(names[i], r.to(DEV), g.to(DEV), d.to(DEV))
    full2, pv2 = es2.results()
    for i in range(2):
        r, g, d = ER.images(*shapes[i], seed=40 + i, outside=bool(i % 2))
        ref = ER.view_ref(r, g, d, None, torch.float32)
        assert pv2["LPIPS"][names[i]] == pytest.approx(float((ref["renders_masked"] - ref["gt_masked"]).abs().mean()), abs=1e-6)
    assert full2["AVG"] == full2["LPIPS"] and set(pv2) == {"SSIM", "PSNR", "LPIPS", "AVG"}


def test_evaluate_view_is_captured_and_replayed():
    """The capture itself proves that evaluate_view reads nothing on the host: a synchronising call inside it would fail."""
    H, W = 2 * TH + 1, 2 * TW + 1
    r0, g0, d0 = (t.to(DEV) for t in ER.images(H, W, seed=60))
    m0 = _mask(H, W, 61).to(DEV)
    r1, g1, d1 = ER.images(H, W, seed=62, outside=True)
    m1 = _mask(H, W, 63)
    record = torch.zeros(evaluate.RECORD_WORDS, dtype=torch.int64, device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        evaluate.evaluate_view(r0, g0, d0, m0, record)         # warm: library loaded, allocator primed
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = evaluate.evaluate_view(r0, g0, d0, m0, record)
    for src, dst in ((r1, r0), (g1, g0), (d1, d0), (m1, m0)):
        dst.copy_(src.to(DEV))
    record.zero_()
    graph.replay()
    torch.cuda.synchronize()
    eager = _run(r1, g1, d1, m1)
    for k in ("renders", "gt", "depth", "error_map", "dtumask", "error_map_f32", "renders_masked", "gt_masked"):
        assert torch.equal(out[k], eager[k]), k
    assert torch.equal(record, eager["record"]) and eager["K"] > 0


def test_render_set_end_to_end(tmp_path):
    from PIL import Image
    P, W, H = 2000, 72, 52
    sc = syn.make_scene(P, W, H, seed=5)
    model = syn.make_raw_model(sc).to(DEV)
    model.active_sh_degree = 3
    bg = torch.zeros(3, device=DEV)
    pipe = rmod.PipelineParams()
    views = []
    for i, yaw in enumerate((0.0, 8.0, -6.0)):
        cam = syn.orbit_camera(W, H, yaw, -2.0, 7.0).to(DEV)
        with torch.no_grad():
            img = rmod.render(cam, model, pipe, bg)["render"]
        gt = (img + 0.05 * torch.randn(3, H, W, device=DEV, generator=torch.Generator(DEV).manual_seed(i))).clamp(0, 1)
        v = types.SimpleNamespace(**cam._asdict(), original_image=gt, dtumask=(_mask(H, W, i).to(DEV)[None] if i == 1 else None))
        views.append(v)
    full, per_view, images = evaluate.render_set(views, model, pipe, bg, out_dir=str(tmp_path), name="test", iteration=7)
    assert list(full) == list(per_view) == ["ours_7"] and set(full["ours_7"]) == {"SSIM", "PSNR"} and len(images) == 3
    names = [f"{i:05d}.png" for i in range(3)]
    assert list(per_view["ours_7"]["PSNR"]) == names and list(per_view["ours_7"]["SSIM"]) == names
    base = tmp_path / "test" / "ours_7"
    for i, im in enumerate(images):
        for sub, key in zip(evaluate.SUBDIRS, ("renders", "gt", "depth", "error_map", "dtumask")):
            path = base / sub / names[i]
            if im[key] is None:
                assert key == "dtumask" and i != 1 and not path.exists()
                continue
            back = np.array(Image.open(path))
            want = im[key].cpu().numpy()
            assert back.shape == (H, W, 3) and back.dtype == np.uint8
            assert np.array_equal(back, want if want.ndim == 3 else np.repeat(want[:, :, None], 3, axis=2)), (i, key)
        # the numbers are those of the files: PSNR from what was written
        r, g = (np.array(Image.open(base / s / names[i])).astype(np.int64) for s in ("renders", "gt"))
        sel = np.ones((H, W), bool) if i != 1 else np.array(Image.open(base / "dtumask" / names[i]))[:, :, 0] == 255
        want_psnr = evaluate.psnr_from_sums(int(((r - g) ** 2)[sel].sum()), 3 * int(sel.sum()))
        assert per_view["ours_7"]["PSNR"][names[i]] == pytest.approx(want_psnr, abs=1e-4)
        assert 10 < want_psnr < 60 and 0.3 < per_view["ours_7"]["SSIM"][names[i]] <= 1.0
    evaluate.write_results(str(tmp_path), full, per_view)
    assert (tmp_path / "results.json").exists() and (tmp_path / "per_view.json").exists()
    # without out_dir: the same numbers, nothing written
    full_b, per_view_b, _ = evaluate.render_set(views, model, pipe, bg, iteration=7)
    assert full_b == full and per_view_b == per_view

"""CPU-side checks of the test-set evaluation (scgaussian_amd/evaluate.py, csrc/evalview.hip): the references the GPU tests lean on,
the host arithmetic of EvalSet.results, the ABI and the argument validation.  No kernel runs here.

What anchors what: eval_refs.pixel_loss_ref, ssim_ref and psnr_ref are pinned to numbers the reference's own get_pixel_loss, ssim
and psnr produced (tests/golden/ref_eval.npz, written by tests/golden/make_golden_eval.py).  torchvision is absent, so the quantiser
rests on its restatement, held here to planted values worked out by hand, and a PIL round trip shows that the PNG adds nothing."""
import io
import json
import math
import os

import numpy as np
import pytest
import torch

import abi_text
import eval_refs as ER
from scgaussian_amd import _lib, evaluate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "ref_eval.npz")
CASES = ("plain", "binary", "fractional", "outside")
NEW_SYMBOLS = ("scg_eval_depth_range_scratch_bytes", "scg_eval_depth_range", "scg_eval_view_tile", "scg_eval_view")


def _case(z, name):
    t = lambda k: torch.from_numpy(z[f"{name}_{k}"])          # noqa: E731
    return t("render"), t("gt"), t("depth"), (t("mask") if f"{name}_mask" in z.files else None)


@pytest.mark.parametrize("name", CASES)
def test_restatement_is_the_reference(name):
    z = np.load(GOLDEN)
    render, gt, depth, mask = _case(z, name)
    for tag, dtype, tol in (("64", torch.float64, 1e-14), ("32", torch.float32, 1e-6)):
        r = ER.view_ref(render, gt, depth, mask, dtype)
        assert np.abs(r["error_map_val"].double().numpy() - z[f"{name}_error_{tag}"]).max() <= tol
        assert abs(r["ssim"] - float(z[f"{name}_ssim_{tag}"])) <= tol
        assert abs(r["psnr"] - float(z[f"{name}_psnr_{tag}"])) <= tol * 100
        assert r["S"] == int(z[f"{name}_S"]) and r["K"] == int(z[f"{name}_K"])
        # the PSNR is a function of the two integers, up to the rounding of fl(q / 255) the reference carries: 3e-8 per operand
        # against a smallest difference of 1 / 255, 3e-5 relative in the mse at the most, 1.3e-4 dB
        assert abs(evaluate.psnr_from_sums(r["S"], r["K"]) - float(z[f"{name}_psnr_64"])) <= 1.3e-4
    assert 1e-8 < float(z[f"{name}_e_ref"]) < 1e-6
    assert ER.view_ref(render, gt, depth, mask, torch.float32)["error_map_val"].dtype == torch.float32


def test_the_golden_cases_bite():
    z = np.load(GOLDEN)
    assert float(z["outside_render"].min()) < -0.3 and float(z["outside_render"].max()) > 1.3
    m = z["fractional_mask"]
    assert ((m > 0) & (m < 1)).sum() > 100 and (m == 1).sum() * 3 == int(z["fractional_K"]) and (m == 0).sum() > 100
    assert int(z["plain_K"]) == 3 * 12 * 9 and set(np.unique(z["binary_mask"])) == {0.0, 1.0}
    assert 0 < int(z["binary_K"]) < 3 * 17 * 33


def test_quantiser_on_planted_values():
    f32 = np.float32
    up, down = lambda v: np.nextafter(f32(v), f32(np.inf)), lambda v: np.nextafter(f32(v), f32(-np.inf))          # noqa: E731
    q = lambda v: int(ER.quantise(torch.tensor([v], dtype=torch.float32))[0])          # noqa: E731
    assert [q(0.0), q(-0.0), q(1.0), q(0.5), q(-0.3), q(1.7), q(-1e30), q(1e30)] == [0, 0, 255, 128, 0, 255, 0, 255]
    assert q(float("inf")) == 255 and q(float("-inf")) == 0 and q(float("nan")) == 0
    for k in (0, 1, 2, 127, 128, 254, 255):
        assert q(f32(k) / f32(255)) == k and q(up(f32(k) / f32(255))) == k and q(down(f32(k) / f32(255))) == k
    # the restatement is the formula, operation by operation, in numpy's fp32
    vals = np.array([(k + h) / 255 for k in range(256) for h in (0.0, 0.5)], dtype=f32)
    vals = np.concatenate([vals, up(vals), down(vals), -vals, vals + f32(1)])
    want = np.trunc(np.clip((vals * f32(255)).astype(f32) + f32(0.5), 0, 255)).astype(np.uint8)
    assert np.array_equal(ER.quantise(torch.from_numpy(vals)).numpy(), want)
    assert len(set(want.tolist())) == 256


def test_png_round_trip_adds_nothing():
    from PIL import Image
    render, gt, depth = ER.images(19, 23, seed=3, outside=True)
    mask = (torch.rand(19, 23, generator=torch.Generator().manual_seed(4)) > 0.5).float()
    r = ER.view_ref(render, gt, depth, mask, torch.float32)

    def round_trip(arr):
        buf = io.BytesIO()
        evaluate._save_png(buf, arr)
        buf.seek(0)
        return np.array(Image.open(buf))
    back = {k: round_trip(r[k].numpy()) for k in ("renders", "gt", "depth", "error_map", "dtumask")}
    assert np.array_equal(back["renders"], r["renders"].numpy()) and np.array_equal(back["gt"], r["gt"].numpy())
    for k in ("depth", "error_map", "dtumask"):                 # a single channel is written as three equal ones
        assert back[k].shape == (19, 23, 3) and all(np.array_equal(back[k][:, :, c], r[k].numpy()) for c in range(3))
    # / 255 of what was read back are the floats the metrics use (metrics.py:39-44)
    a, b, mask_bin = ER.masked_images(torch.from_numpy(back["renders"]), torch.from_numpy(back["gt"]), torch.from_numpy(back["dtumask"][:, :, 0]))
    assert torch.equal(a[0], r["renders_masked"]) and torch.equal(b[0], r["gt_masked"]) and int(mask_bin.sum()) == r["K"]


def _records(rows):
    rec = torch.zeros((len(rows), evaluate.RECORD_WORDS), dtype=torch.int64)
    for i, (S, K, ssim_sum) in enumerate(rows):
        rec[i, 0], rec[i, 1] = S, K
        rec[i, 2:3].view(torch.float32)[:] = torch.tensor([123.0, ssim_sum])          # (sum |a - b|, sum of the SSIM map)
    return rec


def test_results_from_planted_records():
    n = 3 * 10 * 20
    rows = [(4000, 600, 0.9 * n), (0, 600, 1.0 * n), (4000, 0, 0.5 * n), (1, 3, 0.25 * n)]
    names = [f"{i:05d}.png" for i in range(4)]
    full, per_view = evaluate.results_from_records(_records(rows), names, [n] * 4)
    assert set(full) == set(per_view) == {"SSIM", "PSNR"} and list(per_view["PSNR"]) == names
    psnr = per_view["PSNR"]
    assert psnr[names[0]] == pytest.approx(10 * math.log10(255 ** 2 * 600 / 4000), abs=1e-5)
    assert psnr[names[1]] == float("inf") and math.isnan(psnr[names[2]])
    assert psnr[names[3]] == pytest.approx(10 * math.log10(255 ** 2 * 3), abs=1e-5)
    assert [per_view["SSIM"][k] for k in names] == pytest.approx([0.9, 1.0, 0.5, 0.25], abs=1e-6)
    assert full["SSIM"] == pytest.approx(np.mean([0.9, 1.0, 0.5, 0.25]), abs=1e-6) and math.isnan(full["PSNR"])
    # the set means are fp32 tensor means, as metrics.py:104-105 takes them
    full2, pv2 = evaluate.results_from_records(_records(rows[:1] + rows[3:]), names[:2], [n] * 2)
    want = torch.tensor([pv2["PSNR"][k] for k in names[:2]]).mean().item()
    assert full2["PSNR"] == want and isinstance(full2["PSNR"], float)
    assert evaluate.psnr_from_sums(0, 0) != evaluate.psnr_from_sums(0, 0)          # K == 0 wins over S == 0: an empty mean is NaN


def test_lpips_and_the_avg_quirk():
    n = 3 * 8 * 8
    rows = [(4000, 192, 0.9 * n), (9000, 192, 0.8 * n)]
    names = ["00000.png", "00001.png"]
    full, per_view = evaluate.results_from_records(_records(rows), names, [n] * 2, lpips=[0.2, 0.4])
    assert set(full) == set(per_view) == {"SSIM", "PSNR", "LPIPS", "AVG"}
    assert [per_view["LPIPS"][k] for k in names] == pytest.approx([0.2, 0.4], abs=1e-7)
    for k, lp in zip(names, (0.2, 0.4)):
        want = math.exp(np.mean(np.log([10 ** (-per_view["PSNR"][k] / 10), math.sqrt(1 - per_view["SSIM"][k]), lp])))
        assert per_view["AVG"][k] == pytest.approx(want, rel=1e-5)
    # metrics.py:107: the set's "AVG" is the mean of the LPIPS values, not of the per-view AVGs
    assert full["AVG"] == full["LPIPS"] == pytest.approx(0.3, abs=1e-6)
    assert full["AVG"] != pytest.approx(np.mean(list(per_view["AVG"].values())), abs=1e-3)


def test_write_results_json_shape(tmp_path):
    n = 3 * 8 * 8
    full, per_view = evaluate.results_from_records(_records([(4000, 192, 0.9 * n)]), ["00000.png"], [n])
    evaluate.write_results(str(tmp_path / "model"), {"ours_7": full}, {"ours_7": per_view})
    a = json.load(open(tmp_path / "model" / "results.json"))
    b = json.load(open(tmp_path / "model" / "per_view.json"))
    assert a == {"ours_7": full} and set(a["ours_7"]) == {"SSIM", "PSNR"}
    assert b["ours_7"]["PSNR"] == {"00000.png": per_view["PSNR"]["00000.png"]} and set(b["ours_7"]) == {"SSIM", "PSNR"}


def test_new_symbols_are_declared_exported_and_bound():
    lib = _lib.load()
    declared = abi_text.declared_by("scg_eval.h")
    assert declared == sorted(NEW_SYMBOLS)
    for name in declared:
        assert name in _lib.SYMBOLS, f"ctypes binding lacks {name}"
        assert hasattr(lib, name), f"libscg_raster.so does not export {name}"
    assert lib.scg_abi_version() == _lib.ABI_VERSION == 10
    assert lib.scg_eval_view_tile(0) >= 4 and lib.scg_eval_view_tile(1) >= 4 and lib.scg_eval_view_tile(2) == 0
    assert lib.scg_eval_depth_range_scratch_bytes(1) >= 8
    assert lib.scg_eval_depth_range_scratch_bytes(1600 * 1200) > lib.scg_eval_depth_range_scratch_bytes(400 * 300)
    # the source is built without contraction: the quantiser's two roundings
    from scgaussian_amd import build
    assert "-ffp-contract=off" in build.SOURCES["evalview.hip"]


def test_argument_validation_returns_codes_without_a_gpu():
    lib = _lib.load()
    fake = 0x10000            # never dereferenced: validation fails first
    NULL, RANGE, SCRATCH, ALIGN = -1, -2, -4, -5
    assert lib.scg_eval_depth_range(None, 10, fake, fake, 1 << 20, None) == NULL
    assert lib.scg_eval_depth_range(fake, 10, None, fake, 1 << 20, None) == NULL
    assert lib.scg_eval_depth_range(fake, 10, fake, None, 1 << 20, None) == NULL
    assert lib.scg_eval_depth_range(fake, 0, fake, fake, 1 << 20, None) == RANGE
    assert lib.scg_eval_depth_range(fake, 1 << 31, fake, fake, 1 << 30, None) == RANGE
    assert lib.scg_eval_depth_range(fake, 100_000, fake, fake, 16, None) == SCRATCH
    assert lib.scg_eval_depth_range(fake, 10, fake, fake + 4, 1 << 20, None) == ALIGN

    def view(H=8, W=8, **kw):
        names = ("render", "gt", "depth", "dtumask", "range", "render_u8", "gt_u8", "depth_u8", "error_u8", "mask_u8", "error_f32",
                 "render_masked", "gt_masked", "sk")
        a = {k: fake for k in names}
        a.update(kw)
        return lib.scg_eval_view(a["render"], a["gt"], a["depth"], a["dtumask"], a["range"], H, W, *[a[k] for k in names[5:]], None)
    for H, W in ((2, 8), (8, 2), (0, 0), (-1, 8)):
        assert view(H, W) == RANGE
    assert b"3 x 3" in lib.scg_last_error() or b"smaller" in lib.scg_last_error()
    assert view(65536, 32768) == RANGE                                  # H * W = 2^31
    for k in ("render", "gt", "depth", "range", "render_u8", "gt_u8", "depth_u8", "error_u8", "render_masked", "gt_masked", "sk"):
        assert view(**{k: None}) == NULL, k
    assert view(mask_u8=None) == NULL                                   # a mask comes with its output
    assert view(sk=fake + 4) == ALIGN


def test_cpu_tensors_are_refused():
    r, g, d = ER.images(8, 8, 0)
    with pytest.raises(_lib.ScgError, match="no CPU path"):
        evaluate.evaluate_view(r, g, d)
    with pytest.raises(_lib.ScgError, match="no CPU path"):
        evaluate.EvalSet(2, device="cpu")

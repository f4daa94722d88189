"""CPU-side checks of the DTU path (scgaussian_amd/dtu.py, csrc/dtumask.hip): the references the GPU tests lean on, the ABI and the
argument validation.  No kernel runs here.

What anchors what: eval_metrics_ref (tests/dtu_refs.py) in fp64 is pinned to numbers the reference's own l1_loss / psnr / mse
produced (tests/golden/ref_dtu.npz, written by tests/golden/make_golden_dtu.py).  The background-mask rule lives inline in the
reference's train.py:149-158 and cannot be imported, so the mask rests on its restatement, dtu_refs.bg_mask_loop; this file holds
that loop equal to the one-rule-per-pixel form the kernel implements."""
import os

import numpy as np
import pytest
import torch

import abi_text
import dtu_refs as DR
from scgaussian_amd import _lib, dtu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_dtu.npz")
NEW_SYMBOLS = ("scg_dtu_bg_mask", "scg_dtu_bg_mask_segment_rows", "scg_masked_mean_scratch_bytes", "scg_masked_mean_forward",
               "scg_masked_mean_backward", "scg_eval_metrics_scratch_bytes", "scg_eval_metrics")


@pytest.mark.parametrize("H", [1, 49, 50, 51, 120])
@pytest.mark.parametrize("thr", [DR.THR, DR.THR_SCAN110])
def test_the_reference_loop_is_the_closed_form(H, thr):
    for seed, share in ((0, 0.97), (1, 0.8), (2, 1.0), (3, 0.0)):
        img = DR.dark_run_image(H, 23, seed + 10 * H, share)
        mask, gt_masked, count = DR.bg_mask_loop(img, thr)
        want = DR.bg_mask_closed_form(img.numpy(), thr)
        assert mask.shape == (1, H, 23) and np.array_equal(mask[0].numpy(), want)
        assert int(count) == int(want.sum())
        assert torch.equal(gt_masked, torch.where(torch.from_numpy(want)[None].expand(3, -1, -1), torch.zeros(()), img))
        if share == 0.97 and H >= 50:
            assert 0 < int(count) < H * 23                                # the case bites: some runs reach 50 rows, some break
        # the rule is idempotent: the masked image has the same mask
        again, gt2, _ = DR.bg_mask_loop(gt_masked, thr)
        assert torch.equal(again, mask) and torch.equal(gt2, gt_masked)


def test_the_threshold_itself_is_not_dark():
    t32 = np.float32(DR.THR)
    below = np.nextafter(t32, np.float32(0))
    img = torch.zeros(3, 2, 2)
    img[1, 0, 0] = float(t32)
    img[2, 0, 1] = float(below)
    mask, _, _ = DR.bg_mask_loop(img, DR.THR)
    assert mask[0].tolist() == [[False, True], [False, True]]
    assert np.array_equal(DR.bg_mask_closed_form(img.numpy(), DR.THR), mask[0].numpy())


def test_threshold_for():
    assert dtu.threshold_for("/data/dtu/scan24") == 30 / 255 == DR.THR
    assert dtu.threshold_for("/data/dtu/scan110/") == 15 / 255 == DR.THR_SCAN110


def test_metric_restatement_in_fp64_is_the_reference():
    z = np.load(GOLDEN)
    for name in ("plain", "masked", "clamped"):
        img, gt = torch.from_numpy(z[f"{name}_img"]), torch.from_numpy(z[f"{name}_gt"])
        m = torch.from_numpy(z[f"{name}_mask"]) if f"{name}_mask" in z.files else None
        for tag, dtype, tol in (("64", torch.float64, 1e-14), ("32", torch.float32, 1e-6)):
            r = DR.eval_metrics_ref(img, gt, m, dtype)
            assert abs(r["l1"] - float(z[f"{name}_l1_{tag}"])) <= tol
            assert abs(r["psnr"] - float(z[f"{name}_psnr_{tag}"])) <= tol * 100
            assert np.abs(r["mse"] - z[f"{name}_mse_{tag}"]).max() <= tol
    assert int(z["masked_selected"]) == 43 and int(z["clamped_selected"]) == 55 and float(z["clamped_img"].min()) < 0 and float(z["clamped_gt"].max()) > 1


def test_new_symbols_are_declared_exported_and_bound():
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert abi_text.header_of(name) == "scg_loss.h", f"include/scg_loss.h does not declare {name}"
        assert name in _lib.SYMBOLS, f"ctypes binding lacks {name}"
        assert hasattr(lib, name), f"libscg_raster.so does not export {name}"
    assert lib.scg_abi_version() == _lib.ABI_VERSION == 10
    assert lib.scg_dtu_bg_mask_segment_rows() >= 1
    assert lib.scg_masked_mean_scratch_bytes(1) >= 4 and lib.scg_masked_mean_scratch_bytes(10_000_000) >= 10_000_000 // 4096 * 4
    assert lib.scg_eval_metrics_scratch_bytes(3, 1200, 1600) > lib.scg_eval_metrics_scratch_bytes(3, 300, 400) > 0


def test_argument_validation_returns_codes_without_a_gpu():
    lib = _lib.load()
    fake, other = 0x10000, 0x4000000            # never dereferenced: validation fails first
    NULL, RANGE, SCRATCH = -1, -2, -4
    # background mask
    assert lib.scg_dtu_bg_mask(None, 8, 8, 0.1, 50, fake, other, fake, None) == NULL
    assert lib.scg_dtu_bg_mask(fake, 8, 8, 0.1, 50, None, other, fake, None) == NULL
    assert lib.scg_dtu_bg_mask(fake, 8, 8, 0.1, 50, fake, None, fake, None) == NULL
    assert lib.scg_dtu_bg_mask(fake, 8, 8, 0.1, 50, fake, other, None, None) == NULL
    assert lib.scg_dtu_bg_mask(fake, 8, 8, 0.1, 0, fake, other, fake, None) == RANGE and b"run" in lib.scg_last_error()
    assert lib.scg_dtu_bg_mask(fake, 8, 8, 0.1, -3, fake, fake, fake, None) == RANGE
    assert lib.scg_dtu_bg_mask(fake, 8, 8, 0.0, 50, fake, fake, fake, None) == RANGE and b"alias" in lib.scg_last_error()
    assert lib.scg_dtu_bg_mask(fake, 8, 8, -1.0, 50, fake, fake, fake, None) == RANGE
    assert lib.scg_dtu_bg_mask(fake, 8, 8, 0.1, 50, fake, fake + 64, fake, None) == RANGE and b"overlap" in lib.scg_last_error()
    assert lib.scg_dtu_bg_mask(fake, 0, 8, 0.1, 50, fake, other, fake, None) == RANGE
    assert lib.scg_dtu_bg_mask(fake, 65536, 32768, 0.1, 50, fake, other, fake, None) == RANGE          # H * W = 2^31
    # masked mean
    assert lib.scg_masked_mean_forward(None, fake, 10, fake, fake, fake, 1 << 20, None) == NULL
    assert lib.scg_masked_mean_forward(fake, fake, 10, None, fake, fake, 1 << 20, None) == NULL
    assert lib.scg_masked_mean_forward(fake, fake, 10, fake, fake, None, 1 << 20, None) == NULL
    assert lib.scg_masked_mean_forward(fake, fake, 0, fake, fake, fake, 1 << 20, None) == RANGE
    assert lib.scg_masked_mean_forward(fake, fake, 100_000, fake, fake, fake, 16, None) == SCRATCH
    assert lib.scg_masked_mean_backward(fake, 10, fake, None, fake, None) == NULL
    assert lib.scg_masked_mean_backward(None, 10, fake, fake, fake, None) == NULL
    assert lib.scg_masked_mean_backward(fake, -1, fake, fake, fake, None) == RANGE
    # metrics
    assert lib.scg_eval_metrics(None, fake, None, 3, 8, 8, fake, fake, 1 << 20, None) == NULL
    assert lib.scg_eval_metrics(fake, fake, None, 3, 8, 8, None, fake, 1 << 20, None) == NULL
    assert lib.scg_eval_metrics(fake, fake, None, 0, 8, 8, fake, fake, 1 << 20, None) == RANGE
    assert lib.scg_eval_metrics(fake, fake, None, 17, 8, 8, fake, fake, 1 << 20, None) == RANGE
    assert lib.scg_eval_metrics(fake, fake, None, 3, 800, 800, fake, fake, 16, None) == SCRATCH


def test_cpu_tensors_are_refused():
    gt = torch.rand(3, 8, 8)
    with pytest.raises(_lib.ScgError, match="no CPU path"):
        dtu.background_mask(gt)
    with pytest.raises(_lib.ScgError, match="no CPU path"):
        dtu.DtuView(gt)
    with pytest.raises(_lib.ScgError, match="no CPU path"):
        dtu.eval_metrics(gt, gt)
    with pytest.raises(_lib.ScgError, match="no CPU path"):
        dtu.alpha_term(torch.rand(1, 8, 8), None)

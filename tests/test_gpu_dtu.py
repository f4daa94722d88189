"""The DTU path on the GPU (scgaussian_amd/dtu.py, csrc/dtumask.hip) against the plain-torch restatements of tests/dtu_refs.py.

Mask: exact (torch.equal) against dtu_refs.bg_mask_loop, the restatement of train.py:149-158.  That rule is inline code of the
reference's training loop and cannot be imported, so the mask rests on the restatement (tests/test_dtu_cpu.py holds it equal to the
closed form); the metrics rest on numbers the reference's own l1_loss / psnr produced (tests/golden/ref_dtu.npz).
Values: err <= max(4 * e32, floor) with e32 the error of the fp32 restatement against the fp64 one (loss_refs.held_to).
Whole step: parity_utils.assert_close, eager and replayed from a captured graph."""
import math
import os
import types

import numpy as np
import pytest
import torch

import dtu_refs as DR
import loss_refs as LR
import parity_utils as pu
from scgaussian_amd import _lib, dtu
from scgaussian_amd import graph_step as gs
from scgaussian_amd import rasterizer as R
from scgaussian_amd import synthetic as syn

pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_dtu.npz")
SEG = _lib.load().scg_dtu_bg_mask_segment_rows()
HEIGHTS = sorted({1, 49, 50, 51, 99, 100, 101, 130, SEG - 1, SEG, SEG + 1})
WIDTHS = [1, 63, 64, 65, 257]
# element counts of the sums: one wave short / exact / over, one workgroup chunk (4 096) plus one, and more than 1 024 chunks,
# where a thread of the final reduction adds more than one partial sum (the second level of the reduction)
SIZES = {1: (1, 1), 63: (7, 9), 64: (8, 8), 65: (5, 13), 4097: (17, 241), 4096 * 1024 + 2048: (2049, 2048)}


def _check_mask(img, thr, run=DR.RUN):
    want_mask, want_gt, want_count = DR.bg_mask_loop(img, thr, run)
    mask, gt_masked, count = dtu.background_mask(img.to(DEV), thr, run)
    assert mask.dtype == torch.bool and mask.shape == want_mask.shape and count.dim() == 0
    assert torch.equal(mask.cpu(), want_mask)
    assert torch.equal(gt_masked.cpu(), want_gt)
    assert torch.equal(count.cpu().long(), want_count)
    return want_mask, mask, gt_masked, count


@pytest.mark.parametrize("W", WIDTHS)
@pytest.mark.parametrize("H", HEIGHTS)
def test_mask_random_runs(H, W):
    for thr in (DR.THR, DR.THR_SCAN110):
        if H * W == 1:                                       # one pixel: masked or not, both
            for v in (0.0, 0.5):
                _check_mask(torch.full((3, 1, 1), v), thr)
            continue
        for seed in range(40):                               # inputs whose masked share is neither nothing nor everything
            img = DR.dark_run_image(H, W, 1000 * H + 10 * W + seed)
            share = float(DR.bg_mask_loop(img, thr)[0].float().mean())
            if 0.02 < share < 0.98:
                break
        assert 0.02 < share < 0.98, (H, W, share)
        want_mask, mask, gt_masked, count = _check_mask(img, thr)
        # in place equals out of place, and the ground truth handed in IS the one written
        gt = img.to(DEV).clone()
        m2, g2, c2 = dtu.background_mask(gt, thr, inplace=True)
        assert g2 is gt and torch.equal(gt, gt_masked) and torch.equal(m2, mask) and torch.equal(c2, count)
        # the rule is idempotent: applied to its own output, nothing changes
        m3, g3, c3 = dtu.background_mask(gt_masked, thr)
        assert torch.equal(m3, mask) and torch.equal(g3, gt_masked) and torch.equal(c3, count)


@pytest.mark.parametrize("thr", [DR.THR, DR.THR_SCAN110])
def test_mask_planted_patterns(thr):
    H, W = 130, 65
    t32 = np.float32(thr)
    below = float(np.nextafter(t32, np.float32(0)))
    img = torch.full((3, H, W), 0.5)
    dark = 0.01

    def run_of(col, start, length):
        img[:, start:start + length, col] = dark
    run_of(0, 0, H)                                          # all dark
    # column 1: none dark
    for col, n in ((2, 49), (3, 50), (4, 51)):               # runs from row 0
        run_of(col, 0, n)
    for col, n in ((5, 49), (6, 50), (7, 51)):               # runs from row 60
        run_of(col, 60, n)
    run_of(8, 10, 70)
    img[1, 40, 8] = 0.5                                      # broken by a pixel bright in ONE channel: 30 + 39 rows
    run_of(9, 0, 100)
    img[2, 60, 9] = 0.5                                      # rows 0..59 from the top, then 39 rows
    run_of(10, 0, H)
    img[1, 5, 10] = float(t32)                               # the threshold itself is not dark
    run_of(11, 0, H)
    img[1, 5, 11] = below                                    # one ulp under it is
    want_mask, mask, _, _ = _check_mask(img, thr)
    m = mask[0].cpu()
    rows = lambda col: m[:, col].nonzero().flatten().tolist()             # noqa: E731
    assert rows(0) == list(range(H)) and rows(1) == []
    assert rows(2) == list(range(49)) and rows(3) == list(range(50)) and rows(4) == list(range(51))
    assert rows(5) == [] and rows(6) == [109] and rows(7) == [109, 110]
    assert rows(8) == [] and rows(9) == list(range(60))
    assert rows(10) == list(range(5)) + list(range(55, H)) and rows(11) == list(range(H))
    # other run lengths than the reference's 50, the shortest included
    for run in (1, 2, 33):
        _check_mask(img, thr, run)
    # a NaN channel is not dark (torch: the max is NaN and NaN < thr is false); the pixel keeps its values
    img[0, 70, 0] = float("nan")
    want_mask, want_gt, want_count = DR.bg_mask_loop(img, thr)
    mask, gt_masked, count = dtu.background_mask(img.to(DEV), thr)
    assert torch.equal(mask.cpu(), want_mask) and int(count) == int(want_count)
    assert mask[0, :, 0].nonzero().flatten().tolist() == list(range(70)) + list(range(120, H))
    assert torch.equal(gt_masked.cpu().nan_to_num(7.0), want_gt.nan_to_num(7.0)) and math.isnan(float(gt_masked[0, 70, 0]))


def _view(mask_bool):
    """What alpha_term reads of a DtuView, around a mask chosen by the test."""
    m = mask_bool.to(DEV).contiguous()
    return types.SimpleNamespace(mask=m, _mask_u8=m.view(torch.uint8).reshape(-1), count=m.sum().to(torch.int32))


def _alpha_case(alpha, mask, upstream, what):
    a = alpha.to(DEV).requires_grad_(True)
    view = _view(mask)
    out = dtu.alpha_term(a, view)
    out.backward(torch.tensor(upstream, device=DEV))
    torch.cuda.synchronize()
    a2 = alpha.to(DEV).requires_grad_(True)                               # a second run: bitwise the same
    out2 = dtu.alpha_term(a2, view)
    out2.backward(torch.tensor(upstream, device=DEV))
    assert torch.equal(out.detach().view(torch.int32), out2.detach().view(torch.int32)) and torch.equal(a.grad, a2.grad)
    return float(out.detach()), a.grad.cpu()


@pytest.mark.parametrize("n", sorted(SIZES))
def test_alpha_term_value_and_gradient(n):
    H, W = SIZES[n]
    g = torch.Generator().manual_seed(n)
    alpha = torch.rand(1, H, W, generator=g)
    cases = {"full": torch.ones(1, H, W, dtype=torch.bool), "single": torch.zeros(1, H, W, dtype=torch.bool)}
    cases["single"][0, H // 2, W // 3] = True
    if n > 1:
        cases["random"] = torch.rand(1, H, W, generator=g) < 0.4
        assert 0 < int(cases["random"].sum()) < n
    upstream = 0.7
    for name, mask in cases.items():
        got, grad = _alpha_case(alpha, mask, upstream, name)
        v64, g64, e32 = DR.alpha_term_bars(alpha, mask, upstream)
        LR.held_to(f"dtu alpha {n} {name} value", abs(got - v64), e32, LR.VALUE_FLOOR)
        # the gradient: exactly the fp32 quotient upstream / count under the mask, exactly 0 elsewhere
        q = torch.tensor(upstream, dtype=torch.float32) / torch.tensor(float(int(mask.sum())), dtype=torch.float32)
        assert torch.equal(grad, torch.where(mask, q, torch.zeros(())))
        _, g32 = DR.alpha_term_ref(alpha, mask, torch.float32, upstream)
        s = float(g64.abs().max())
        LR.held_to(f"dtu alpha {n} {name} grad", float((grad.double() - g64).abs().max()) / s,
                   float((g32.double() - g64).abs().max()) / s, LR.GRAD_FLOOR, elements=n)


def test_alpha_term_empty_mask_is_nan_with_zero_gradient():
    alpha = torch.rand(1, 17, 241)
    got, grad = _alpha_case(alpha, torch.zeros(1, 17, 241, dtype=torch.bool), 1.0, "empty")
    assert math.isnan(got) and torch.equal(grad, torch.zeros(1, 17, 241))
    # masked-out entries never enter the sum, whatever they hold
    alpha[0, 3, 3] = float("inf")
    mask = torch.rand(1, 17, 241) < 0.5
    mask[0, 3, 3] = False
    got, _ = _alpha_case(alpha, mask, 1.0, "inf outside")
    assert math.isfinite(got)


def _metrics_case(what, img, gt, m, r64, e32):
    l1, psnr, mse = dtu.eval_metrics_all(img.to(DEV), gt.to(DEV), None if m is None else m.to(DEV))
    l1b, psnrb = dtu.eval_metrics(img.to(DEV), gt.to(DEV), None if m is None else m.to(DEV))
    assert torch.equal(l1, l1b) and torch.equal(psnr, psnrb)               # fixed order: bitwise the same twice
    LR.held_to(f"dtu metrics {what} l1", abs(float(l1) - r64["l1"]), e32["l1"], LR.VALUE_FLOOR)
    for c in range(img.shape[0]):
        LR.held_to(f"dtu metrics {what} mse[{c}]", abs(float(mse[c]) - float(r64["mse"][c])), float(e32["mse"][c]), LR.VALUE_FLOOR)
    LR.held_to(f"dtu metrics {what} psnr", abs(float(psnr) - r64["psnr"]), e32["psnr"], DR.psnr_floor(r64["mse"]))


def test_metrics_match_the_reference_golden():
    z = np.load(GOLDEN)
    for name in ("plain", "masked", "clamped"):
        img, gt = torch.from_numpy(z[f"{name}_img"]), torch.from_numpy(z[f"{name}_gt"])
        m = torch.from_numpy(z[f"{name}_mask"]) if f"{name}_mask" in z.files else None
        r64 = dict(l1=float(z[f"{name}_l1_64"]), psnr=float(z[f"{name}_psnr_64"]), mse=z[f"{name}_mse_64"])
        e32 = dict(l1=abs(float(z[f"{name}_l1_32"]) - r64["l1"]), psnr=abs(float(z[f"{name}_psnr_32"]) - r64["psnr"]),
                   mse=np.abs(z[f"{name}_mse_32"] - r64["mse"]))
        _metrics_case(f"golden {name}", img, gt, m, r64, e32)


@pytest.mark.parametrize("n", sorted(SIZES))
def test_metrics_match_the_restatement(n):
    H, W = SIZES[n]
    g = torch.Generator().manual_seed(100 + n)
    img = torch.rand(3, H, W, generator=g) * 1.8 - 0.4                    # about a third outside [0, 1]: clamped in the kernel
    gt = torch.rand(3, H, W, generator=g) * 1.8 - 0.4
    if n == 1:                                                            # one pixel: clamped below, inside, clamped above; no mse of 0
        img, gt = torch.tensor([-0.2, 0.4, 1.3]).reshape(3, 1, 1), torch.tensor([0.3, 0.9, 0.6]).reshape(3, 1, 1)
    masks = {"unmasked": None, "all": torch.full((H, W), 255.0)}
    if n > 1:
        m = torch.randn(H, W, generator=g)
        m[m.abs() < 0.3] = 0.0                                            # zeros and negative entries are not selected
        masks["masked"] = m
    for name, m in masks.items():
        r64, e32 = DR.eval_metrics_bars(img, gt, m)
        _metrics_case(f"{n} {name}", img, gt, m, r64, e32)
    # clamping happens inside: the same numbers, bit for bit, from inputs clamped beforehand
    a = dtu.eval_metrics_all(img.to(DEV), gt.to(DEV))
    b = dtu.eval_metrics_all(img.clamp(0, 1).to(DEV), gt.clamp(0, 1).to(DEV))
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    if n > 1:
        assert float(img.min()) < 0 and float(img.max()) > 1


def test_metrics_of_an_empty_selection_are_nan():
    img, gt = torch.rand(3, 12, 9), torch.rand(3, 12, 9)
    l1, psnr, mse = dtu.eval_metrics_all(img.to(DEV), gt.to(DEV), torch.zeros(12, 9, device=DEV))
    assert math.isnan(float(l1)) and math.isnan(float(psnr)) and bool(torch.isnan(mse).all())
    l1, psnr, mse = dtu.eval_metrics_all(img.to(DEV), gt.to(DEV), -torch.ones(1, 12, 9, device=DEV))
    assert math.isnan(float(l1)) and math.isnan(float(psnr))


def test_whole_dtu_step_eager_and_captured():
    """About 2 000 Gaussians at 64 x 64, a ground truth with a dark band at the top: dtu.training_loss and its parameter gradients
    against the torch restatement of train.py:149-161 + :167-168 on the same render; then the same closure captured and replayed."""
    P, W, H = 2000, 64, 64
    sc = syn.make_scene(P, W, H, seed=21)
    cam = syn.orbit_camera(W, H, 3.0, -2.0, 7.0)
    rast = R.GaussianRasterizer(pu.hip_settings(cam, 3, (0.0, 0.0, 0.0)))
    leaves = [t.detach().clone().to(DEV).requires_grad_(True) for t in (sc.means3D, sc.shs, sc.opacities, sc.scales, sc.rotations)]

    def render():
        m, f, o, s, r = leaves
        c, _radii, _d, a = rast(means3D=m, means2D=torch.zeros_like(m, requires_grad=True), opacities=o, shs=f, scales=s, rotations=r)
        return c, a
    with torch.no_grad():
        c0, _ = render()
    gt = (c0 * 0.7 + 0.2).clamp(0, 1)                                    # nowhere dark by itself
    gt[:, :30, 8:56] = 0.02                                               # the dark band: 30 rows from the top
    view = dtu.DtuView(gt)
    assert int(view.count) == 30 * 48 and torch.equal(view.gt[:, :30, 8:56], torch.zeros(3, 30, 48, device=DEV))

    def fn():
        c, a = render()
        loss = dtu.training_loss(c, a, view)
        loss.backward()
        return loss, c, a

    def restated():
        c, a = render()
        loss = DR.training_loss_torch(c, a, gt)
        loss.backward()
        return loss

    def run(f):
        for p in leaves:
            p.grad = None
        out = f()
        torch.cuda.synchronize()
        loss = out[0] if isinstance(out, tuple) else out
        return loss.detach().clone().reshape(1), [p.grad.detach().clone() for p in leaves]
    want_loss, want_g = run(restated)
    got_loss, got_g = run(fn)
    names = ("means3D", "shs", "opacities", "scales", "rotations")
    pu.assert_close(got_loss, want_loss, ("dtu step", "loss"))
    for k, g, w in zip(names, got_g, want_g):
        pu.assert_close(g, w, ("dtu step", "grad", k))
    # the alpha term reached the rasterizer: without it the opacity gradient differs
    assert float(view.count) > 0 and float((got_g[2]).abs().max()) > 0
    # captured: a host read inside fn would fail the capture
    step = gs.CapturedStep(fn, params=leaves)
    for _ in range(3):
        out = step.replay()
    torch.cuda.synchronize()
    pu.assert_close(out[0].detach().reshape(1), got_loss, ("dtu step replay", "loss"))
    pu.assert_close(out[0].detach().reshape(1), want_loss, ("dtu step replay", "loss vs torch"))
    for k, p, g, w in zip(names, leaves, got_g, want_g):
        pu.assert_close(p.grad, g, ("dtu step replay", "grad", k))
        pu.assert_close(p.grad, w, ("dtu step replay", "grad vs torch", k))
    assert step.overflows == 0 and step.recaptures == 0
    step.close()

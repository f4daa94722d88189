"""Fused L1 + SSIM image loss against vectors produced by the REFERENCE's own
utils/loss_utils.py (tests/golden/make_golden.py): values and the gradient w.r.t. the rendered image."""
import numpy as np
import pytest
import torch

import loss_refs as lr


@pytest.mark.gpu
@pytest.mark.parametrize("tag", ["a", "b"])
def test_image_loss_matches_reference_golden(ref_pieces, tag):
    from scgaussian_amd import losses
    x = torch.from_numpy(ref_pieces[f"iloss_{tag}_img"]).cuda().requires_grad_(True)
    y = torch.from_numpy(ref_pieces[f"iloss_{tag}_gt"]).cuda()
    l1, s = losses.l1_and_ssim(x, y)
    assert abs(float(l1) - float(ref_pieces[f"iloss_{tag}_l1"])) < 1e-6
    assert abs(float(s) - float(ref_pieces[f"iloss_{tag}_ssim"])) < 2e-6
    loss = losses.image_loss(x, y, 0.2)
    assert abs(float(loss) - float(ref_pieces[f"iloss_{tag}_loss"])) < 2e-6
    loss.backward()
    ref = ref_pieces[f"iloss_{tag}_grad"]
    err = np.abs(x.grad.cpu().numpy() - ref).max() / np.abs(ref).max()
    assert err < 1e-4, err


@pytest.mark.gpu
def test_image_loss_matches_small_golden_and_separate_functions(ref_pieces):
    from scgaussian_amd import losses
    a = torch.from_numpy(ref_pieces["loss_img1"]).cuda()
    b = torch.from_numpy(ref_pieces["loss_img2"]).cuda()
    assert abs(float(losses.l1_loss(a, b)) - float(ref_pieces["loss_l1"])) < 1e-6
    assert abs(float(losses.ssim(a, b)) - float(ref_pieces["loss_ssim"])) < 2e-6
    # batched input and identical images
    assert abs(float(losses.ssim(a[None], a[None])) - 1.0) < 1e-6
    assert float(losses.l1_loss(a, a)) == 0.0


@pytest.mark.gpu
def test_image_loss_gradient_against_torch_autograd_at_training_size():
    """1008x756 (BASELINE cfg 2): gradient vs a plain-torch fp32 SSIM (conv2d) on the same GPU."""
    import torch.nn.functional as F
    from scgaussian_amd import losses
    g = torch.Generator().manual_seed(0)
    H, W = 756, 1008
    x = torch.rand(3, H, W, generator=g).cuda().requires_grad_(True)
    y = (x.detach().cpu() + 0.1 * torch.randn(3, H, W, generator=g)).clamp(0, 1).cuda()
    loss = losses.image_loss(x, y, 0.2)
    loss.backward()
    got = x.grad.clone()
    x.grad = None
    gauss = torch.tensor([np.exp(-(i - 5) ** 2 / (2 * 1.5 ** 2)) for i in range(11)], dtype=torch.float32)
    gauss = gauss / gauss.sum()
    win = (gauss[:, None] @ gauss[None, :]).expand(3, 1, 11, 11).contiguous().cuda()
    conv = lambda t: F.conv2d(t[None], win, padding=5, groups=3)[0]      # noqa: E731
    mu1, mu2 = conv(x), conv(y)
    s1, s2, s12 = conv(x * x) - mu1 * mu1, conv(y * y) - mu2 * mu2, conv(x * y) - mu1 * mu2
    smap = ((2 * mu1 * mu2 + 1e-4) * (2 * s12 + 9e-4)) / ((mu1 * mu1 + mu2 * mu2 + 1e-4) * (s1 + s2 + 9e-4))
    ref_loss = 0.8 * (x - y).abs().mean() + 0.2 * (1 - smap.mean())
    ref_loss.backward()
    assert abs(float(loss) - float(ref_loss)) < 1e-5
    err = float((got - x.grad).abs().max() / x.grad.abs().max())
    assert err < 1e-4, err


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16, torch.float64])
def test_image_and_match_loss_gradients_come_back_in_the_input_dtype(dtype):
    """Non-fp32 inputs are converted for the kernels; autograd must get the gradient back in the input's dtype."""
    from scgaussian_amd import losses
    from scgaussian_amd.match_loss import match_loss_from_depth
    g = torch.Generator().manual_seed(1)
    x = torch.rand(3, 40, 56, generator=g).cuda().to(dtype).requires_grad_(True)
    y = torch.rand(3, 40, 56, generator=g).cuda()
    losses.image_loss(x, y, 0.2).backward()
    assert x.grad is not None and x.grad.dtype == dtype and torch.isfinite(x.grad.float()).all()
    d = (torch.rand(1, 40, 56, generator=g) * 3 + 4).cuda().to(dtype).requires_grad_(True)
    M = 50
    pair = dict(uv0=torch.rand(M, 2, generator=g).cuda() * 40, rays_o=torch.zeros(M, 3).cuda(),
                rays_d=torch.nn.functional.normalize(torch.rand(M, 3, generator=g) + torch.tensor([0.0, 0.0, 2.0]), dim=1).cuda(),
                cam_rays_d=torch.nn.functional.normalize(torch.rand(M, 3, generator=g) + torch.tensor([0.0, 0.0, 2.0]), dim=1).cuda(),
                mask0=None, mask1=None, intr1=torch.tensor([[50.0, 0, 28], [0, 50.0, 20], [0, 0, 1]]).cuda(),
                w2c1=torch.eye(4).cuda(), uv1=torch.rand(M, 2, generator=g).cuda() * 40)
    match_loss_from_depth(d, [pair], 56.0, 40.0).backward()
    assert d.grad is not None and d.grad.dtype == dtype


@pytest.mark.gpu
@pytest.mark.parametrize("lam,scale", [(0.2, 1.0), (0.0, 1.0), (1.0, 1.0), (0.35, -2.5)])
def test_combined_image_loss_equals_the_separate_calls_and_the_expression_around_them(lam, scale):
    """losses.image_loss (one scalar from the reduction kernel, the upstream gradient read by the backward kernel) against
    l1_and_ssim + the reference's expression in torch (train.py:160-161): the value to the last bit or two (each operation
    rounded on its own, the reference's order), the image gradient to 1e-6 of its maximum; with an upstream gradient that is
    not 1 (the loss scaled and summed with another term, as the match loss is)."""
    from scgaussian_amd import losses
    g = torch.Generator().manual_seed(3)
    H, W = 97, 130
    x0 = torch.rand(3, H, W, generator=g).cuda()
    y = (x0.cpu() + 0.1 * torch.randn(3, H, W, generator=g)).clamp(0, 1).cuda()
    xa = x0.clone().requires_grad_(True)
    xb = x0.clone().requires_grad_(True)
    la = losses.image_loss(xa, y, lam)
    l1, s = losses.l1_and_ssim(xb, y)
    lb = (1.0 - lam) * l1 + lam * (1.0 - s)
    assert la.shape == lb.shape == ()
    assert abs(float(la) - float(lb)) <= 2.5e-7 * max(1.0, abs(float(lb))), (float(la), float(lb))
    (scale * la + 1.0).backward()
    (scale * lb + 1.0).backward()
    err = float((xa.grad - xb.grad).abs().max() / xb.grad.abs().max())
    assert err < 1e-6, err
    with torch.no_grad():                                   # no gradient wanted: no derivative maps are written
        assert abs(float(losses.image_loss(x0, y, lam)) - float(la)) == 0.0


@pytest.mark.gpu
def test_image_loss_takes_any_lambda_the_reference_expression_takes():
    """a lambda outside [0, 1] or a tensor lambda (with a gradient of its own) is combined in torch from the fused
    L1 / SSIM pair — the combined kernel only takes a plain number in [0, 1]."""
    from scgaussian_amd import losses
    g = torch.Generator().manual_seed(5)
    x = torch.rand(3, 48, 64, generator=g).cuda().requires_grad_(True)
    y = torch.rand(3, 48, 64, generator=g).cuda()
    l1, s = losses.l1_and_ssim(x.detach(), y)
    for lam in (1.5, -0.25):
        got = losses.image_loss(x, y, lam)
        assert abs(float(got) - float((1.0 - lam) * l1 + lam * (1.0 - s))) <= 1e-6
    lam_t = torch.tensor(0.3, device="cuda", requires_grad=True)
    losses.image_loss(x, y, lam_t).backward()
    assert x.grad is not None and lam_t.grad is not None
    assert abs(float(lam_t.grad) - float((1.0 - s) - l1)) <= 1e-6       # d/d lambda of (1 - lambda) L1 + lambda (1 - SSIM)


# --------------------------------------------------------------------------------------------------------------------------------
# fp64 edge parity.  Reference: loss_refs.image_loss_ref(float64) on the CPU (pinned to the reference project's goldens by
# tests/test_loss_refs_cpu.py).  Bar per case: err_kernel <= max(4 * e32, floor), e32 = the error of the SAME expression evaluated
# with plain torch in fp32; floors 2e-6 (values, absolute) and 1e-6 (gradient, normalised by s = max(max|g64|, 1 / (C*H*W))).
# The bar is therefore never looser than the 1e-4 / 2e-6 of the tests above, with ONE exception: constant images, where
# e11 - m1 * m1 cancels in fp32 (e32 of the normalised gradient 6.9e-5 at 3x64x96) and 4 * e32 is the bar.
#
# SHAPES (C,H,W)                       what the shape exercises (32x32 output tiles, 42x42 halo, 11-tap window)
EDGE_SHAPES = [
    (3, 1, 1),                       # a single pixel: every tap but the centre is padding
    (3, 5, 7),                       # smaller than the 5-pixel halo
    (1, 11, 11),                     # exactly the window; C = 1
    (3, 10, 43),                     # one less than the window high, one past the halo tile wide
    (3, 31, 64),                     # one short of a tile high, exactly two tiles wide
    (3, 32, 32),                     # exactly one tile
    (3, 33, 65),                     # one past a tile edge both ways
    (4, 200, 3),                     # a tall sliver, C = 4
    (2, 3, 200),                     # a wide sliver, C = 2
    (1, 64, 96),                     # exact tiles, C = 1
    (5, 37, 70),                     # the golden's size with C = 5
    (3, 97, 130),                    # the size of the combined-loss test
    (2, 3, 37, 70),                  # batched (B,C,H,W)
]
# CONTENT KINDS
EDGE_KINDS = ["random", "hdr", "constant", "same", "one_pixel"]
# SEAM IMPULSES: zero images with a single pixel set, on the corner shared by four tiles and on the last row / column; one
# impulse's 11x11 footprint crosses four tiles in both separable passes.  "corner36" is the LAST element of tile (0,0)'s 42x42 halo
# (row 36, column 36), weight 1e-6 in exactly one output pixel: amplitude 100 makes that one tap visible in the SSIM value.
SEAM_SHAPE = (3, 66, 70)
SEAM_IMPULSES = {"31_31": (31, 31, 1.0), "31_32": (31, 32, 1.0), "32_31": (32, 31, 1.0), "32_32": (32, 32, 1.0),
                 "last_row": (65, 40, 1.0), "last_col": (20, 69, 1.0), "last_corner": (65, 69, 1.0), "corner36": (36, 36, 100.0)}
LAMBDAS = [0.0, 0.2, 1.0]


def _content(kind, shape, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(*shape, generator=g)
    y = (x + 0.1 * torch.randn(*shape, generator=g)).clamp(0, 1)
    if kind == "hdr":                                   # values outside [0, 1]
        x, y = 8 * x - 2, 8 * y - 2
    elif kind == "constant":
        x, y = torch.full(shape, 0.5), torch.full(shape, 0.25)
    elif kind == "same":                                # gt == img exactly
        y = x.clone()
    elif kind == "one_pixel":                           # gt == img except for one pixel
        y = x.clone()
        y.view(-1)[y.numel() // 2] += 0.25
    return x, y


def _check_all_paths(tag, x, y):
    """l1_and_ssim; image_loss at lambda 0 / 0.2 / 1 (value, gradient, no-grad forward bit-identical); a non-unit upstream."""
    from scgaussian_amd import losses
    xd, yd = x.cuda(), y.cuda()
    n = x.numel()
    for lam in LAMBDAS:
        r64, e32, s = lr.image_loss_bars(x, y, lam)
        xa = xd.clone().requires_grad_(True)
        la = losses.image_loss(xa, yd, lam)
        assert la.shape == ()
        la.backward()
        assert xa.grad.shape == x.shape and torch.isfinite(xa.grad).all()
        with torch.no_grad():                               # no gradient wanted: the same value to the last bit
            assert float(losses.image_loss(xd, yd, lam)) == float(la)
        lr.held_to(f"iloss {tag} lam={lam} loss", abs(float(la) - r64["loss"]), e32["loss"], lr.VALUE_FLOOR)
        err = float((xa.grad.cpu().double() - r64["grad"]).abs().max()) / s
        lr.held_to(f"iloss {tag} lam={lam} grad", err, e32["grad"], lr.GRAD_FLOOR, n)
    # the separate pair, its gradient through the reference's expression in torch
    r64, e32, s = lr.image_loss_bars(x, y, 0.2)
    xb = xd.clone().requires_grad_(True)
    l1, ss = losses.l1_and_ssim(xb, yd)
    lr.held_to(f"iloss {tag} l1", abs(float(l1) - r64["l1"]), e32["l1"], lr.VALUE_FLOOR)
    lr.held_to(f"iloss {tag} ssim", abs(float(ss) - r64["ssim"]), e32["ssim"], lr.VALUE_FLOOR)
    (0.8 * l1 + 0.2 * (1.0 - ss)).backward()
    err = float((xb.grad.cpu().double() - r64["grad"]).abs().max()) / s
    lr.held_to(f"iloss {tag} pair grad", err, e32["grad"], lr.GRAD_FLOOR, n)
    with torch.no_grad():
        l1n, ssn = losses.l1_and_ssim(xd, yd)
        assert float(l1n) == float(l1) and float(ssn) == float(ss)
    # a non-unit upstream gradient: -2.5 * loss + 1
    r64, e32, s = lr.image_loss_bars(x, y, 0.2, upstream=(-2.5, 1.0))
    xc = xd.clone().requires_grad_(True)
    (-2.5 * losses.image_loss(xc, yd, 0.2) + 1.0).backward()
    err = float((xc.grad.cpu().double() - r64["grad"]).abs().max()) / s
    lr.held_to(f"iloss {tag} upstream -2.5 grad", err, e32["grad"], lr.GRAD_FLOOR, n)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", EDGE_KINDS)
@pytest.mark.parametrize("shape", EDGE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_image_loss_edge_shapes_against_fp64(shape, kind):
    x, y = _content(kind, shape, seed=sum(shape) + len(kind))
    _check_all_paths(f"{'x'.join(map(str, shape))} {kind}", x, y)


@pytest.mark.gpu
@pytest.mark.parametrize("side", ["img", "gt"])
@pytest.mark.parametrize("name", list(SEAM_IMPULSES))
def test_image_loss_seam_impulses_against_fp64(name, side):
    """Forward (the impulse in the image) and backward (the impulse in gt: the image gradient exists only through the maps the
    backward kernel convolves) of one impulse whose footprint crosses the tile seams."""
    r, c, amp = SEAM_IMPULSES[name]
    a, b = torch.zeros(SEAM_SHAPE), torch.zeros(SEAM_SHAPE)
    a[:, r, c] = amp
    a[1, r, c] = 0.5 * amp                                    # the channels differ
    x, y = (a, b) if side == "img" else (b, a)
    _check_all_paths(f"seam {name} in {side}", x, y)


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["channel_slice", "column_slice", "permuted_hwc"])
def test_image_loss_non_contiguous_image_against_fp64(layout):
    from scgaussian_amd import losses
    g = torch.Generator().manual_seed(17)
    C, H, W = 3, 37, 70
    if layout == "channel_slice":                             # every other channel of a larger tensor
        base = torch.rand(2 * C, H, W, generator=g).cuda().requires_grad_(True)
        view = base[::2]
    elif layout == "column_slice":
        base = torch.rand(C, H, W + 9, generator=g).cuda().requires_grad_(True)
        view = base[:, :, 4:4 + W]
    else:
        base = torch.rand(H, W, C, generator=g).cuda().requires_grad_(True)
        view = base.permute(2, 0, 1)
    assert not view.is_contiguous() and view.shape == (C, H, W)
    y = torch.rand(C, H, W, generator=g)
    x = view.detach().cpu().contiguous()
    r64, e32, s = lr.image_loss_bars(x, y, 0.2)
    loss = losses.image_loss(view, y.cuda(), 0.2)
    loss.backward()
    lr.held_to(f"iloss {layout} loss", abs(float(loss) - r64["loss"]), e32["loss"], lr.VALUE_FLOOR)
    # the gradient arrives in the BASE tensor's layout: zero outside the view, the reference's inside
    want = torch.zeros(base.shape, dtype=torch.float64)
    if layout == "channel_slice":
        want[::2] = r64["grad"]
    elif layout == "column_slice":
        want[:, :, 4:4 + W] = r64["grad"]
    else:
        want = r64["grad"].permute(1, 2, 0)
    err = float((base.grad.cpu().double() - want).abs().max()) / s
    lr.held_to(f"iloss {layout} grad", err, e32["grad"], lr.GRAD_FLOOR, x.numel())


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16, torch.float64])
def test_image_loss_other_input_dtypes_against_fp64_of_the_converted_input(dtype):
    """The kernels take fp32: an fp16 / bf16 image is widened (exactly), an fp64 one rounded.  The value is held against the fp64
    reference of the CONVERTED input; the gradient comes back in the input's dtype, so its bar adds that dtype's rounding."""
    from scgaussian_amd import losses
    g = torch.Generator().manual_seed(23)
    shape = (3, 37, 70)
    x = torch.rand(*shape, generator=g, dtype=torch.float64).to(dtype)
    y = torch.rand(*shape, generator=g)
    xf = x.float()                                            # what the kernel sees
    r64, e32, s = lr.image_loss_bars(xf, y, 0.2)
    xd = x.cuda().requires_grad_(True)
    loss = losses.image_loss(xd, y.cuda(), 0.2)
    loss.backward()
    lr.held_to(f"iloss {dtype} loss", abs(float(loss) - r64["loss"]), e32["loss"], lr.VALUE_FLOOR)
    assert xd.grad.dtype == dtype and xd.grad.shape == shape
    out_rounding = 0.0 if dtype == torch.float64 else float(torch.finfo(dtype).eps) / 2      # of the returned gradient
    err = float((xd.grad.cpu().double() - r64["grad"]).abs().max()) / s
    lr.held_to(f"iloss {dtype} grad", err, e32["grad"] + out_rounding / lr.FACTOR, lr.GRAD_FLOOR, x.numel())

"""tests/loss_refs.py pinned on the CPU: the fp64 image-loss reference against the goldens the reference project produced, the
kd-tree kNN reference against the fp32 brute force on the adversarial clouds, and the match-loss reference against the oracle it
wraps.  The edge-parity GPU tests compare the kernels with these helpers, so the helpers are anchored here, not to the kernels."""
import numpy as np
import pytest
import torch

import loss_refs as lr
from oracle import knn_oracle as ko
from oracle import match_loss_oracle as mlo


@pytest.mark.parametrize("tag", ["a", "b"])
def test_image_loss_ref_fp64_reproduces_the_reference_goldens(ref_pieces, tag):
    x = torch.from_numpy(ref_pieces[f"iloss_{tag}_img"])
    y = torch.from_numpy(ref_pieces[f"iloss_{tag}_gt"])
    r = lr.image_loss_ref(x, y, 0.2, torch.float64)
    # the goldens are fp32 evaluations stored as fp32: a few ulp of values in [0, 1]
    for k in ("l1", "ssim", "loss"):
        want = float(ref_pieces[f"iloss_{tag}_{k}"])
        assert abs(r[k] - want) <= 4 * np.finfo(np.float32).eps * max(1.0, abs(want)), (k, r[k], want)
    g = ref_pieces[f"iloss_{tag}_grad"]
    err = np.abs(r["grad"].numpy() - g).max() / np.abs(g).max()
    assert err < 2e-6, err                                  # measured 2e-7 .. 4e-7: the golden's own fp32 rounding
    assert r["grad"].dtype == torch.float64 and r["grad"].shape == x.shape


def test_image_loss_ref_fp32_is_a_plain_fp32_evaluation_and_batches_like_the_reference():
    g = torch.Generator().manual_seed(0)
    x, y = torch.rand(2, 3, 20, 31, generator=g), torch.rand(2, 3, 20, 31, generator=g)
    r64, e32, s = lr.image_loss_bars(x, y, 0.2)
    assert 0 < e32["grad"] < 1e-5 and e32["loss"] < 1e-6 and s == float(r64["grad"].abs().max())
    assert lr.image_loss_ref(x, y, 0.2, torch.float32)["grad"].dtype == torch.float32
    # (B,C,H,W) is B*C independent planes under one mean: the same numbers as the (B*C,H,W) stack
    flat = lr.image_loss_ref(x.reshape(6, 20, 31), y.reshape(6, 20, 31), 0.2, torch.float64)
    assert abs(flat["loss"] - r64["loss"]) < 1e-15 and torch.allclose(flat["grad"].reshape(x.shape), r64["grad"], rtol=1e-12, atol=1e-18)
    # gt == img: the fp64 gradient is 0 up to fp64 rounding and the scale falls back to the L1 term's 1 / numel
    same = lr.image_loss_ref(x, x, 0.2, torch.float64)
    assert float(same["grad"].abs().max()) < 1e-15 and lr.grad_scale(same["grad"]) == 1.0 / x.numel()
    # an upstream gradient a * loss + b scales the gradient by a
    up = lr.image_loss_ref(x, y, 0.2, torch.float64, upstream=(-2.5, 1.0))
    assert torch.allclose(up["grad"], -2.5 * r64["grad"], rtol=1e-10, atol=1e-18)


CLOUD_CASES = [(kind, n) for kind in ("lattice", "identical", "collinear", "clusters", "offset1e3", "aniso")
               for n in (4, 5, 64, 1025, 3000)]


@pytest.mark.parametrize("kind,n", CLOUD_CASES)
def test_knn_ref64_equals_the_fp32_brute_force_on_the_adversarial_clouds(kind, n):
    p = lr.CLOUDS[kind](n, 11 * n + 3)
    assert p.shape == (n, 3) and p.dtype == np.float32
    ref = lr.knn_ref64(p)
    bf = ko.mean_dist2_bruteforce(p)
    # fp32 brute force: every squared distance carries the rounding of (a - b) at the coordinates' magnitude
    scale = float(np.abs(p).max())
    atol = 8 * np.finfo(np.float32).eps * scale * np.sqrt(ref.max() + 1e-30) + 1e-12
    np.testing.assert_allclose(bf, ref, rtol=2e-5, atol=atol)
    if kind == "identical":
        assert not ref.any() and not bf.any()
    if kind == "lattice" and n >= 64:                       # interior points: three neighbours at exactly one spacing
        assert np.isclose(np.median(ref), 0.25)


def test_match_loss_ref_is_the_oracle_on_cast_inputs_and_decisions_agree_with_it():
    g = torch.Generator().manual_seed(4)
    M, W, H = 200, 40, 30
    depth = 5.0 + torch.rand(H, W, generator=g)
    uv0 = torch.rand(M, 2, generator=g) * torch.tensor([W + 4.0, H + 4.0]) - 2
    cam = torch.nn.functional.normalize(torch.cat([(uv0 - torch.tensor([W / 2.0, H / 2.0])) / 50.0, torch.ones(M, 1)], 1), dim=1)
    p = dict(uv0=uv0, rays_o=torch.zeros(M, 3), rays_d=cam.clone(), cam_rays_d=cam, mask0=(torch.rand(M, generator=g) > 0.3).float(),
             mask1=None, intr1=torch.tensor([[50.0, 0, W / 2.0], [0, 50.0, H / 2.0], [0, 0, 1]]),
             w2c1=torch.tensor([[1.0, 0, 0, 0.4], [0, 1, 0, -0.2], [0, 0, 1, 0.1], [0, 0, 0, 1]]),
             uv1=torch.rand(M, 2, generator=g) * torch.tensor([float(W), float(H)]))
    p["mask1"] = torch.ones(M)
    for dtype in (torch.float32, torch.float64):
        d = depth.to(dtype).clone().requires_grad_(True)
        want = mlo.match_loss_pair(d, *(p[k].to(dtype) for k in ("uv0", "rays_o", "rays_d", "cam_rays_d", "mask0", "mask1", "intr1",
                                                                 "w2c1", "uv1")), float(W), float(H))
        want.backward()
        got, grad = lr.match_loss_ref(depth, [p], W, H, dtype)
        assert got == float(want) and torch.equal(grad, d.grad) and grad.dtype == dtype
    two, grad2 = lr.match_loss_ref(depth, [p, p], W, H, torch.float64, upstream=0.5)
    assert abs(two - 2 * got) < 1e-14 and torch.allclose(grad2, grad, rtol=1e-13, atol=0)
    dec = lr.match_decisions(depth, p, W, H)
    assert 0 < int(dec["counts"].sum()) < M
    # the loss recomputed from the decisions is the oracle's
    cur = 0.5 * ((dec["xy"][0] - p["uv1"][:, 0].double()).abs() / W + (dec["xy"][1] - p["uv1"][:, 1].double()).abs() / H)
    assert abs(float((cur * dec["counts"]).sum() / (dec["counts"].sum() + 1e-8)) - got) < 1e-12
    empty, g0 = lr.match_loss_ref(depth, [{k: (v[:0] if v.dim() and v.shape[0] == M else v) for k, v in p.items()}], W, H, torch.float64)
    assert empty == 0.0 and not g0.any()

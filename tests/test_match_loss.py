"""Fused match loss from the rendered depth against the line-by-line CPU restatement of
scene/gaussian_model.py:241-282 (oracle/match_loss_oracle.py), value and gradient w.r.t. the depth image."""
import math

import numpy as np
import pytest
import torch

import loss_refs as lr
from oracle import match_loss_oracle as mlo
from scgaussian_amd import synthetic as syn


def _intr(cam):
    W, H = cam.image_width, cam.image_height
    fx, fy = W / (2 * math.tan(cam.FoVx / 2)), H / (2 * math.tan(cam.FoVy / 2))
    return torch.tensor([[fx, 0, W / 2.0], [0, fy, H / 2.0], [0, 0, 1]], dtype=torch.float32)


def _pair(cam0, cam1, depth0, M, seed, with_masks=True):
    """Matches of view 0 -> view 1 built from a depth map of view 0 (plus pixel noise on the view-1 side)."""
    g = torch.Generator().manual_seed(seed)
    W, H = cam0.image_width, cam0.image_height
    K0, K1 = _intr(cam0), _intr(cam1)
    w2c0, w2c1 = cam0.world_view_transform.t().contiguous(), cam1.world_view_transform.t().contiguous()
    c2w0 = torch.linalg.inv(w2c0)
    uv0 = torch.stack([torch.rand(M, generator=g) * (W + 6) - 3, torch.rand(M, generator=g) * (H + 6) - 3], 1)
    cam_rays = (torch.linalg.inv(K0) @ torch.cat([uv0, torch.ones(M, 1)], 1).t()).t()
    cam_rays = cam_rays / cam_rays.norm(dim=1, keepdim=True)
    rays_d = (c2w0[:3, :3] @ cam_rays.t()).t().contiguous()
    rays_o = c2w0[:3, 3][None].repeat(M, 1).contiguous()
    # "true" matches: sample the depth, lift, project into view 1, add noise
    with torch.no_grad():
        gx = (uv0[:, 0] / W) * 2 - 1
        gy = (uv0[:, 1] / H) * 2 - 1
        d = torch.nn.functional.grid_sample(depth0[None, None], torch.stack([gx, gy], -1)[None, None], align_corners=False).reshape(-1)
        z = d / cam_rays[:, 2]
        world = rays_o + rays_d * z[:, None]
        cam = (w2c1 @ torch.cat([world, torch.ones(M, 1)], 1).t())[:3]
        xyz = K1 @ cam
        uv1 = (xyz[:2] / (xyz[2:] + 1e-8)).t() + torch.randn(M, 2, generator=g) * 3.0
    mask0 = (torch.rand(M, generator=g) > 0.2).float() if with_masks else None
    mask1 = (torch.rand(M, generator=g) > 0.2).float() if with_masks else None
    return dict(uv0=uv0.contiguous(), rays_o=rays_o, rays_d=rays_d, cam_rays_d=cam_rays.contiguous(), mask0=mask0,
                mask1=mask1, intr1=K1, w2c1=w2c1, uv1=uv1.contiguous())


@pytest.mark.gpu
@pytest.mark.parametrize("M", [1, 37, 1999, 5000])
def test_match_loss_matches_oracle(M):
    from scgaussian_amd.match_loss import match_loss_from_depth
    W, H = 252, 189
    cam0 = syn.orbit_camera(W, H, 0.0, 0.0, 7.0)
    cams = [syn.orbit_camera(W, H, 9.0, 2.0, 7.0), syn.orbit_camera(W, H, -7.0, -3.0, 7.5)]
    g = torch.Generator().manual_seed(M)
    yy, xx = torch.meshgrid(torch.arange(H).float(), torch.arange(W).float(), indexing="ij")
    depth = 6.0 + 1.5 * torch.sin(xx / 31.0) * torch.cos(yy / 23.0) + 0.05 * torch.randn(H, W, generator=g)
    pairs = [_pair(cam0, c, depth, M, 10 * M + k) for k, c in enumerate(cams)]

    d_cpu = depth.clone().requires_grad_(True)
    ones = torch.ones(M)
    ref = sum(mlo.match_loss_pair(d_cpu, p["uv0"], p["rays_o"], p["rays_d"], p["cam_rays_d"],
                                  p["mask0"] if p["mask0"] is not None else ones,
                                  p["mask1"] if p["mask1"] is not None else ones, p["intr1"], p["w2c1"], p["uv1"],
                                  float(W), float(H)) for p in pairs)
    (ref * 0.3).backward()                      # train.py:165 weights it by 0.3

    d_gpu = depth.clone().cuda()[None].requires_grad_(True)           # (1,H,W) like rendered_depth
    out = match_loss_from_depth(d_gpu, [{k: (v.cuda() if v is not None else None) for k, v in p.items()} for p in pairs],
                                float(W), float(H))
    (out * 0.3).backward()
    assert abs(float(out.detach()) - float(ref.detach())) <= 2e-5 * max(1.0, abs(float(ref.detach())))
    gref = d_cpu.grad.numpy()
    ggot = d_gpu.grad[0].cpu().numpy()
    assert np.abs(gref).max() > 0
    assert np.abs(ggot - gref).max() <= 1e-4 * np.abs(gref).max()
    assert (ggot != 0).sum() <= 4 * 2 * M


@pytest.mark.gpu
def test_match_loss_without_masks_and_no_grad():
    from scgaussian_amd.match_loss import match_loss_from_depth
    W, H = 100, 80
    cam0, cam1 = syn.orbit_camera(W, H, 0.0, 0.0, 7.0), syn.orbit_camera(W, H, 6.0, 0.0, 7.0)
    depth = torch.full((H, W), 7.0)
    p = _pair(cam0, cam1, depth, 300, 5, with_masks=False)
    ones = torch.ones(300)
    ref = mlo.match_loss_pair(depth, p["uv0"], p["rays_o"], p["rays_d"], p["cam_rays_d"], ones, ones, p["intr1"],
                              p["w2c1"], p["uv1"], float(W), float(H))
    with torch.no_grad():
        out = match_loss_from_depth(depth.cuda(), [{k: (v.cuda() if v is not None else None) for k, v in p.items()}],
                                    float(W), float(H))
    assert abs(float(out) - float(ref)) < 2e-5


# --------------------------------------------------------------------------------------------------------------------------------
# fp64 edge parity.  Reference: loss_refs.match_loss_ref(float64) = oracle.match_loss_oracle.match_loss_pair on inputs cast to fp64,
# value and gradient w.r.t. the depth.  Bar: err_kernel <= max(4 * e32, floor) with e32 = the fp32 CPU oracle against fp64 and the
# floors of the test above (2e-5 * max(1, |ref|) on the value, 1e-4 * max|g| on the gradient).
#
# The in-image test of view 1 and the sign of px - uv1.x / py - uv1.y are step functions.  NO match is excluded for lying near
# one: every generator below is seeded so that the fp64 reference has no match within 1e-3 pixel of a step, and _compare asserts
# that on the reference before it compares anything.
#
# CASES                                  what they exercise
#   M sweep (EDGE_M)                     two register matches per thread up to 2 048, the loop path beyond, min(i, M - 1) clamps
#   count 0 (three variants)             1 / (0 + 1e-8) times a zero numerator; nothing scattered
#   border taps                          bilinear taps on and across the depth image's border, the four corners
#   hot pixel                            2 048 matches on one pixel: all atomics on four addresses
#   behind view 1                        Z < 0 and |Z| small in the second camera
#   non-binary masks                     mask0 * mask1 > 0 with values in {0, 0.5, 1, -1}
#   width, height = 2 W, 2 H             the image size the matches live in is not the depth map's
#   six pairs, different M               the reference's 2 000 x 6 into one gradient image
#   non-contiguous fp64 pair tensors     the binding's conversion
EDGE_M = [0, 1, 63, 64, 65, 1023, 1024, 1025, 2047, 2048, 2049, 3073, 4097]
MW, MH = 252, 189


def _depth(W, H, seed):
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.arange(H).float(), torch.arange(W).float(), indexing="ij")
    return 6.0 + 1.5 * torch.sin(xx / 31.0 * 252.0 / W) * torch.cos(yy / 23.0 * 189.0 / H) + 0.05 * torch.randn(H, W, generator=g)


def _pair_from_uv0(cam0, cam1, depth0, uv0, seed, masks="binary", w2c1=None, noise=3.0):
    """Matches of view 0 -> view 1 at GIVEN uv0 (pixels of the cameras' image size, which need not be the depth map's size); uv1 is
    the projection plus noise of at least 0.05 pixel per axis, so no match sits on the L1 term's kink."""
    g = torch.Generator().manual_seed(seed)
    M = uv0.shape[0]
    W, H = cam0.image_width, cam0.image_height
    K0, K1 = _intr(cam0), _intr(cam1)
    w2c0 = cam0.world_view_transform.t().contiguous()
    w2c1 = cam1.world_view_transform.t().contiguous() if w2c1 is None else w2c1
    c2w0 = torch.linalg.inv(w2c0)
    cam_rays = (torch.linalg.inv(K0) @ torch.cat([uv0, torch.ones(M, 1)], 1).t()).t()
    cam_rays = cam_rays / cam_rays.norm(dim=1, keepdim=True)
    rays_d = (c2w0[:3, :3] @ cam_rays.t()).t().contiguous()
    rays_o = c2w0[:3, 3][None].repeat(M, 1).contiguous()
    p = dict(uv0=uv0.contiguous(), rays_o=rays_o, rays_d=rays_d, cam_rays_d=cam_rays.contiguous(), mask0=None, mask1=None,
             intr1=K1, w2c1=w2c1, uv1=torch.zeros(M, 2))
    if M == 0:
        p["mask0"], p["mask1"] = (torch.zeros(0), torch.zeros(0)) if masks else (None, None)
        return p
    xy = lr.match_decisions(depth0, p, float(W), float(H))["xy"].t().float()
    n = torch.randn(M, 2, generator=g) * noise
    p["uv1"] = (xy + n + torch.sign(n) * 0.05).contiguous()
    if masks == "binary":
        p["mask0"], p["mask1"] = ((torch.rand(M, generator=g) > 0.2).float() for _ in range(2))
    elif masks == "nonbinary":
        vals = torch.tensor([0.0, 0.5, 1.0, -1.0])
        p["mask0"], p["mask1"] = (vals[torch.randint(0, 4, (M,), generator=g)] for _ in range(2))
    return p


def _random_uv0(W, H, M, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.stack([torch.rand(M, generator=g) * (W + 6) - 3, torch.rand(M, generator=g) * (H + 6) - 3], 1)


def _cams(W, H):
    return syn.orbit_camera(W, H, 0.0, 0.0, 7.0), [syn.orbit_camera(W, H, 9.0, 2.0, 7.0), syn.orbit_camera(W, H, -7.0, -3.0, 7.5)]


def _to_cuda(p):
    return {k: (v.cuda() if v is not None else None) for k, v in p.items()}


def _compare(tag, depth, pairs, width, height, grad_e32=None, expect_zero=False):
    """The kernel against the fp64 reference under max(4 * e32, floor); returns (reference decisions per pair, gradient)."""
    from scgaussian_amd.match_loss import match_loss_from_depth
    decs = [lr.match_decisions(depth, p, width, height) for p in pairs if p["uv0"].shape[0]]
    for k, d in enumerate(decs):                                  # the precondition: no decision of the reference is marginal
        assert float(d["margin"].min()) >= lr.MARGIN_PX, (tag, "pair", k, "a match lies", float(d["margin"].min()), "px from a step")
    ref, g64 = lr.match_loss_ref(depth, pairs, width, height, torch.float64, upstream=0.3)
    r32, g32 = lr.match_loss_ref(depth, pairs, width, height, torch.float32, upstream=0.3)
    d_gpu = depth.clone().cuda()[None].requires_grad_(True)           # (1,H,W) like rendered_depth
    out = match_loss_from_depth(d_gpu, [_to_cuda(p) for p in pairs], float(width), float(height))
    (out * 0.3).backward()
    got, ggot = float(out.detach()), d_gpu.grad[0].cpu()
    assert np.isfinite(got) and torch.isfinite(ggot).all()
    with torch.no_grad():                                             # the forward without a gradient image: one workgroup
        out_ng = match_loss_from_depth(depth.cuda(), [_to_cuda(p) for p in pairs], float(width), float(height))
    assert abs(float(out_ng) - got) <= 1e-6 * max(1.0, abs(got))      # (the loss word is summed over the pairs by atomics)
    m_total = sum(p["uv0"].shape[0] for p in pairs)
    assert int((ggot != 0).sum()) <= 4 * m_total
    if expect_zero:
        assert ref == 0.0 and not g64.any()
        assert got == 0.0 and not ggot.any()
        return decs, ggot
    lr.held_to(f"mloss {tag} value", abs(got - ref), abs(r32 - ref), 2e-5 * max(1.0, abs(ref)))
    gmax = float(g64.abs().max())
    assert gmax > 0
    e32 = float((g32.double() - g64).abs().max()) if grad_e32 is None else grad_e32
    lr.held_to(f"mloss {tag} grad", float((ggot.double() - g64).abs().max()) / gmax, e32 / gmax, 1e-4, g64.numel())
    return decs, ggot


@pytest.mark.gpu
@pytest.mark.parametrize("M", EDGE_M)
def test_match_loss_path_switches_against_fp64(M):
    cam0, cams = _cams(MW, MH)
    depth = _depth(MW, MH, 1000 + M)
    uvs = [_random_uv0(MW, MH, M, 31 * M + k) for k in range(2)]
    if M:
        uvs[0][M - 1] = torch.tensor([140.25, 90.5])          # the last match, whose index the clamps repeat, lies in both views
    pairs = [_pair_from_uv0(cam0, c, depth, uvs[k], 77 * M + k) for k, c in enumerate(cams)]
    if M:
        pairs[0]["mask0"][M - 1] = pairs[0]["mask1"][M - 1] = 1.0
    decs, _ = _compare(f"M={M}", depth, pairs, MW, MH, expect_zero=(M == 0))
    if M > 2048:                # the loop path's gradient is only tested if matches beyond the register pair count
        assert any(bool(d["counts"][2048:].any()) for d in decs)
    if M:                       # ... and the last match counts in the first pair
        assert bool(decs[0]["counts"][M - 1])


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["mask0_zero", "all_outside_view1", "both"])
def test_match_loss_with_no_counting_match_is_exactly_zero(variant):
    cam0, cams = _cams(MW, MH)
    depth = _depth(MW, MH, 5)
    M = 1500
    w2c1 = None
    if variant != "mask0_zero":                                   # view 1 moved 1 000 units sideways: every projection leaves it
        w2c1 = cams[0].world_view_transform.t().contiguous().clone()
        w2c1[0, 3] += 1000.0
    p = _pair_from_uv0(cam0, cams[0], depth, _random_uv0(MW, MH, M, 3), 4, w2c1=w2c1)
    if variant != "all_outside_view1":
        p["mask0"] = torch.zeros(M)
    if variant == "all_outside_view1":
        p["mask0"], p["mask1"] = torch.ones(M), torch.ones(M)
    decs, _ = _compare(f"count0 {variant}", depth, [p], MW, MH, expect_zero=True)
    assert int(decs[0]["counts"].sum()) == 0
    if variant != "mask0_zero":
        assert not bool(decs[0]["in_img"].any())


@pytest.mark.gpu
def test_match_loss_bilinear_taps_on_and_across_the_border():
    """Sample coordinates ix in {-1.5, -1, -0.5, 0, W-1.5, W-1, W-0.5, W} times the same in y (the four corners included): taps
    outside the depth image contribute zero, as grid_sample(padding_mode="zeros") does."""
    cam0, cams = _cams(MW, MH)
    depth = _depth(MW, MH, 6)
    ix = torch.tensor([-1.5, -1.0, -0.5, 0.0, MW - 1.5, MW - 1.0, MW - 0.5, float(MW)])
    iy = torch.tensor([-1.5, -1.0, -0.5, 0.0, MH - 1.5, MH - 1.0, MH - 0.5, float(MH)])
    uv0 = torch.stack([(ix + 0.5)[None, :].expand(8, 8).reshape(-1), (iy + 0.5)[:, None].expand(8, 8).reshape(-1)], 1)   # width == W
    wide = syn.orbit_camera(MW, MH, 2.0, 1.0, 7.0, fovy_deg=110.0)   # a wide second view: the half-weighted samples stay inside it
    p = _pair_from_uv0(cam0, wide, depth, uv0, 8, masks=None)
    decs, ggot = _compare("border taps", depth, [p], MW, MH)
    assert int(decs[0]["counts"].sum()) >= 16                       # the samples with a tap inside project into view 1
    # the gradient only exists on the outermost two rows / columns
    inner = ggot[2:-2, :].clone()
    inner[:, :2], inner[:, -2:] = 0, 0
    assert not inner.any()


@pytest.mark.gpu
def test_match_loss_hot_pixel_2048_matches_on_four_addresses():
    """Identical uv0, different uv1: every atomic of the gradient lands on the same four words.  2 048 adds legitimately lose bits,
    so e32 is that of a SEQUENTIALLY summed fp32 reference (per-match gradients from the fp32 oracle, accumulated in order)."""
    cam0, cams = _cams(MW, MH)
    depth = _depth(MW, MH, 7)
    M = 2048
    uv0 = torch.tensor([[100.3, 77.8]]).repeat(M, 1)
    p = _pair_from_uv0(cam0, cams[0], depth, uv0, 9, masks=None, noise=4.0)
    dec = lr.match_decisions(depth, p, MW, MH)
    assert bool(dec["counts"].all())
    # per-match gradient of each sign class (sx, sy) from the fp32 oracle on ONE match, then an in-order fp32 sum over the matches
    sx = (dec["xy"][0] > p["uv1"][:, 0].double()).long()
    sy = (dec["xy"][1] > p["uv1"][:, 1].double()).long()
    cls = (2 * sx + sy).numpy()
    taps = {}
    for c in np.unique(cls):
        i = int(np.nonzero(cls == c)[0][0])
        one = {k: (v[i:i + 1] if (v is not None and v.dim() and v.shape[0] == M) else v) for k, v in p.items()}
        taps[c] = lr.match_loss_ref(depth, [one], MW, MH, torch.float32, upstream=0.3)[1].numpy()
    nz = np.nonzero(np.any([t != 0 for t in taps.values()], axis=0))
    assert len(nz[0]) == 4
    per_match = np.stack([taps[c][nz] for c in cls]).astype(np.float32) / np.float32(M)          # (M, 4)
    seq32 = np.cumsum(per_match, axis=0, dtype=np.float32)[-1]
    _, g64 = lr.match_loss_ref(depth, [p], MW, MH, torch.float64, upstream=0.3)
    e32 = float(np.abs(seq32.astype(np.float64) - g64.numpy()[nz]).max())
    _, ggot = _compare("hot pixel", depth, [p], MW, MH, grad_e32=e32)
    assert int((ggot != 0).sum()) <= 4


@pytest.mark.gpu
def test_match_loss_points_behind_and_close_to_the_second_camera():
    cam0, cams = _cams(MW, MH)
    depth = _depth(MW, MH, 10)
    M = 1200
    w2c1 = cams[0].world_view_transform.t().contiguous().clone()
    w2c1[2, 3] -= 6.0                                             # view 1 moved INTO the surface: part of it lies behind
    uv0 = _random_uv0(MW, MH, M, 12)
    p = _pair_from_uv0(cam0, cams[0], depth, uv0, 13, masks=None, w2c1=w2c1)
    # a few points at |Z| small but not 0: shifted along view 1's axis (its third row) by eps - Z
    z = lr.match_decisions(depth, p, MW, MH)["z"]
    eps = torch.tensor([1e-2, -1e-2, 3e-3, -3e-3, 1e-1, -1e-1])
    idx = torch.arange(100, 100 + eps.numel())
    p["rays_o"][idx] += ((eps.double() - z[idx])[:, None] * w2c1[2, :3].double()[None]).float()
    p = _pair_from_uv0_uv1_again(p, depth, 14)
    dec = lr.match_decisions(depth, p, MW, MH)
    assert float((dec["z"][idx] - eps.double()).abs().max()) < 1e-4 and float(dec["z"][idx].abs().min()) > 1e-3
    assert int((dec["z"] < 0).sum()) > M // 10 and int(dec["counts"].sum()) >= 50
    assert bool((dec["in_img"] & (dec["z"] < 0)).any())           # xy is still formed behind the camera; the mask decides
    _compare("behind view 1", depth, [p], MW, MH)


def _pair_from_uv0_uv1_again(p, depth, seed):
    """uv1 of an edited pair: the fp64 projection plus noise of at least 0.05 pixel per axis."""
    g = torch.Generator().manual_seed(seed)
    xy = lr.match_decisions(depth, p, float(MW), float(MH))["xy"].t().float()
    n = torch.randn(xy.shape[0], 2, generator=g) * 3.0
    p["uv1"] = (xy.clamp(-1e6, 1e6) + n + torch.sign(n) * 0.05).contiguous()
    return p


@pytest.mark.gpu
def test_match_loss_non_binary_masks():
    cam0, cams = _cams(MW, MH)
    depth = _depth(MW, MH, 15)
    M = 1900
    p = _pair_from_uv0(cam0, cams[1], depth, _random_uv0(MW, MH, M, 16), 17, masks="nonbinary")
    prod = p["mask0"] * p["mask1"]
    assert set(prod.unique().tolist()) >= {-1.0, -0.5, 0.0, 0.25, 0.5, 1.0}
    decs, _ = _compare("non-binary masks", depth, [p], MW, MH)
    assert bool((decs[0]["counts"] & (p["mask0"] == -1.0) & (p["mask1"] == -1.0)).any())         # (-1) * (-1) > 0 counts
    assert not bool((decs[0]["counts"] & (prod <= 0)).any())


@pytest.mark.gpu
def test_match_loss_image_size_twice_the_depth_maps():
    """width, height are the size of the images the matches were found in; the depth map may be rendered at another resolution."""
    W2, H2 = 2 * MW, 2 * MH
    cam0, cams = _cams(W2, H2)
    depth = _depth(MW, MH, 18)                                    # (H, W): half the cameras' size
    M = 2000
    p = _pair_from_uv0(cam0, cams[0], depth, _random_uv0(W2, H2, M, 19), 20)
    decs, ggot = _compare("width = 2 W", depth, [p], W2, H2)
    assert int(decs[0]["counts"].sum()) > M // 3 and ggot.shape == (MH, MW)


@pytest.mark.gpu
def test_match_loss_six_pairs_with_different_m_into_one_gradient_image():
    cam0, _ = _cams(MW, MH)
    depth = _depth(MW, MH, 21)
    views = [(9.0, 2.0, 7.0), (-7.0, -3.0, 7.5), (4.0, -6.0, 6.5), (-12.0, 1.0, 7.2), (2.0, 8.0, 7.0), (15.0, 0.0, 8.0)]
    Ms = [2000, 1500, 1024, 2049, 1, 700]
    pairs = [_pair_from_uv0(cam0, syn.orbit_camera(MW, MH, *v), depth, _random_uv0(MW, MH, M, 40 + k), 50 + k)
             for k, (v, M) in enumerate(zip(views, Ms))]
    _compare("six pairs", depth, pairs, MW, MH)
    # (the reference of the call is the sum of the single-pair references)
    whole = lr.match_loss_ref(depth, pairs, MW, MH, torch.float64)
    singles = [lr.match_loss_ref(depth, [p], MW, MH, torch.float64) for p in pairs]
    assert abs(whole[0] - sum(s[0] for s in singles)) < 1e-13
    assert float((whole[1] - sum(s[1] for s in singles)).abs().max()) < 1e-15


@pytest.mark.gpu
def test_match_loss_non_contiguous_fp64_pair_tensors():
    cam0, cams = _cams(MW, MH)
    depth = _depth(MW, MH, 22)
    M = 1025
    p = _pair_from_uv0(cam0, cams[0], depth, _random_uv0(MW, MH, M, 23), 24)
    q = dict(p)
    q["uv0"] = torch.cat([p["uv0"], torch.zeros(M, 1)], 1).double()[:, :2]
    q["uv1"] = torch.cat([torch.zeros(M, 1), p["uv1"]], 1).double()[:, 1:]
    for k in ("rays_o", "rays_d", "cam_rays_d"):
        q[k] = p[k].double().t().contiguous().t()
    q["mask0"], q["mask1"] = torch.stack([p["mask0"], p["mask1"]], 1).double().unbind(1)
    q["intr1"], q["w2c1"] = p["intr1"].double().t().contiguous().t(), p["w2c1"].double().t().contiguous().t()
    assert not any(q[k].is_contiguous() for k in ("uv0", "uv1", "rays_o", "rays_d", "cam_rays_d", "mask0", "intr1", "w2c1"))
    for k in q:
        assert q[k].dtype == torch.float64 and torch.equal(q[k].float(), p[k])
    _compare("non-contiguous fp64", depth, [q], MW, MH)

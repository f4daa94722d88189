"""Shared helpers for the parity tests: run the CPU oracle and the HIP path on the same seeded inputs."""
from __future__ import annotations

import math

import numpy as np
import torch

from oracle import torch_rasterizer as orc
from scgaussian_amd import synthetic as syn

# north_star tolerance: rendered RGB + depth and gradients within 1e-4 relative (fp32); integer artefacts
# (radii, offsets, keys, sort indices, ranges) bit-exact.
REL_TOL = 1e-4


def nrm_err(a, b) -> float:
    """max|a-b| / max|b| — error relative to the tensor's scale."""
    a = torch.as_tensor(a).detach().cpu().double()
    b = torch.as_tensor(b).detach().cpu().double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30)) if b.numel() else 0.0


def elem_violations(a, b, rel: float = REL_TOL, floor_frac: float = 1e-6):
    """Element-wise form of the north-star bar ("within 1e-4 rel"): an element violates when
    |a - b| > rel * |b| + floor_frac * max|b|  (the floor is the fp32 resolution of a sum whose terms are of the
    tensor's scale: an entry that is the cancelled remainder of such terms cannot be resolved below it).
    Returns (fraction of violating elements, worst ratio |a - b| / bound)."""
    a = torch.as_tensor(a).detach().cpu().double().reshape(-1)
    b = torch.as_tensor(b).detach().cpu().double().reshape(-1)
    if b.numel() == 0:
        return 0.0, 0.0
    bound = rel * b.abs() + floor_frac * b.abs().max().clamp_min(1e-30)
    ratio = (a - b).abs() / bound
    return float((ratio > 1.0).double().mean()), float(ratio.max())


# The element-wise form is asserted in two tiers: at most ELEM_FRAC_MAX of the elements may sit outside the bound at
# all, and none may sit further out than ELEM_WORST_MAX times the bound.  Not zero / one, for two documented reasons:
# (1) a per-pixel decision (alpha >= 1/255, T >= 1e-4) taken 1 ulp differently by two fp32 evaluation orders blends or
# skips one splat in one pixel — the images report those pixels separately (threshold_flips), but a flipped pixel also
# moves the gradient entries of the handful of splats it touches; (2) a gradient entry is a sum of thousands of fp32
# terms of either sign, accumulated in a different order (float atomics) and, for the per-splat sums of the blend
# backward, as moments about the quadrant centre shifted to the splat centre — an entry that is the small remainder of
# cancelling terms carries the rounding of the terms, not of the remainder.  Set from the measured census of the
# suite on the MI355X (profiles/r02z_tolerance_census.json: worst share 3.3e-7 — 1.25e-6 in another capture —, worst
# ratio 1.22 over 253 comparisons; gpurun_out/tolerance_census.json is rewritten by conftest at every run): 30x / 1.6x
# above it, so a regression of that size fails.  A tensor too small for the share to mean anything (fewer than
# 1 / ELEM_FRAC_MAX elements) may hold ONE such RECORD (the last dimension of a per-Gaussian tensor: an ill-conditioned
# Gaussian takes the components of its record along together) — still no further out than ELEM_WORST_MAX times the bound.
# Measured (round 3's one-off tools/debug/second_backward.py, in the history: 300 x two backward passes over ONE forward, i.e. nothing but the order of the float
# atomics differs): 4 times two of the four rotation-gradient components of one Gaussian sit 1.8x the bound apart.
ELEM_FRAC_MAX = 1e-5
ELEM_WORST_MAX = 2.0


CENSUS = []          # (what, tensor-scale error, violating share, worst ratio, elements): dumped by conftest at session end


def assert_close(a, b, what="", rel: float = REL_TOL, frac_max: float = ELEM_FRAC_MAX, mask=None):
    """Both forms of the bar: the tensor-scale error and the element-wise one.  `mask` (bool, same shape) removes
    elements that the caller accounts for separately (threshold-flip pixels)."""
    a = torch.as_tensor(a).detach().cpu()
    b = torch.as_tensor(b).detach().cpu()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    assert torch.isfinite(a).all(), what
    record = 1                                   # elements per Gaussian of a (P, ...) tensor with P rows of up to 48 floats
    if mask is None and a.dim() >= 2 and a.shape[0] > 0 and a.numel() // a.shape[0] <= 48:
        record = max(1, a.numel() // a.shape[0])
    if mask is not None:
        keep = ~torch.as_tensor(mask).cpu().expand_as(a)
        a, b = a[keep], b[keep]
    e = nrm_err(a, b)
    frac, worst = elem_violations(a, b, rel)
    CENSUS.append((str(what), e, frac, worst, int(a.numel())))
    assert e < rel, (what, "max|a-b|/max|b|", e)
    n_out = int(round(frac * a.numel()))
    allowed = max(int(frac_max * a.numel()), record) if frac_max > 0.0 else 0
    assert n_out <= allowed, (what, "elements outside 1e-4*|b| + 1e-6*max|b|", n_out, "of", int(a.numel()), "allowed",
                              allowed, "worst ratio", worst)
    assert frac_max == 0.0 or worst <= ELEM_WORST_MAX, (what, "worst |a-b| / (1e-4*|b| + 1e-6*max|b|)", worst)
    return e, frac, worst


def threshold_flips(n_contrib_a, n_contrib_b):
    """Pixels whose contributor count differs between two implementations: a knife-edge alpha / transmittance
    decision.  Returned as a bool (H, W) mask; callers assert on its share and exclude it from the image comparison."""
    a = torch.as_tensor(n_contrib_a).cpu().to(torch.int64)
    b = torch.as_tensor(n_contrib_b).cpu().to(torch.int64)
    return a != b


def tans(cam):
    return math.tan(cam.FoVx / 2), math.tan(cam.FoVy / 2)


def oracle_settings(cam, deg, bg, mod=1.0):
    tx, ty = tans(cam)
    return orc.Settings(cam.image_height, cam.image_width, tx, ty, torch.tensor(bg, dtype=torch.float32), mod,
                        cam.world_view_transform, cam.full_proj_transform, deg, cam.camera_center, False, False)


def hip_settings(cam, deg, bg, mod=1.0, device="cuda"):
    from scgaussian_amd.rasterizer import GaussianRasterizationSettings
    tx, ty = tans(cam)
    camd = cam.to(device)
    return GaussianRasterizationSettings(cam.image_height, cam.image_width, tx, ty,
                                         torch.tensor(bg, dtype=torch.float32, device=device), mod,
                                         camd.world_view_transform, camd.full_proj_transform, deg,
                                         camd.camera_center, False, False)


def scene_inputs(sc, cam, deg, mode="sh_sr"):
    """Input tensors for the four input paths: SH|precomputed colour x scale+rot|precomputed cov3D."""
    P = sc.means3D.shape[0]
    d = dict(means3D=sc.means3D, means2D=torch.zeros(P, 3), opacities=sc.opacities)
    if "sh" in mode.split("_")[0]:
        d["shs"] = sc.shs
    else:
        dirs = sc.means3D - cam.camera_center[None]
        dirs = dirs / dirs.norm(dim=1, keepdim=True)
        d["colors_precomp"] = torch.clamp_min(orc.eval_sh_rgb(deg, sc.shs, dirs) + 0.5, 0.0)
    return d


def run_oracle(sc, cam, deg, bg, mod=1.0, mode="sh_sr", grads=None, aux=True):
    """mode: 'sh_sr' | 'col_sr' | 'sh_cov' | 'col_cov'."""
    P = sc.means3D.shape[0]
    st = oracle_settings(cam, deg, bg, mod)
    col_mode, cov_mode = mode.split("_")
    leaves = {"means3D": sc.means3D.clone().requires_grad_(True), "means2D": torch.zeros(P, 3, requires_grad=True),
              "opacities": sc.opacities.clone().requires_grad_(True)}
    kw = {}
    if col_mode == "sh":
        leaves["shs"] = sc.shs.clone().requires_grad_(True)
        kw["shs"] = leaves["shs"]
    else:
        dirs = sc.means3D - cam.camera_center[None]
        dirs = dirs / dirs.norm(dim=1, keepdim=True)
        leaves["colors_precomp"] = torch.clamp_min(orc.eval_sh_rgb(deg, sc.shs, dirs) + 0.5, 0.0).detach().requires_grad_(True)
        kw["colors_precomp"] = leaves["colors_precomp"]
    if cov_mode == "sr":
        leaves["scales"] = sc.scales.clone().requires_grad_(True)
        leaves["rotations"] = sc.rotations.clone().requires_grad_(True)
        kw["scales"], kw["rotations"] = leaves["scales"], leaves["rotations"]
    else:
        leaves["cov3D_precomp"] = orc.cov3d_from_scale_rot(sc.scales, sc.rotations, mod).detach().requires_grad_(True)
        kw["cov3D_precomp"] = leaves["cov3D_precomp"]
    c, r, d, a, ax = orc.rasterize(leaves["means3D"], leaves["means2D"], leaves["opacities"], st, return_aux=True, **kw)
    out = dict(color=c.detach(), radii=r, depth=d.detach(), alpha=a.detach(), aux=ax, leaves=leaves)
    if grads is not None:
        dc, dd, da = grads
        loss = (c * dc).sum()
        if dd is not None:
            loss = loss + (d * dd).sum()
        if da is not None:
            loss = loss + (a * da).sum()
        loss.backward()
        out["grads"] = {k: v.grad for k, v in leaves.items()}
    return out


def run_hip(sc, cam, deg, bg, mod=1.0, mode="sh_sr", grads=None, leaves_from=None, device="cuda"):
    from scgaussian_amd.rasterizer import GaussianRasterizer
    st = hip_settings(cam, deg, bg, mod, device)
    if leaves_from is None:
        leaves_from = run_oracle_inputs(sc, cam, deg, mod, mode)
    leaves = {k: v.detach().to(device).requires_grad_(True) for k, v in leaves_from.items()}
    kw = {k: v for k, v in leaves.items() if k not in ("means3D", "means2D", "opacities")}
    c, r, d, a = GaussianRasterizer(st)(means3D=leaves["means3D"], means2D=leaves["means2D"],
                                        opacities=leaves["opacities"], **kw)
    out = dict(color=c.detach(), radii=r, depth=d.detach(), alpha=a.detach(), leaves=leaves)
    if grads is not None:
        dc, dd, da = grads
        loss = (c * dc.to(device)).sum()
        if dd is not None:
            loss = loss + (d * dd.to(device)).sum()
        if da is not None:
            loss = loss + (a * da.to(device)).sum()
        loss.backward()
        out["grads"] = {k: v.grad for k, v in leaves.items()}
    torch.cuda.synchronize()
    return out


def run_oracle_inputs(sc, cam, deg, mod, mode):
    """The leaf tensors of `mode` without running the oracle rasterizer."""
    P = sc.means3D.shape[0]
    col_mode, cov_mode = mode.split("_")
    leaves = {"means3D": sc.means3D, "means2D": torch.zeros(P, 3), "opacities": sc.opacities}
    if col_mode == "sh":
        leaves["shs"] = sc.shs
    else:
        dirs = sc.means3D - cam.camera_center[None]
        dirs = dirs / dirs.norm(dim=1, keepdim=True)
        leaves["colors_precomp"] = torch.clamp_min(orc.eval_sh_rgb(deg, sc.shs, dirs) + 0.5, 0.0)
    if cov_mode == "sr":
        leaves["scales"], leaves["rotations"] = sc.scales, sc.rotations
    else:
        leaves["cov3D_precomp"] = orc.cov3d_from_scale_rot(sc.scales, sc.rotations, mod)
    return leaves


def as_u32(t) -> np.ndarray:
    return t.detach().cpu().numpy().astype(np.int64).astype(np.uint32) if t.dtype != torch.int32 else \
        t.detach().cpu().numpy().view(np.uint32)


def gradients_for_fixed_upstream(st, scd, W, H, seed=1):
    """Gradients of sum(color * g0) + sum(depth * g1) + sum(alpha * g2) through the product autograd node (numpy, by input name);
    the upstream g comes from synthetic.make_upstream_grads(seed).  `scd` on the device."""
    from scgaussian_amd import rasterizer as R, synthetic as syn
    dev = scd.means3D.device
    leaves = {k: getattr(scd, k).detach().clone().requires_grad_(True) for k in ("means3D", "shs", "opacities", "scales", "rotations")}
    m2 = torch.zeros_like(leaves["means3D"], requires_grad=True)
    c, radii, d, a = R.GaussianRasterizer(st)(means3D=leaves["means3D"], means2D=m2, opacities=leaves["opacities"],
                                             shs=leaves["shs"], scales=leaves["scales"], rotations=leaves["rotations"])
    g = [t.to(dev) for t in syn.make_upstream_grads(W, H, seed=seed)]
    loss = (c * g[0]).sum() + (d * g[1]).sum() + (a * g[2]).sum()
    loss.backward()
    torch.cuda.synchronize()
    out = {k: v.grad.cpu().numpy() for k, v in leaves.items()}
    out["means2D"] = m2.grad.cpu().numpy()
    return out


def one_call_forward(st, scd):
    """Outputs and saved state of the ONE-CALL forward (scg_forward: the path the bench times) as numpy arrays; `scd` on the
    device.  The capacity of the shape must be known (a staged forward of the same shape ran before)."""
    from scgaussian_amd import rasterizer as R
    out = R.forward_fused(st, scd.means3D, scd.opacities, scd.shs, None, scd.scales, scd.rotations, None, True)
    assert out is not None, "the one-call path did not apply (no capacity known for the shape?)"
    torch.cuda.synchronize()
    c, radii, d, a, state = out
    ws, plan, Rn = state["ws"], state["plan"], int(state["num_rendered"])
    H, W = int(st.image_height), int(st.image_width)
    n_tiles = ((W + 15) // 16) * ((H + 15) // 16)

    def words(off, n, dtype):
        return ws[off: off + 4 * n].view(dtype).cpu().numpy()
    return dict(color=c.cpu().numpy(), depth=d.cpu().numpy(), alpha=a.cpu().numpy(), radii=radii.cpu().numpy(),
                final_T=words(plan.final_T, H * W, torch.float32).reshape(H, W),
                n_contrib=words(plan.n_contrib, H * W, torch.int32).reshape(H, W),
                point_list=words(plan.point_list, Rn, torch.int32).view(np.uint32),
                ranges=words(plan.ranges, 2 * n_tiles, torch.int32).view(np.uint32).reshape(n_tiles, 2),
                num_rendered=np.int64(Rn))


def one_quadrant_scene(P, W, H, seed=0):
    """syn.make_scene with every Gaussian's footprint inside ONE 8x8-pixel quadrant of syn.default_camera's W x H image (W, H
    multiples of 8): centres on quadrant centres, projected sigma <= 0.7 px (log-scale mean -6 + the 0.3 px^2 low-pass filter), so
    alpha falls below 1/255 within 2.3 px of the centre, 1.2 px short of the quadrant's edge.  The blend backward adds one
    floating-point atomic per (Gaussian, quadrant) to the Gaussian's gradient record (DESIGN.md "Determinism"): with a single
    contribution per record the sum has no order, and the gradients of such a scene are bit-reproducible run to run — what a
    test needs that compares two runs with torch.equal."""
    import math
    from scgaussian_amd import synthetic as syn
    assert W % 8 == 0 and H % 8 == 0
    sc = syn.make_scene(P, W, H, seed=seed, log_scale_mean=-6.0)
    g = torch.Generator().manual_seed(seed + 1)
    qx, qy = torch.randint(0, W // 8, (P,), generator=g), torch.randint(0, H // 8, (P,), generator=g)
    tany = math.tan(math.radians(50.0) / 2)
    z = sc.means3D[:, 2]
    # pixel 8 q + 3.5 in normalised device coordinates (pixel = ((ndc + 1) * size - 1) / 2)
    sc.means3D[:, 0] = z * (tany * W / H) * ((16 * qx + 8) / W - 1)
    sc.means3D[:, 1] = z * tany * ((16 * qy + 8) / H - 1)
    return sc


def model_oracle_side(model_cpu, act):
    """Raw CPU leaves, the reference getters on them (autograd), the getters' VALUES replaced by the kernel's activated values
    `act` = (xyz, opacity, scaling, rotation) so that the oracle runs at the very point the kernels run at."""
    from scgaussian_amd import ply_io
    leaves = ply_io.RayBoundModel(**{k: (v.clone().requires_grad_(k not in ("rayo", "rayd")) if isinstance(v, torch.Tensor) else v)
                                     for k, v in model_cpu.__dict__.items()})
    xyz, opa, sca, rot = (a.cpu() for a in act)

    def at(getter, value):
        return getter + (value - getter).detach()
    inputs = dict(means3D=at(leaves.get_xyz, xyz), opacities=at(leaves.get_opacity, opa), scales=at(leaves.get_scaling, sca),
                  rotations=at(leaves.get_rotation, rot), shs=leaves.get_features)
    return leaves, inputs

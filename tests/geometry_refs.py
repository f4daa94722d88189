"""Plain-torch restatement of the per-Gaussian geometry stage (include/scg_raster.h "stage 1" / "stage 5"), any dtype.

Called with torch.float64 it IS the reference of tests/test_gpu_geometry_edges.py; called with torch.float32 it gives the error
of a plain fp32 evaluation of the same expressions (`e32`), from which those tests derive their bar through loss_refs.held_to.
It is a second statement of the stage, written from the header and the kernel's comments in matrix form
(cov2D = T Sigma T^T + 0.3 I with T = J W); oracle/torch_rasterizer.py::preprocess is the first.  tests/test_geometry_refs_cpu.py
holds the two against each other at fp32 and this one's fp64 autograd against central differences.

Constants are the kernel's fp32 constants cast to `dtype` (0.2f, 0.3f, 1e-7f, the SH factors, focal / limit as the host
computes them), so that an fp64 evaluation differs from the kernel by the rounding of the arithmetic alone.  Decisions (near
cull, clamp flags, det != 0, tiles > 0, SH clamp bits) are taken in `dtype` and returned as masks.

`planted()` is the scene the edge tests run on: every class of Gaussian the stage treats differently, at least 16 of each.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from oracle import torch_rasterizer as orc
from scgaussian_amd import synthetic as syn

_f = lambda v: float(np.float32(v))                                   # noqa: E731 - an fp32 constant's value
NEAR_Z, LOWPASS, W_EPS = _f(0.2), _f(0.3), _f(1e-7)
C0, C1 = _f(orc.SH_C0), _f(orc.SH_C1)
C2 = [_f(v) for v in orc.SH_C2]
C3 = [_f(v) for v in orc.SH_C3]
TILE = 16
USED_SLOTS = (0, 1, 2, 3, 4, 5, 6, 8, 9, 10)                           # of the 16-float gradient record; the others are unused
OUTPUTS = {"sh_sr": ("means3D", "opacities", "shs", "scales", "rotations"), "col_sr": ("means3D", "opacities", "colors_precomp", "scales", "rotations"),
           "sh_cov": ("means3D", "opacities", "shs", "cov3D_precomp"), "col_cov": ("means3D", "opacities", "colors_precomp", "cov3D_precomp")}


def _np_sqrt(t):
    """Correctly rounded square root of the values that decide the radius (numpy: the hardware instruction)."""
    return torch.from_numpy(np.sqrt(t.detach().numpy()))


def sh_basis(deg: int, d):
    """(P, (deg+1)^2) real SH basis at unit directions d (P,3), the polynomials and signs of the reference's sh_utils."""
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    b = [torch.full_like(x, C0)]
    if deg > 0:
        b += [-C1 * y, C1 * z, -C1 * x]
    if deg > 1:
        xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
        b += [C2[0] * xy, C2[1] * yz, C2[2] * (2 * zz - xx - yy), C2[3] * xz, C2[4] * (xx - yy)]
        if deg > 2:
            b += [C3[0] * y * (3 * xx - yy), C3[1] * xy * z, C3[2] * y * (4 * zz - xx - yy),
                  C3[3] * z * (2 * zz - 3 * xx - 3 * yy), C3[4] * x * (4 * zz - xx - yy), C3[5] * z * (xx - yy),
                  C3[6] * x * (xx - 3 * yy)]
    return torch.stack(b, 1)


def rotation_matrix(q):
    """(P,3,3) from quaternions (r,x,y,z), NOT normalised here (the stage takes them as given)."""
    r, x, y, z = q.unbind(1)
    rows = [1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
            2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
            2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)]
    return torch.stack(rows, 1).reshape(-1, 3, 3)


def _sym(c6):
    xx, xy, xz, yy, yz, zz = c6.unbind(1)
    return torch.stack([xx, xy, xz, xy, yy, yz, xz, yz, zz], 1).reshape(-1, 3, 3)


def _mm(a, b):
    """Batched small matrix product as broadcast multiply + sum (no BLAS: the same bits on every host)."""
    return (a[:, :, :, None] * b[:, None, :, :]).sum(2)


def camera_constants(cam, dtype):
    W, H = cam.image_width, cam.image_height
    fx, fy, limx, limy = orc.host_scalars(W, H, math.tan(cam.FoVx / 2), math.tan(cam.FoVy / 2))
    return dict(W=W, H=H, fx=fx, fy=fy, limx=limx, limy=limy, V=cam.world_view_transform.to(dtype),
                PM=cam.full_proj_transform.to(dtype), campos=cam.camera_center.to(dtype))


def geometry_forward_ref(inputs, cam, deg, mod, mode, dtype, clamp_off=(), probe=None, cov_offset=None):
    """inputs: dict of the stage's input tensors for `mode` ('sh_sr' | 'col_sr' | 'sh_cov' | 'col_cov') in `dtype` (leaves or not).
    Returns the stage's per-Gaussian outputs (differentiable) and its decisions.  A Gaussian behind the near plane is evaluated
    at a harmless stand-in point so that nothing non-finite enters autograd; every output of a Gaussian with visible == False
    is meaningless and must be masked by the caller.
    clamp_off: subset of ('x', 'y') — the clamped component keeps its VALUE but is differentiated as if it were not clamped
    (what the backward would compute with that flag ignored).  probe: a dict that receives the view-space position `tview`
    (P,3) as a graph node feeding the covariance path and the depth only (the pixel position comes from the projection matrix).
    cov_offset: (P,3) added to the 2D covariance (A, B, C) — the handle finite differences need to take the chain in two legs
    where the projected covariance is tiny next to the 0.3 low-pass term (returned without that term as 'cov2d_raw')."""
    k = camera_constants(cam, dtype)
    W, H, V, PM = k["W"], k["H"], k["V"], k["PM"]
    col_mode, cov_mode = mode.split("_")
    m3 = inputs["means3D"]
    P = m3.shape[0]
    one = torch.ones(P, 1, dtype=dtype)
    with torch.no_grad():
        in_front = (torch.cat([m3, one], 1)[:, :, None] * V[None, :, :3]).sum(1)[:, 2] > NEAR_Z
    stand_in = torch.tensor([0.0, 0.0, 1.0], dtype=dtype) @ torch.linalg.inv(V[:3, :3]) - V[3, :3] @ torch.linalg.inv(V[:3, :3])
    pos = torch.where(in_front[:, None], m3, stand_in[None].expand(P, 3))
    hom = torch.cat([pos, one], 1)
    tview = (hom[:, :, None] * V[None, :, :3]).sum(1)                     # row vector times the (transposed) view matrix
    if probe is not None:
        tview.retain_grad()
        probe["tview"] = tview
    tx, ty, tz = tview.unbind(1)
    clip = (hom[:, :, None] * PM[None]).sum(1)
    m_w = 1.0 / (clip[:, 3] + W_EPS)
    px = ((clip[:, 0] * m_w + 1.0) * W - 1.0) * 0.5
    py = ((clip[:, 1] * m_w + 1.0) * H - 1.0) * 0.5

    if cov_mode == "sr":
        L = rotation_matrix(inputs["rotations"]) * (mod * inputs["scales"])[:, None, :]          # R S
        Sigma = _mm(L, L.transpose(1, 2))
    else:
        Sigma = _sym(inputs["cov3D_precomp"])

    # frustum clamp: a clamped component is a CONSTANT of the backward (no gradient to t.x, none to t.z through the product)
    def clamped(t, lim, off):
        r = t / tz
        cl = ((r < -lim) | (r > lim)).detach()
        val = (torch.clamp(r, -lim, lim) * tz).detach()
        free = t + (val - t).detach()                                       # the value the stage uses, the derivative of t
        return torch.where(cl & (not off), val, free), cl
    t_x, cl_x = clamped(tx, k["limx"], "x" in clamp_off)
    t_y, cl_y = clamped(ty, k["limy"], "y" in clamp_off)
    zero = torch.zeros_like(tz)
    # (tensor / tensor: `float / tensor` is evaluated as reciprocal times float, two roundings)
    J = torch.stack([torch.full_like(tz, k["fx"]) / tz, zero, -(k["fx"] * t_x) / (tz * tz),
                     zero, torch.full_like(tz, k["fy"]) / tz, -(k["fy"] * t_y) / (tz * tz)], 1).reshape(P, 2, 3)
    Wm = V[:3, :3].t()                                                      # world -> view rotation, column-vector form
    T = _mm(J, Wm[None].expand(P, 3, 3))
    cov = _mm(_mm(T, Sigma), T.transpose(1, 2))
    raw_cov = torch.stack([cov[:, 0, 0], cov[:, 0, 1], cov[:, 1, 1]], 1)
    shifted = raw_cov if cov_offset is None else raw_cov + cov_offset
    A, B, C = shifted[:, 0] + LOWPASS, shifted[:, 1], shifted[:, 2] + LOWPASS
    det = A * C - B * B
    det_ok = (det != 0).detach()
    inv = 1.0 / torch.where(det_ok, det, torch.ones_like(det))
    conic = torch.stack([C * inv, -B * inv, A * inv], 1)

    with torch.no_grad():
        mid = 0.5 * (A + C)
        disc = mid * mid - det
        lam1 = mid + _np_sqrt(torch.clamp_min(disc, 0.1))
        radius_f = torch.ceil(3.0 * _np_sqrt(lam1))
        gx, gy = (W + TILE - 1) // TILE, (H + TILE - 1) // TILE

        def rect_of(rad):
            t = lambda v, g: torch.clamp(torch.trunc(v * 0.0625), 0.0, float(g)).to(torch.int32)      # noqa: E731
            return torch.stack([t(px - rad, gx), t(py - rad, gy), t(px + rad + 15.0, gx), t(py + rad + 15.0, gy)], 1)
        rect = rect_of(radius_f)
        tiles = (rect[:, 2] - rect[:, 0]) * (rect[:, 3] - rect[:, 1])
        # the same decision with the radius 0.2 % smaller / larger: a planted Gaussian's tiles > 0 must not hang on that
        tiles_robust = torch.stack([((r[:, 2] - r[:, 0]) * (r[:, 3] - r[:, 1])) > 0
                                    for r in (rect_of(radius_f * 0.998 - 0.01), rect_of(radius_f * 1.002 + 0.01))], 1)
        visible = in_front & det_ok & (tiles > 0)
        radii = torch.where(visible, torch.clamp(radius_f, 0.0, 2.0e9).to(torch.int32), torch.zeros(P, dtype=torch.int32))
        rect = torch.where(visible[:, None], rect, torch.zeros_like(rect))

    if col_mode == "col":
        rgb, raw = inputs["colors_precomp"], None
        sh_clamped = torch.zeros(P, 3, dtype=torch.bool)
    else:
        d = pos - k["campos"][None]
        d = d / torch.sqrt((d * d).sum(1, keepdim=True))
        K = (deg + 1) ** 2
        raw = (sh_basis(deg, d)[:, :, None] * inputs["shs"][:, :K, :]).sum(1) + 0.5
        sh_clamped = (raw < 0).detach()
        rgb = torch.where(sh_clamped, torch.zeros_like(raw), raw)
    return dict(xy=torch.stack([px, py], 1), depth=tz, conic=conic, opacity=inputs["opacities"].reshape(-1), rgb=rgb, raw=raw,
                cov2d=torch.stack([A, B, C], 1), cov2d_raw=raw_cov, disc=disc, radius_f=radius_f, ratio=torch.stack([tx / tz, ty / tz], 1).detach(),
                in_front=in_front, cl_x=cl_x, cl_y=cl_y, det_ok=det_ok, tiles_ok=tiles > 0, tiles_robust=tiles_robust,
                sh_clamped=sh_clamped, visible=visible, radii=radii, rect=rect, grid=(gx, gy))


def coefficients(conic, opacity, records):
    """The per-Gaussian derivative coefficients the header states, from the blend backward's raw sums (P,16): conic detached."""
    a, b, c = conic.detach().unbind(1)
    r = records
    op = opacity.detach()
    return dict(x=-(a * r[:, 0] + b * r[:, 1]), y=-(b * r[:, 0] + c * r[:, 1]), a=-0.5 * r[:, 4], b=-r[:, 5], c=-0.5 * r[:, 6],
                opacity=torch.where(op > 0, r[:, 3] / torch.where(op > 0, op, torch.ones_like(op)), torch.zeros_like(op)),
                depth=r[:, 2], rgb=r[:, 8:11])


def contract_terms(out, k):
    """(P,) <coefficients k, forward outputs> per Gaussian."""
    return k["x"] * out["xy"][:, 0] + k["y"] * out["xy"][:, 1] + k["depth"] * out["depth"] + k["opacity"] * out["opacity"] + \
        (k["rgb"] * out["rgb"]).sum(1) + k["a"] * out["conic"][:, 0] + k["b"] * out["conic"][:, 1] + k["c"] * out["conic"][:, 2]


def contract(out, records, visible):
    """sum over the visible Gaussians of <coefficients, forward outputs>: the scalar whose gradient the stage's backward is.
    `out`: xy, conic, opacity, depth, rgb (this module's forward or the oracle's preprocess).  Returns (scalar, coefficients)."""
    k = coefficients(out["conic"], out["opacity"], records)
    return contract_terms(out, k)[visible.nonzero().reshape(-1)].sum(), k


def _leaves(inputs, mode, dtype):
    return {n: inputs[n].detach().to(dtype).clone().requires_grad_(True) for n in OUTPUTS[mode]}


def _finish(leaves, s, k, visible, W, H, dtype):
    if s.requires_grad:
        s.backward()
    g = {n: (v.grad if v.grad is not None else torch.zeros_like(v)).detach() for n, v in leaves.items()}
    vis = visible.to(dtype)
    g["means2D"] = torch.stack([k["x"] * (0.5 * W) * vis, k["y"] * (0.5 * H) * vis, torch.zeros_like(vis)], 1).detach()
    if "opacities" in g:
        g["opacities"] = g["opacities"].reshape(leaves["opacities"].shape)
    return g


def geometry_backward_ref(inputs, cam, deg, mod, mode, records, dtype, clamp_off=(), probe=None):
    """Gradients of the stage's inputs for the raw sums `records` (P,16; only USED_SLOTS are read): {input name: gradient} +
    'means2D' = (dL/dx_pix 0.5 W, dL/dy_pix 0.5 H, 0) + 'fw' (the forward).  Zero for Gaussians with radius 0."""
    leaves = _leaves(inputs, mode, dtype)
    fw = geometry_forward_ref(leaves, cam, deg, mod, mode, dtype, clamp_off, probe)
    s, k = contract(fw, records.detach().to(dtype), fw["visible"])
    g = _finish(leaves, s, k, fw["visible"], cam.image_width, cam.image_height, dtype)
    g["fw"] = fw
    return g


def oracle_settings(cam, deg, mod):
    return orc.Settings(cam.image_height, cam.image_width, math.tan(cam.FoVx / 2), math.tan(cam.FoVy / 2), torch.zeros(3), mod,
                        cam.world_view_transform, cam.full_proj_transform, deg, cam.camera_center, False, False)


def oracle_preprocess(leaves, cam, deg, mod):
    P = leaves["means3D"].shape[0]
    return orc.preprocess(leaves["means3D"], torch.zeros(P, 3), leaves["opacities"], oracle_settings(cam, deg, mod),
                          **{n: v for n, v in leaves.items() if n not in ("means3D", "opacities")})


def oracle_backward(inputs, cam, deg, mod, mode, records):
    """The same scalar through the fp32 oracle's preprocess and autograd (the kernel's operation order): the second fp32 evaluation."""
    leaves = _leaves(inputs, mode, torch.float32)
    pre = oracle_preprocess(leaves, cam, deg, mod)
    s, k = contract(pre, records.detach().float(), pre["visible"])
    g = _finish(leaves, s, k, pre["visible"], cam.image_width, cam.image_height, torch.float32)
    g["pre"] = pre
    return g


def mode_inputs(sc, cam, deg, mod, mode):
    """The stage's fp32 input tensors of `mode` for a synthetic.Scene (precomputed colours / covariances from the oracle's helpers)."""
    col_mode, cov_mode = mode.split("_")
    d = dict(means3D=sc.means3D, opacities=sc.opacities)
    if col_mode == "sh":
        d["shs"] = sc.shs
    else:
        dirs = sc.means3D - cam.camera_center[None]
        dirs = dirs / dirs.norm(dim=1, keepdim=True)
        d["colors_precomp"] = torch.clamp_min(orc.eval_sh_rgb(deg, sc.shs, dirs) + 0.5, 0.0)
    if cov_mode == "sr":
        d["scales"], d["rotations"] = sc.scales, sc.rotations
    else:
        d["cov3D_precomp"] = orc.cov3d_from_scale_rot(sc.scales, sc.rotations, mod)
    return d


def make_records(P, seed):
    """Seeded raw sums: every used slot non-zero (|v| in 0.5 .. 2) and of mixed sign, the unused slots NaN."""
    g = torch.Generator().manual_seed(seed)
    mag = 0.5 + 1.5 * torch.rand(P, 16, generator=g)
    sign = torch.where(torch.rand(P, 16, generator=g) < 0.5, -1.0, 1.0)
    rec = (mag * sign).float()
    unused = [i for i in range(16) if i not in USED_SLOTS]
    rec[:, unused] = float("nan")
    return rec


def normalise_records(records, g64, names):
    """Scale every Gaussian's record (the backward is linear in it) so that its largest fp64 output gradient is 1."""
    P = records.shape[0]
    big = torch.zeros(P, dtype=torch.float64)
    for n in names:
        big = torch.maximum(big, g64[n].reshape(P, -1).abs().max(1).values)
    scale = torch.where(big > 0, 1.0 / big, torch.ones_like(big))
    # a power of two: the scaled record is exact, and so is the scaling of the gradients that were already computed
    scale = torch.exp2(torch.round(torch.log2(scale)))
    return (records.double() * scale[:, None]).float(), scale


def per_gaussian_error(got, want64):
    """(P,) max_j |got - want| / max_j |want| per Gaussian over its record of one output tensor; 0 where want is all zero and got
    equals it, inf where want is all zero and got is not."""
    P = want64.shape[0]
    d = (got.detach().cpu().double().reshape(P, -1) - want64.reshape(P, -1)).abs().max(1).values
    s = want64.reshape(P, -1).abs().max(1).values
    return torch.where(s > 0, d / torch.where(s > 0, s, torch.ones_like(s)), torch.where(d > 0, torch.full_like(d, float("inf")), d))


# ------------------------------------------------------------------------------------------------------------------ planted set

CLASSES = ("near_on", "inside", "edge_x_on", "edge_x_over", "edge_y_on", "edge_y_over", "clamp_x", "clamp_y", "clamp_xy",
           "clamp_offscreen", "near_over", "lowpass", "lam_floor", "sh_neg", "opacity_edges", "partial")
PER_CLASS = 16
CULLED = ("near_on", "clamp_offscreen")
CLAMPED = ("edge_x_over", "edge_y_over", "clamp_x", "clamp_y", "clamp_xy")
PLANTED_MOD = 1.25                      # the scale modifier the planted scene is rendered with (its scales are designed / 1.25)
SH_TARGETS = ((-0.3, 0.6, 0.4), (0.5, -0.2, 5e-4), (-0.1, -0.4, 0.7), (-0.25, 5e-4, -0.15), (-0.5, -0.05, -0.2), (5e-4, -0.3, 0.2),
              (0.3, 0.2, -0.6), (-0.02, -0.03, -0.04))


class Planted:
    """scene: synthetic.Scene (fp32); cls: list of class names per Gaussian; cam: syn.default_camera(W, H); mod: PLANTED_MOD."""

    def __init__(self, scene, cls, cam):
        self.scene, self.cls, self.cam, self.mod = scene, list(cls), cam, PLANTED_MOD
        self.W, self.H = cam.image_width, cam.image_height

    def members(self, name):
        return torch.tensor([i for i, c in enumerate(self.cls) if c == name], dtype=torch.long)

    def inputs(self, deg, mode):
        return mode_inputs(self.scene, self.cam, deg, self.mod, mode)

    def subset(self, idx):
        """The members `idx` (a LongTensor of indices into the set, repeats allowed) as a planted set of their own."""
        return Planted(syn.Scene(*[t[idx].contiguous() for t in self.scene]), [self.cls[i] for i in idx.tolist()], self.cam)


def planted(W=64, H=48, seed=7):
    cam = syn.default_camera(W, H)
    assert torch.equal(cam.world_view_transform, torch.eye(4))        # t = (x, y, z): x / z hits a threshold exactly for z = 2^k
    f32 = np.float32
    tanx, tany = math.tan(cam.FoVx / 2), math.tan(cam.FoVy / 2)
    fx, fy, limx, limy = (f32(v) for v in orc.host_scalars(W, H, tanx, tany))
    g = torch.Generator().manual_seed(seed)
    rnd = lambda lo, hi: float(lo + (hi - lo) * torch.rand((), generator=g))          # noqa: E731
    rows, cls = [], []

    def add(name, x, y, z, sigma_px, aniso=None, opacity=None, iso=False):
        """One Gaussian at (x, y, z) whose projected sigma is about sigma_px pixels (scale = sigma_px z / focal)."""
        s = float(sigma_px) * float(z) / float(fx)
        ratios = (1.0, 1.0, 1.0) if iso else (aniso or (rnd(0.6, 1.0), rnd(1.0, 1.6), rnd(0.8, 1.2)))
        q = torch.randn(4, generator=g)
        q = q / q.norm()
        rows.append(dict(m=(f32(x), f32(y), f32(z)), s=[s * r / PLANTED_MOD for r in ratios], q=q,
                         o=rnd(0.1, 0.9) if opacity is None else opacity))
        cls.append(name)

    n = PER_CLASS
    sgn = lambda i: 1.0 if i % 2 == 0 else -1.0                                      # noqa: E731
    depth2 = lambda i: (2.0, 4.0, 8.0, 4.0)[(i // 2) % 4]                            # noqa: E731 - powers of two
    for i in range(n):
        z = f32(NEAR_Z)                                                               # z == 0.2f: culled (the test is tz > 0.2)
        add("near_on", rnd(-0.5, 0.5) * tanx * z, rnd(-0.5, 0.5) * tany * z, z, rnd(1.5, 3.0))
    for i in range(n):
        z = rnd(1.5, 9.0)
        add("inside", rnd(-0.9, 0.9) * tanx * z, rnd(-0.9, 0.9) * tany * z, z, rnd(1.0, 6.0))
    for axis in ("x", "y"):
        lim, tan_o = (limx, tany) if axis == "x" else (limy, tanx)
        for over in (False, True):
            for i in range(n):
                z = f32(depth2(i))
                r = f32(sgn(i)) * (np.nextafter(lim, f32(np.inf)) if over else lim)  # x / z == the limit: NOT clamped (strict test)
                a, b = r * z, rnd(-0.7, 0.7) * tan_o * float(z)                     # (r z is exact: z is a power of two)
                assert f32(a) / z == r
                add(f"edge_{axis}_{'over' if over else 'on'}", *((a, b) if axis == "x" else (b, a)), z, rnd(6.0, 7.5))
    # clamped and visible: 1.1 .. 1.5 times the limit; the footprint has to reach back over the image border
    for name in ("clamp_x", "clamp_y", "clamp_xy"):
        for i in range(n):
            z = rnd(2.0, 8.0)
            kx = sgn(i) * rnd(1.1, 1.5) * float(limx) if "x" in name[6:] else rnd(-0.6, 0.6) * tanx
            ky = sgn(i // 2) * rnd(1.1, 1.5) * float(limy) if "y" in name[6:] else rnd(-0.6, 0.6) * tany
            out_px = max(0.5 * W * (abs(kx) / tanx - 1.0), 0.5 * H * (abs(ky) / tany - 1.0))      # centre's distance from the image
            add(name, kx * z, ky * z, z, (out_px + 16.0) / 3.0, aniso=(rnd(0.9, 1.0), rnd(1.0, 1.2), rnd(0.9, 1.1)))
    for i in range(n):
        z = rnd(2.0, 8.0)
        both = i % 4 == 3
        kx = sgn(i) * rnd(1.2, 1.6) * float(limx) if (i % 4 != 1) else rnd(-0.6, 0.6) * tanx
        ky = sgn(i // 2) * rnd(1.2, 1.6) * float(limy) if (i % 4 == 1 or both) else rnd(-0.6, 0.6) * tany
        add("clamp_offscreen", kx * z, ky * z, z, rnd(0.2, 0.6))
    for i in range(n):
        z = np.nextafter(f32(NEAR_Z), f32(1.0))                                       # the first z that is visible
        add("near_over", rnd(-0.6, 0.6) * tanx * z, rnd(-0.6, 0.6) * tany * z, z, rnd(1.5, 3.0))
    for i in range(n):
        z = rnd(1.5, 9.0)
        add("lowpass", rnd(-0.9, 0.9) * tanx * z, rnd(-0.9, 0.9) * tany * z, z, 1.0)
        rows[-1]["s"] = [1e-5 * r for r in (rnd(0.7, 1.0), rnd(1.0, 1.4), 1.0)]     # the 0.3 px^2 term is all of the 2D covariance
    for i in range(n):
        z = rnd(2.0, 8.0)                                                              # near the axis, isotropic: A ~ C, B ~ 0
        add("lam_floor", sgn(i) * rnd(0.0, 0.04) * tanx * z, sgn(i // 2) * rnd(0.0, 0.04) * tany * z, z, rnd(2.0, 6.0), iso=True)
    for i in range(n):
        z = rnd(1.5, 9.0)
        add("sh_neg", rnd(-0.9, 0.9) * tanx * z, rnd(-0.9, 0.9) * tany * z, z, rnd(1.0, 6.0))
    for i in range(n):
        z = rnd(1.5, 9.0)
        add("opacity_edges", rnd(-0.9, 0.9) * tanx * z, rnd(-0.9, 0.9) * tany * z, z, rnd(1.0, 6.0), opacity=(0.0, 1e-6, 1.0)[i % 3])
    for i in range(n):                                                                # centre outside, NOT clamped: the rectangle is clipped
        z = rnd(2.0, 8.0)
        side = i % 8                                                                  # 4 borders, then 4 corners
        kx = {0: -1.15, 1: 1.15, 4: -1.15, 5: 1.15, 6: -1.15, 7: 1.15}.get(side, rnd(-0.5, 0.5)) * tanx
        ky = {2: -1.15, 3: 1.15, 4: -1.15, 5: -1.15, 6: 1.15, 7: 1.15}.get(side, rnd(-0.5, 0.5)) * tany
        add("partial", kx * z, ky * z, z, rnd(4.0, 6.0))

    P = len(rows)
    means = torch.tensor(np.array([r["m"] for r in rows], dtype=np.float32))
    scales = torch.tensor([r["s"] for r in rows], dtype=torch.float32)
    rot = torch.stack([r["q"] for r in rows]).float()
    opac = torch.tensor([[r["o"]] for r in rows], dtype=torch.float32)
    dc = torch.rand(P, 1, 3, generator=g) * 1.5 - 0.3
    rest = torch.randn(P, 15, 3, generator=g) * 0.1
    shs = torch.cat([dc, rest], 1).contiguous()
    # sh_neg: the DC term is solved for (in fp64) so that the degree-3 colour lands on the targets — one, two, three channels
    # below 0 by at least 0.02, and channels 5e-4 ABOVE 0 that must not be clamped
    ids = [i for i, c in enumerate(cls) if c == "sh_neg"]
    d = means[ids].double() - cam.camera_center.double()[None]
    d = d / d.norm(dim=1, keepdim=True)
    basis = sh_basis(3, d)
    higher = (basis[:, 1:, None] * shs[ids, 1:].double()).sum(1)
    tgt = torch.tensor([SH_TARGETS[j % len(SH_TARGETS)] for j in range(len(ids))], dtype=torch.float64)
    shs[ids, 0] = ((tgt - 0.5 - higher) / C0).float()
    return Planted(syn.Scene(means.contiguous(), scales.contiguous(), rot.contiguous(), opac.contiguous(), shs), cls, cam)


def assert_premises(pl, fw64, deg=3):
    """Every planted class asserts what it was planted for, from the fp64 forward `fw64` of (sh_sr, degree 3)."""
    k = camera_constants(pl.cam, torch.float64)
    lim = torch.tensor([k["limx"], k["limy"]], dtype=torch.float64)
    rel = (fw64["ratio"].abs() / lim[None] - 1.0)                                   # > 0: beyond the limit
    for name in CLASSES:
        m = pl.members(name)
        assert len(m) >= PER_CLASS, name
        vis, cx, cy = fw64["visible"][m], fw64["cl_x"][m], fw64["cl_y"][m]
        assert bool((fw64["radii"][m] > 0).eq(vis).all())
        if name in CULLED:
            assert not bool(vis.any()), name
        else:
            assert bool(vis.all()), (name, vis)
            assert bool(fw64["tiles_robust"][m].all()), name
        if name == "near_on":
            assert bool((pl.scene.means3D[m, 2].double() == NEAR_Z).all()) and not bool(fw64["in_front"][m].any())
        elif name == "near_over":
            assert bool((fw64["depth"][m] == float(np.nextafter(np.float32(NEAR_Z), np.float32(1)))).all())
        else:
            assert bool((fw64["depth"][m] > 1.0).all()), name
        if name.startswith("edge_"):
            ax = 0 if name[5] == "x" else 1
            over = name.endswith("over")
            want = float(np.nextafter(np.float32(lim[ax]), np.float32(np.inf))) if over else float(lim[ax])
            assert bool((fw64["ratio"][m, ax].abs() == want).all()), name
            assert bool(((cx if ax == 0 else cy) == over).all()) and not bool((cy if ax == 0 else cx).any()), name
            assert bool((fw64["ratio"][m, ax] > 0).any()) and bool((fw64["ratio"][m, ax] < 0).any()), name
            assert bool((rel[m, 1 - ax] < -1e-3).all())
        else:
            assert bool((rel[m].abs() > 1e-3).all()), name                          # no clamp decision near flipping
            want_x = name in ("clamp_x", "clamp_xy")
            want_y = name in ("clamp_y", "clamp_xy")
            if name == "clamp_offscreen":
                assert bool((cx | cy).all()) and not bool(fw64["tiles_ok"][m].any()) and not bool(fw64["tiles_robust"][m].any())
            else:
                assert bool((cx == want_x).all()) and bool((cy == want_y).all()), name
        if name == "lowpass":
            assert bool(((fw64["cov2d"][m][:, [0, 2]] - LOWPASS).abs() < 1e-3 * LOWPASS).all())
        if name == "lam_floor":
            assert bool((fw64["disc"][m] < 0.09).all()) and bool((fw64["cov2d"][m][:, 0] > 2.0).all())
        if name not in CULLED:
            assert bool(((fw64["disc"][m] - 0.1).abs() > 1e-3).all()), (name, fw64["disc"][m])   # the 0.1 floor of lam1: not near flipping
        if name == "sh_neg":
            n_neg = fw64["sh_clamped"][m].sum(1)
            assert set(n_neg.tolist()) == {1, 2, 3}
            raw = fw64["raw"][m]
            assert bool((raw[fw64["sh_clamped"][m]] < -1e-3).all())
            just = (raw > 0) & (raw < 1e-3)
            assert int(just.sum()) >= 3 and bool((raw[just] > 1e-4).all())
        if name == "opacity_edges":
            assert set(fw64["opacity"][m].float().tolist()) == {0.0, float(np.float32(1e-6)), 1.0}
        if name == "partial":
            r = fw64["rect"][m]
            gx, gy = fw64["grid"]
            xy = fw64["xy"][m]
            outside = (xy[:, 0] < 0) | (xy[:, 0] > pl.W - 1) | (xy[:, 1] < 0) | (xy[:, 1] > pl.H - 1)
            assert bool(outside.all())
            assert bool((r[:, 0] == 0).any()) and bool((r[:, 2] == gx).any()) and bool((r[:, 1] == 0).any()) and bool((r[:, 3] == gy).any())
            corner = ((xy[:, 0] < 0) | (xy[:, 0] > pl.W - 1)) & ((xy[:, 1] < 0) | (xy[:, 1] > pl.H - 1))
            assert int(corner.sum()) >= 4


def sh_margin(fw):
    """Smallest |colour before the clamp| over the visible Gaussians: how far every SH clamp bit is from flipping."""
    return float(fw["raw"][fw["visible"]].abs().min())

"""fp64 numpy restatement of the camera-gradient rule (include/camgrad/scg_camgrad.h): from (inputs, camera, gradient
records, radii) to the 35 numbers dL/dviewmatrix (16) | dL/dprojmatrix (16) | dL/dcampos (3).

Written from the header in MATRIX form (T = J W, cov2D = T Sigma T^T + 0.3 I, conic = cov2D^-1, dL/dcov2D = -Q G Q), not from the
kernel's scalar chain, in numpy and without autograd: a second statement of the rule.  oracle/torch_rasterizer.py's autograd with
the three camera tensors as leaves is the first; tests/test_camgrad_cpu.py holds the two against each other, and mutants of this
one against the oracle.  Constants are the kernel's fp32 constants; decisions (the 1.3 tanfov clamp, the colour clamp) are taken in
fp64 from the fp32 inputs, visibility is an INPUT (radii > 0).

Also here: the map from the oracle's per-Gaussian gradients (dL/dxy, dL/dconic, dL/dopacity, dL/ddepth, dL/drgb) to the raw-sum
records the blend backward leaves, and the oracle-side drivers the CPU and GPU tests share.
"""
from __future__ import annotations

import importlib.util
import math
import os

import numpy as np
import torch

import geometry_refs as G
from oracle import torch_rasterizer as orc

MUTANTS = ("clamped_dtx_let_through", "channel_clamp_ignored", "dead_column_written", "invisible_summed")
DEAD = np.array([3, 7, 11, 15, 16 + 2, 16 + 6, 16 + 10, 16 + 14])              # the output words that are always zero


def _np(t, dtype=np.float64):
    return (t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)).astype(dtype)


def camera_of(cam):
    """The camera's numbers as the rule takes them: fp32 values in fp64, the host scalars as oracle.host_scalars forms them."""
    W, H = int(cam.image_width), int(cam.image_height)
    fx, fy, limx, limy = orc.host_scalars(W, H, math.tan(cam.FoVx / 2), math.tan(cam.FoVy / 2))
    return dict(W=W, H=H, fx=fx, fy=fy, limx=limx, limy=limy, V=_np(cam.world_view_transform).reshape(4, 4),
                PM=_np(cam.full_proj_transform).reshape(4, 4), campos=_np(cam.camera_center).reshape(3))


def _basis_and_jacobian(deg, d):
    """B (P,K) and dB/ddir (P,K,3) of the real SH basis at unit directions d (P,3): utils/sh_utils.py's polynomials."""
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    o, zero = np.ones_like(x), np.zeros_like(x)
    C0, C1, C2, C3 = G.C0, G.C1, G.C2, G.C3
    rows = [(C0 * o, zero, zero, zero)]
    if deg > 0:
        rows += [(-C1 * y, zero, -C1 * o, zero), (C1 * z, zero, zero, C1 * o), (-C1 * x, -C1 * o, zero, zero)]
    if deg > 1:
        rows += [(C2[0] * x * y, C2[0] * y, C2[0] * x, zero),
                 (C2[1] * y * z, zero, C2[1] * z, C2[1] * y),
                 (C2[2] * (2 * z * z - x * x - y * y), -2 * C2[2] * x, -2 * C2[2] * y, 4 * C2[2] * z),
                 (C2[3] * x * z, C2[3] * z, zero, C2[3] * x),
                 (C2[4] * (x * x - y * y), 2 * C2[4] * x, -2 * C2[4] * y, zero)]
    if deg > 2:
        rows += [(C3[0] * y * (3 * x * x - y * y), 6 * C3[0] * x * y, C3[0] * (3 * x * x - 3 * y * y), zero),
                 (C3[1] * x * y * z, C3[1] * y * z, C3[1] * x * z, C3[1] * x * y),
                 (C3[2] * y * (4 * z * z - x * x - y * y), -2 * C3[2] * x * y, C3[2] * (4 * z * z - x * x - 3 * y * y), 8 * C3[2] * y * z),
                 (C3[3] * z * (2 * z * z - 3 * x * x - 3 * y * y), -6 * C3[3] * x * z, -6 * C3[3] * y * z,
                  C3[3] * (6 * z * z - 3 * x * x - 3 * y * y)),
                 (C3[4] * x * (4 * z * z - x * x - y * y), C3[4] * (4 * z * z - 3 * x * x - y * y), -2 * C3[4] * x * y, 8 * C3[4] * x * z),
                 (C3[5] * z * (x * x - y * y), 2 * C3[5] * x * z, -2 * C3[5] * y * z, C3[5] * (x * x - y * y)),
                 (C3[6] * x * (x * x - 3 * y * y), C3[6] * (3 * x * x - 3 * y * y), -6 * C3[6] * x * y, zero)]
    B = np.stack([r[0] for r in rows], 1)
    J = np.stack([np.stack(r[1:], 1) for r in rows], 1)
    return B, J


def camera_rule(inputs, cam, deg, mod, records, radii, mutant=None, want_campos=True, per_gaussian=False):
    """The 35 numbers (fp64).  inputs: {means3D, shs | colors_precomp, scales + rotations | cov3D_precomp} (tensors or arrays; the
    opacities are not the camera's); cam: camera_of(...) or a dict like it; records (P,16) raw sums; radii (P,).
    per_gaussian: the (P,35) contributions instead of their sum; per_gaussian = "scale": the (P,35) MAGNITUDES of what is added up
    to form each contribution — |contribution| itself for the two matrices, and for campos, whose contribution is the small
    remainder -(g - u (u . g)) / |d| of the larger g = sum_k (sh_k . dRGB) dB_k/ddir, the magnitudes of those products:
    (sum_k |sh_k . dRGB| |dB_k/ddir| + |u| (|u| . the same)) / |d|.  An fp32 evaluation rounds each of these products, so its
    error is relative to them and not to the remainder."""
    k = cam if isinstance(cam, dict) else camera_of(cam)
    V, PM, W, H = k["V"], k["PM"], k["W"], k["H"]
    x = _np(inputs["means3D"])
    P = x.shape[0]
    rec = _np(records)
    vis = np.ones(P, dtype=bool) if mutant == "invisible_summed" else (_np(radii, np.int64) > 0)
    out = np.zeros((P, 35))
    if P == 0:
        return out if per_gaussian else out.sum(0)
    with np.errstate(all="ignore"):
        pos = np.concatenate([x, np.ones((P, 1))], 1)
        t = pos @ V                                                            # t_i = sum_j V[4j+i] pos[j]
        h = pos @ PM
        tx, ty, tz = t[:, 0], t[:, 1], t[:, 2]
        m_w = 1.0 / (h[:, 3] + G.W_EPS)
        if "cov3D_precomp" in inputs and inputs["cov3D_precomp"] is not None:
            c6 = _np(inputs["cov3D_precomp"])
            Sigma = np.stack([c6[:, 0], c6[:, 1], c6[:, 2], c6[:, 1], c6[:, 3], c6[:, 4], c6[:, 2], c6[:, 4], c6[:, 5]], 1).reshape(P, 3, 3)
        else:
            q, s = _np(inputs["rotations"]), _np(inputs["scales"]) * float(mod)
            r, qx, qy, qz = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
            R = np.stack([1 - 2 * (qy * qy + qz * qz), 2 * (qx * qy - r * qz), 2 * (qx * qz + r * qy),
                          2 * (qx * qy + r * qz), 1 - 2 * (qx * qx + qz * qz), 2 * (qy * qz - r * qx),
                          2 * (qx * qz - r * qy), 2 * (qy * qz + r * qx), 1 - 2 * (qx * qx + qy * qy)], 1).reshape(P, 3, 3)
            L = R * s[:, None, :]
            Sigma = L @ L.transpose(0, 2, 1)
        rx, ry = tx / tz, ty / tz
        cl_x, cl_y = (rx < -k["limx"]) | (rx > k["limx"]), (ry < -k["limy"]) | (ry > k["limy"])
        t_x, t_y = np.clip(rx, -k["limx"], k["limx"]) * tz, np.clip(ry, -k["limy"], k["limy"]) * tz
        J = np.zeros((P, 2, 3))
        J[:, 0, 0], J[:, 0, 2] = k["fx"] / tz, -k["fx"] * t_x / (tz * tz)
        J[:, 1, 1], J[:, 1, 2] = k["fy"] / tz, -k["fy"] * t_y / (tz * tz)
        Wm = V[:3, :3].T                                                       # Wm[i][j] = V[4j+i]
        T = J @ Wm
        cov = T @ Sigma @ T.transpose(0, 2, 1)
        cov[:, 0, 0] += G.LOWPASS
        cov[:, 1, 1] += G.LOWPASS
        Q = np.linalg.inv(np.where(np.isfinite(cov), cov, 0.0) + np.where(vis, 0.0, 1.0)[:, None, None] * np.eye(2)[None])
        a, b, c = Q[:, 0, 0], Q[:, 0, 1], Q[:, 1, 1]
        # the records' raw sums -> the gradients of the splat's centre, conic and depth
        d_x, d_y = -(a * rec[:, 0] + b * rec[:, 1]), -(b * rec[:, 0] + c * rec[:, 1])
        Gq = np.zeros((P, 2, 2))                                               # dL/dQ as a symmetric matrix (b stands at two places)
        Gq[:, 0, 0], Gq[:, 1, 1] = -0.5 * rec[:, 4], -0.5 * rec[:, 6]
        Gq[:, 0, 1] = Gq[:, 1, 0] = 0.5 * -rec[:, 5]
        Gm = -Q @ Gq @ Q                                                       # dL/dcov2D (symmetric)
        dT = 2.0 * Gm @ T @ Sigma                                              # cov2D = T Sigma T^T
        dJ = dT @ Wm.T
        dWm = J.transpose(0, 2, 1) @ dT                                        # (P,3,3): dL/dWm[i][j]
        itz2, itz3 = 1.0 / (tz * tz), 1.0 / (tz * tz * tz)
        dtx = np.where(cl_x & (mutant != "clamped_dtx_let_through"), 0.0, -k["fx"] * itz2 * dJ[:, 0, 2])
        dty = np.where(cl_y, 0.0, -k["fy"] * itz2 * dJ[:, 1, 2])
        dtz = -k["fx"] * itz2 * dJ[:, 0, 0] - k["fy"] * itz2 * dJ[:, 1, 1] + 2 * k["fx"] * t_x * itz3 * dJ[:, 0, 2] + \
            2 * k["fy"] * t_y * itz3 * dJ[:, 1, 2] + rec[:, 2]
        dV = np.zeros((P, 4, 4))
        dV[:, :, :3] = pos[:, :, None] * np.stack([dtx, dty, dtz], 1)[:, None, :]
        dV[:, :3, :3] += dWm.transpose(0, 2, 1)                                # dV[4j+i] += dWm[i][j]
        dndc_x, dndc_y = d_x * 0.5 * W, d_y * 0.5 * H
        dh = np.stack([dndc_x * m_w, dndc_y * m_w, np.zeros(P), -(h[:, 0] * dndc_x + h[:, 1] * dndc_y) * m_w * m_w], 1)
        dPM = pos[:, :, None] * dh[:, None, :]
        if mutant == "dead_column_written":
            dV[:, :, 3] = pos * dtz[:, None]
            dPM[:, :, 2] = pos * dh[:, 3:4]
        dcam = np.zeros((P, 3))
        if want_campos and inputs.get("shs") is not None and deg > 0:
            K = (deg + 1) ** 2
            sh = _np(inputs["shs"])[:, :K]
            d = x - k["campos"][None]
            ln = np.sqrt((d * d).sum(1, keepdims=True))
            u = d / ln
            B, dB = _basis_and_jacobian(deg, u)
            raw = (B[:, :, None] * sh).sum(1) + 0.5
            keep = np.ones_like(raw, dtype=bool) if mutant == "channel_clamp_ignored" else ~(raw < 0)
            dRGB = rec[:, 8:11] * keep
            g = ((sh * dRGB[:, None, :]).sum(2)[:, :, None] * dB).sum(1)       # dL/ddir
            dcam = -(g - u * (u * g).sum(1, keepdims=True)) / ln               # through dir = d / |d|, and d = mean - campos
            if per_gaussian == "scale":
                ga = (np.abs((sh * dRGB[:, None, :]).sum(2))[:, :, None] * np.abs(dB)).sum(1)
                dcam = (ga + np.abs(u) * (np.abs(u) * ga).sum(1, keepdims=True)) / ln
        out = np.concatenate([dV.reshape(P, 16), dPM.reshape(P, 16), dcam], 1)
        if per_gaussian == "scale":
            out = np.abs(out)
        out = np.where(vis[:, None], out, 0.0)
    return out if per_gaussian else out.sum(0)


def split(out35):
    o = np.asarray(out35)
    return o[0:16].reshape(4, 4), o[16:32].reshape(4, 4), o[32:35]


def records_from_oracle(conic, opacity, d_xy, d_conic, d_opacity, d_depth, d_rgb):
    """(P,16) raw-sum records from the oracle's per-Gaussian gradients:  S = -conic^-1 dL/dxy,  S_xx = -2 dL/da,  S_xy = -dL/db,
    S_yy = -2 dL/dc,  S_q = opacity dL/dopacity,  [2] = dL/ddepth,  [8..10] = dL/drgb.  Unused slots NaN."""
    conic, opacity, d_xy, d_conic, d_opacity, d_depth, d_rgb = (_np(t) for t in (conic, opacity, d_xy, d_conic, d_opacity, d_depth, d_rgb))
    P = conic.shape[0]
    rec = np.full((P, 16), np.nan)
    a, b, c = conic[:, 0], conic[:, 1], conic[:, 2]
    det = a * c - b * b
    ok = det != 0
    di = 1.0 / np.where(ok, det, 1.0)
    rec[:, 0] = np.where(ok, -(c * d_xy[:, 0] - b * d_xy[:, 1]) * di, 0.0)
    rec[:, 1] = np.where(ok, -(-b * d_xy[:, 0] + a * d_xy[:, 1]) * di, 0.0)
    rec[:, 2] = d_depth.reshape(P)
    rec[:, 3] = opacity.reshape(P) * d_opacity.reshape(P)
    rec[:, 4], rec[:, 5], rec[:, 6] = -2.0 * d_conic[:, 0], -d_conic[:, 1], -2.0 * d_conic[:, 2]
    rec[:, 8:11] = d_rgb
    return rec


# ---- the oracle's side -------------------------------------------------------------------------------------------------------------
def camera_leaves(cam, dtype=torch.float32):
    return [t.detach().clone().to(dtype).requires_grad_(True) for t in (cam.world_view_transform, cam.full_proj_transform, cam.camera_center)]


def oracle_settings(cam, deg, mod, leaves, bg=(0.0, 0.0, 0.0)):
    return orc.Settings(cam.image_height, cam.image_width, math.tan(cam.FoVx / 2), math.tan(cam.FoVy / 2),
                        torch.tensor(bg, dtype=torch.float32), mod, leaves[0], leaves[1], deg, leaves[2], False, False)


def _grads35(leaves):
    return np.concatenate([(_np(t.grad) if t.grad is not None else np.zeros(tuple(t.shape))).reshape(-1) for t in leaves])


def oracle_preprocess_camera_grads(inputs, cam, deg, mod, records):
    """The fp32 oracle's autograd gradients of the three camera tensors for planted records: the scalar
    sum_visible <coefficients(records), preprocess outputs> (geometry_refs.contract) differentiated by them.  Returns (35 fp64
    values of the fp32 gradients, the oracle's preprocess dict)."""
    leaves = camera_leaves(cam)
    P = inputs["means3D"].shape[0]
    kw = {n: v.detach().float() for n, v in inputs.items() if n not in ("means3D", "opacities") and v is not None}
    pre = orc.preprocess(inputs["means3D"].detach().float(), torch.zeros(P, 3), inputs["opacities"].detach().float(),
                         oracle_settings(cam, deg, mod, leaves), **kw)
    s, _k = G.contract(pre, torch.nan_to_num(torch.as_tensor(records).float()), pre["visible"])
    if s.requires_grad:
        s.backward()
    return _grads35(leaves), pre


def oracle_rasterize_camera_grads(inputs, cam, deg, mod, upstream, bg=(0.1, 0.2, 0.3)):
    """The full oracle rasterizer differentiated by the camera, taken in two legs so that the per-Gaussian gradients BETWEEN the
    legs are in hand: the blend differentiated by its per-Gaussian inputs (these map to the records), then preprocess
    differentiated by the camera with those as the upstream — the chain rule autograd applies to rasterize() in one piece.
    Returns (35 values of rasterize() in ONE piece, the records, radii)."""
    leaves = camera_leaves(cam)
    P = inputs["means3D"].shape[0]
    kw = {n: v.detach().float() for n, v in inputs.items() if n not in ("means3D", "opacities") and v is not None}
    st = oracle_settings(cam, deg, mod, leaves, bg)
    pre = orc.preprocess(inputs["means3D"].detach().float(), torch.zeros(P, 3), inputs["opacities"].detach().float(), st, **kw)
    names = ("xy", "conic", "depth", "rgb", "opacity")
    cut = dict(pre)
    for n in names:
        cut[n] = pre[n].detach().clone().requires_grad_(True)
    binning = orc.bin_and_sort(pre, int(cam.image_width), int(cam.image_height))
    c, d, a, _ft, _nc = orc.blend(cut, binning, st)
    ((c * upstream[0]).sum() + (d * upstream[1]).sum() + (a * upstream[2]).sum()).backward()
    g = {n: (cut[n].grad if cut[n].grad is not None else torch.zeros_like(cut[n])) for n in names}
    rec = records_from_oracle(pre["conic"], pre["opacity"], g["xy"], g["conic"], g["opacity"], g["depth"], g["rgb"])
    through = [n for n in names if pre[n].requires_grad]
    torch.autograd.backward([pre[n] for n in through], [g[n] for n in through])
    two_legs = _grads35(leaves)
    # ... and in one piece: rasterize() with the camera tensors as leaves, what a caller of the oracle gets
    whole = camera_leaves(cam)
    c, _r, d, a = orc.rasterize(inputs["means3D"].detach().float(), torch.zeros(P, 3), inputs["opacities"].detach().float(),
                                oracle_settings(cam, deg, mod, whole, bg), **kw)
    ((c * upstream[0]).sum() + (d * upstream[1]).sum() + (a * upstream[2]).sum()).backward()
    one_piece = _grads35(whole)
    assert np.allclose(two_legs, one_piece, rtol=1e-4, atol=1e-6 * np.abs(one_piece).max()), (two_legs, one_piece)
    return one_piece, rec, pre["radii"]


# ---- pose recovery: examples/fit_pose.py's loop with the oracle in place of the kernels ---------------------------------------------
def fit_pose_module():
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "fit_pose.py")
    spec = importlib.util.spec_from_file_location("fit_pose", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def rasterize_oracle(cam, sc, bg, deg=3):
    st = orc.Settings(cam.image_height, cam.image_width, math.tan(cam.FoVx / 2), math.tan(cam.FoVy / 2), bg, 1.0,
                      cam.world_view_transform, cam.full_proj_transform, deg, cam.camera_center, False, False)
    return orc.rasterize(sc.means3D, torch.zeros_like(sc.means3D), sc.opacities, st, shs=sc.shs, scales=sc.scales, rotations=sc.rotations)[0]

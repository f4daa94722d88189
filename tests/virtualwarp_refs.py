"""Restatements of the virtual-view warp loss and the depth smoothness (scgaussian_amd/virtual.py, include/vw/scg_virtualwarp.h)
for the tests: the reference-shaped torch expression in any dtype (fp32 on the CPU: the reference's own arithmetic, whose deviation
from its fp64 run is e_ref) and, with `records`, the fp64 restatement of the header's rule on the composed matrices the kernels are
given (the truth they are held to), both with gradients by autograd; an analytic fp64 gradient of the window term with the
reflection fold written out; the near-tie sets; scenes.  Own code, no kernel.
"""
import os

import numpy as np
import torch
import torch.nn.functional as F

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_virtualwarp.npz")
KEYS = ("virtual_img", "virtual_depth", "vir_c2w", "intrs", "w2cs", "img_colors", "vir_mask")
TIE = 16.0                   # a quantity within TIE * e_ref of a decision's edge is a near tie
MARGIN = 4.0                 # the project's standing margin on e_ref
f32 = np.float32


# ---- scenes ---------------------------------------------------------------------------------------------------------------------
def _rot(axis_angle):
    a = np.asarray(axis_angle, dtype=np.float64)
    th = np.linalg.norm(a)
    if th == 0:
        return np.eye(3)
    k = a / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def _texture(rng, C, H, W, waves=3):
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    out = np.full((C, H, W), 0.5)
    for c in range(C):
        for _ in range(waves):
            fx, fy, ph = rng.uniform(-0.9, 0.9), rng.uniform(-0.9, 0.9), rng.uniform(0, 6.28)
            out[c] += 0.12 * np.sin(fx * xx + fy * yy + ph)
    return np.clip(out + rng.uniform(-0.02, 0.02, out.shape), 0.02, 0.98)


def make_scene(H, W, nv, seed, shift=0.06, tilt=0.02):
    """A smooth textured scene: nv cameras a small rotation and translation away from a virtual one, depths around 3."""
    rng = np.random.default_rng(seed)
    f = 1.1 * max(H, W)
    K = np.array([[f, 0, W / 2.0], [0, f * 1.05, H / 2.0], [0, 0, 1]])
    intrs, w2cs = [], []
    for _ in range(nv):
        k = K.copy()
        k[0, 0] *= rng.uniform(0.97, 1.03)
        k[1, 1] *= rng.uniform(0.97, 1.03)
        e = np.eye(4)
        e[:3, :3] = _rot(rng.uniform(-tilt, tilt, 3))
        e[:3, 3] = rng.uniform(-shift, shift, 3)
        intrs.append(k)
        w2cs.append(e)
    c2w = np.eye(4)
    c2w[:3, :3] = _rot(rng.uniform(-tilt, tilt, 3))
    c2w[:3, 3] = rng.uniform(-shift, shift, 3)
    base = _texture(rng, 3, H, W)
    colors = np.stack([np.clip(base + 0.3 * (_texture(rng, 3, H, W) - 0.5), 0.02, 0.98) for _ in range(nv)])
    img = np.clip(base + 0.3 * (_texture(rng, 3, H, W) - 0.5), 0.02, 0.98)
    depth = 3.0 + 0.6 * (_texture(rng, 1, H, W)[0] - 0.5)
    mask = rng.uniform(size=(H, W)) > 0.1
    return {"virtual_img": img.astype(f32), "virtual_depth": depth.astype(f32), "vir_c2w": c2w[:3].astype(f32),
            "intrs": np.stack(intrs).astype(f32), "w2cs": np.stack(w2cs).astype(f32), "img_colors": colors.astype(f32),
            "vir_mask": mask}


def exact_scene(H, W, nv=1, shift_px=0.0, depth=2.0):
    """Cameras whose whole projection is exact in fp32 AND fp64: K = [[4,0,cx],[0,4,cy]] with integer cx, cy, no rotation, a
    translation along x of shift_px * depth / 4 (a multiple of 1/8 px for dyadic arguments).  Pixel (px, py) lands on
    (px + shift_px, py) exactly."""
    s = make_scene(H, W, nv, seed=H * 131 + W)
    K = np.array([[4.0, 0, W // 2], [0, 4.0, H // 2], [0, 0, 1]], dtype=f32)
    s["intrs"] = np.stack([K] * nv)
    e = np.eye(4, dtype=f32)
    s["w2cs"] = np.stack([e] * nv).copy()
    s["w2cs"][:, 0, 3] = f32(shift_px * depth / 4.0)
    s["vir_c2w"] = np.eye(4, dtype=f32)[:3].copy()
    s["virtual_depth"] = np.full((H, W), depth, dtype=f32)
    s["vir_mask"] = np.ones((H, W), dtype=bool)
    return s


# (H, W, nv, seed) of the scene the non-finite image values are planted in, and the cases: tensor, element, value.  Pixel (8, 7) is
# interior (its 5x5 windows reach no border), three views see it, and texel (8, 7) of view 1 lies under the taps of two pixels.
NONFINITE_SCENE = (17, 15, 3, 28)
NONFINITE_CASES = {"img_nan": ("virtual_img", (1, 8, 7), np.nan), "img_pinf": ("virtual_img", (1, 8, 7), np.inf),
                   "img_ninf": ("virtual_img", (1, 8, 7), -np.inf), "colors_nan": ("img_colors", (1, 1, 8, 7), np.nan),
                   "colors_pinf": ("img_colors", (1, 1, 8, 7), np.inf)}
# (H, W): seed of the one-view scenes with 255, 256 and 272 tiles of 16 x 16 (the last with a partial tile row)
LARGE_SCENES = {(240, 272): 2, (256, 256): 1, (241, 272): 4}


def nonfinite_scene(case, variant, records):
    """(scene, affected): one value of NONFINITE_CASES planted; affected (H,W): the pixels with a NaN s_v in some view that sees them, by the fp64
    restatement on `records`.  variant "inside": the mask keeps every affected pixel; "masked_out": it removes them all."""
    H, W, nv, seed = NONFINITE_SCENE
    sc = make_scene(H, W, nv, seed)
    key, at, value = NONFINITE_CASES[case]
    sc[key][at] = value
    with np.errstate(invalid="ignore"):
        r = warp_reference(sc, grads=False, records=records)
    affected = (np.isnan(r["s"]) & r["in_bounds"]).any(axis=0)
    sc["vir_mask"] = (sc["vir_mask"] | affected) if variant == "inside" else (sc["vir_mask"] & ~affected)
    return sc, affected


def tensors(scene, dtype=torch.float32, device="cpu"):
    out = {k: torch.from_numpy(np.ascontiguousarray(scene[k])) for k in KEYS}
    return {k: (v.to(device) if v.dtype == torch.bool else v.to(device, dtype)) for k, v in out.items()}


# ---- the reference-shaped expression ---------------------------------------------------------------------------------------------
def ssim_terms(x, y):
    """(raw, clamped): (1 - n / d) / 2 per channel with 5x5 box means behind a reflection pad of 2.  x (1,3,H,W), y (nv,3,H,W)."""
    pool = lambda t: F.avg_pool2d(F.pad(t, (2, 2, 2, 2), mode="reflect"), 5, 1)      # noqa: E731
    mu_x, mu_y = pool(x), pool(y)
    sig_x, sig_y, sig_xy = pool(x ** 2) - mu_x ** 2, pool(y ** 2) - mu_y ** 2, pool(x * y) - mu_x * mu_y
    n = (2 * mu_x * mu_y + 0.01 ** 2) * (2 * sig_xy + 0.03 ** 2)
    d = (mu_x ** 2 + mu_y ** 2 + 0.01 ** 2) * (sig_x + sig_y + 0.03 ** 2)
    raw = (1 - n / d) / 2
    return raw, torch.clamp(raw, 0, 1)


def warp_reference(scene, dtype=torch.float64, upstream=1.0, grads=True, records=None, eps=1e-8, sampler=False):
    """The loss as the reference's function shapes it (unprojection through K_0^-1, the virtual pose, each view's w2c and K, one
    matrix product after the other; grid_sample; SSIM; the 1000 marker; min over views), in `dtype` on the CPU.  Returns a dict of
    numpy arrays: loss, d_img, d_depth (for loss * upstream), loss_map, winner, in_bounds, s (nv,H,W) before the marker, raw
    (nv,3,H,W), norm (nv,2,H,W), tap (nv,2,H,W).
    records (nv,12): THE RESTATEMENT of the rule the header states — (X, Y, Z) = d * (M_v (px, py, 1)) + t_v from the composed
    matrices the kernels are given, everything behind it the same; eps: the 1e-8 of the division (0 where fp32 absorbs it).
    sampler (with grads): also "dyd" (nv,3,H,W), d warp[v,c](q) / d depth(q) by autograd of the projection and the sampler ALONE
    (a pixel's sample depends on that pixel's depth only, so the gradient of a channel's sum is the per-pixel derivative)."""
    t = tensors(scene, dtype)
    img, depth = t["virtual_img"].requires_grad_(grads), t["virtual_depth"].requires_grad_(grads)
    H, W = img.shape[1:]
    nv = t["intrs"].shape[0]
    pose = torch.eye(4, dtype=dtype)
    pose[:3] = t["vir_c2w"]
    ys, xs = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    xs, ys = xs.reshape(-1).to(dtype), ys.reshape(-1).to(dtype)
    if records is None:
        rays = torch.stack([xs, ys, torch.ones_like(xs)]) * depth.reshape(1, -1)
        pts = torch.matmul(t["intrs"][0].inverse()[:3, :3], rays)
        world = torch.matmul(pose, torch.cat([pts, torch.ones_like(pts[:1])]))
        cam = torch.matmul(t["w2cs"], world[None])[:, :3]
        proj = torch.matmul(t["intrs"][:, :3, :3], cam)
    else:
        rec = torch.from_numpy(np.ascontiguousarray(records)).to(dtype).reshape(nv, 12)
        a = torch.matmul(rec[:, :9].reshape(nv, 3, 3), torch.stack([xs, ys, torch.ones_like(xs)]))
        proj = depth.reshape(1, 1, -1) * a + rec[:, 9:].reshape(nv, 3, 1)
    xy = proj[:, :2] / (proj[:, 2:] + eps)
    nx, ny = 2 * xy[:, 0] / (W - 1) - 1, 2 * xy[:, 1] / (H - 1) - 1
    grid = torch.stack([nx, ny], dim=-1).unsqueeze(1)
    inb = (grid.abs() <= 1).all(dim=-1).reshape(nv, H, W)
    # the rules the reference leaves open (csrc/mono.hip's): a NaN coordinate, or one whose tap does not fit an int32, samples zero
    # (torch's CPU sampler would return NaN for the first and leaves the second to an undefined cast)
    size = torch.tensor([W, H], dtype=dtype)
    fits = (((grid + 1) * size - 1) / 2).abs() < 2.0 ** 31
    grid = torch.where(fits, grid, torch.full_like(grid, -1e6))
    warp = F.grid_sample(t["img_colors"], grid, mode="bilinear", padding_mode="zeros", align_corners=False).reshape(nv, 3, H, W)
    raw, term = ssim_terms(img.unsqueeze(0), warp)
    s = term.mean(dim=1)
    marked = torch.where(inb, s, torch.full_like(s, 1000.0))
    # torch.min(dim=0) written out: the lowest index attaining the minimum; a NaN IS the minimum and the first NaN view wins
    # (tests/test_virtualwarp_cpu.py holds this to the installed torch.min)
    low = marked.detach().amin(dim=0)
    idx = torch.arange(nv).reshape(nv, 1, 1)
    hit = (marked.detach() == low) | (marked.detach().isnan() & low.isnan())
    w = torch.where(hit, idx, nv).amin(dim=0).clamp_max(nv - 1)
    best = marked.gather(0, w.unsqueeze(0))[0]
    none = (best.detach() >= 1000) | ~t["vir_mask"].reshape(H, W)
    loss_map = torch.where(none, torch.zeros_like(best), best)
    loss = loss_map.mean()
    out = {"loss": loss.detach().numpy(), "loss_map": loss_map.detach().numpy(), "winner": torch.where(none, -1, w).numpy().astype(np.int8),
           "in_bounds": inb.numpy(), "s": s.detach().numpy(), "raw": raw.detach().numpy(), "warp": warp.detach().numpy(),
           "norm": torch.stack([nx, ny], dim=1).reshape(nv, 2, H, W).detach().numpy()}
    out["tap"] = np.stack([((out["norm"][:, 0] + 1) * W - 1) / 2, ((out["norm"][:, 1] + 1) * H - 1) / 2], axis=1)
    if grads and sampler:
        # one (view, channel) plane at a time: torch's sampler backward multiplies every channel's texel by its upstream, and a zero
        # upstream times a NaN texel of ANOTHER channel or view would mark derivatives that do not depend on it
        one = lambda v, c: F.grid_sample(t["img_colors"][v:v + 1, c:c + 1], grid[v:v + 1], mode="bilinear", padding_mode="zeros",      # noqa: E731
                                         align_corners=False).sum()
        out["dyd"] = np.stack([np.stack([torch.autograd.grad(one(v, c), depth, retain_graph=True)[0].numpy() for c in range(3)])
                               for v in range(nv)])
    if grads:
        (loss * upstream).backward()
        out["d_img"], out["d_depth"] = img.grad.numpy(), depth.grad.numpy()
    return out


# ---- the analytic backward of the window term, the reflection fold written out -----------------------------------------------------
def fold_positions(q, n):
    """The padded positions of one axis that reflect onto q: q, -q when 1 <= q <= 2, 2 (n - 1) - q when n - 3 <= q <= n - 2."""
    out = [q]
    if 1 <= q <= 2:
        out.append(-q)
    if n - 3 <= q <= n - 2:
        out.append(2 * (n - 1) - q)
    return out


def fold_count(p, q, n):
    return sum(1 for u in fold_positions(q, n) if abs(p - u) <= 2)


def window_coefficients(x, y):
    """fp64 numpy, x and y (3,H,W): the maps A, A', B, C of the header for the windows of every pixel (zero where the clamp is
    active), so that d term(p) / d y_j = (A + B y_j + C x_j) / 25 and d term(p) / d x_j = (A' + B x_j + C y_j) / 25."""
    X, Y = torch.from_numpy(x)[None], torch.from_numpy(y)[None]
    pool = lambda t: F.avg_pool2d(F.pad(t, (2, 2, 2, 2), mode="reflect"), 5, 1)[0].numpy()      # noqa: E731
    mx, my = pool(X), pool(Y)
    vx, vy, vxy = pool(X * X) - mx * mx, pool(Y * Y) - my * my, pool(X * Y) - mx * my
    n1, n2, d1, d2 = 2 * mx * my + 1e-4, 2 * vxy + 9e-4, mx * mx + my * my + 1e-4, vx + vy + 9e-4
    dd = d1 * d2
    r = n1 * n2 / dd
    raw = (1 - r) / 2
    open_ = (raw >= 0) & (raw <= 1)
    A = np.where(open_, -(mx * (n2 - n1) - r * my * (d2 - d1)) / dd, 0)
    Ap = np.where(open_, -(my * (n2 - n1) - r * mx * (d2 - d1)) / dd, 0)
    return A, Ap, np.where(open_, r * d1 / dd, 0), np.where(open_, -n1 / dd, 0)


def window_gradients(x, y, up, enters=None):
    """d/dx and d/dy of sum over p, c of up[p] * term_c(p), gathered per pixel q over the window centres within 2 of q, each
    counted fold_count times per axis: the rule the backward kernel follows.  fp64 numpy, x, y (3,H,W), up (H,W).
    enters (H,W) bool: the windows that enter the sum at all (default: every one).  A window that does not is SKIPPED, not
    multiplied by zero: the difference shows where x or y is not finite."""
    _, H, W = x.shape
    with np.errstate(invalid="ignore"):
        A, Ap, B, C = window_coefficients(x, y)
    gx, gy = np.zeros_like(x), np.zeros_like(y)
    for qy in range(H):
        for qx in range(W):
            for py in range(max(qy - 2, 0), min(qy + 2, H - 1) + 1):
                for px in range(max(qx - 2, 0), min(qx + 2, W - 1) + 1):
                    if enters is not None and not enters[py, px]:
                        continue
                    k = fold_count(py, qy, H) * fold_count(px, qx, W) * up[py, px] / 25
                    gy[:, qy, qx] += k * (A[:, py, px] + B[:, py, px] * y[:, qy, qx] + C[:, py, px] * x[:, qy, qx])
                    gx[:, qy, qx] += k * (Ap[:, py, px] + B[:, py, px] * x[:, qy, qx] + C[:, py, px] * y[:, qy, qx])
    return gx, gy


def gather_gradients(img, truth, upstream=1.0):
    """(d_img, d_depth) by THE HEADER'S GATHER RULE in fp64, in plain IEEE arithmetic: per view v the windows p with w(p) = v
    enter (the others are skipped), each with the coefficient maps of (virtual_img, y_v) — zero where the clamp is active or the
    term is a NaN — and upstream / (3 H W); d_img is the sum of the x sides over the views, d_depth the sum over views and channels
    of the y side times dy_v,c / ddepth, over EVERY view (a view that wins no window near q contributes 0 * dy/ddepth, which is
    a NaN where the derivative is not finite).  truth: warp_reference(..., sampler=True)'s dict ("warp", "winner", "dyd")."""
    x = np.asarray(img, dtype=np.float64)
    _, H, W = x.shape
    d_img, d_depth = np.zeros_like(x), np.zeros((H, W))
    with np.errstate(invalid="ignore"):
        for v in range(truth["warp"].shape[0]):
            won = truth["winner"] == v
            gx, gy = window_gradients(x, truth["warp"][v].astype(np.float64), np.full((H, W), upstream / (3.0 * H * W)), enters=won)
            d_img += gx
            d_depth += (gy * truth["dyd"][v]).sum(axis=0)
    return d_img, d_depth


# ---- e_ref, near ties, the bar --------------------------------------------------------------------------------------------------
def _dev(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    ok = np.isfinite(a) & np.isfinite(b)
    return float(np.abs(a - b)[ok].max()) if ok.any() else 0.0


def _near(q, edge, e):
    """Within TIE * e of the edge but not ON it: a quantity exactly on an edge in fp64 is there by construction (dyadic cameras,
    bit-identical views, identical images) and is decided the same way in every precision."""
    d = np.abs(np.asarray(q, dtype=np.float64) - edge)
    return (d > 0) & (d < TIE * e)


def _dilate(m, r=2):
    H, W = m.shape
    out = np.zeros_like(m)
    for y, x in zip(*np.nonzero(m)):
        out[max(y - r, 0):y + r + 1, max(x - r, 0):x + r + 1] = True
    return out


def near_ties(r64, r32, truth=None, tie=TIE):
    """e_ref from the pair (r64, r32); the edges looked for in `truth` (default r64), within tie * e_ref.
    {"decision": pixels whose winner / in_bounds may differ, "block": their 5x5 blocks (excluded from both gradients),
    "tap": pixels whose depth gradient alone is excluded, "e": the e_ref of s, raw, norm and tap}."""
    e = {k: _dev(r32[k], r64[k]) for k in ("s", "raw")}
    # the coordinates' e_ref where a decision can hang on them: within a frame's width of the frame (a point projected 2^33 px away
    # deviates by thousands of pixels and decides nothing)
    with np.errstate(invalid="ignore"):
        close = (np.abs(r64["norm"]) <= 2).all(axis=1, keepdims=True) & np.ones_like(r64["norm"], dtype=bool)
    e.update({k: _dev(r32[k][close], r64[k][close]) for k in ("norm", "tap")})
    r64 = r64 if truth is None else truth
    with np.errstate(invalid="ignore"):
        close = (np.abs(r64["norm"]) <= 2).all(axis=1, keepdims=True) & np.ones_like(r64["norm"], dtype=bool)
    e = {k: v * tie / TIE for k, v in e.items()}
    inb = r64["in_bounds"]
    nv = inb.shape[0]
    s = r64["s"]
    tie_s = np.zeros(inb.shape[1:], dtype=bool)
    for a in range(nv):
        for b in range(a + 1, nv):
            both = inb[a] & inb[b]
            tie_s |= both & _near(np.where(both, s[a] - s[b], 1.0), 0.0, e["s"])
    raw = r64["raw"]
    tie_clamp = ((_near(raw, 0.0, e["raw"]) | _near(raw, 1.0, e["raw"])) & inb[:, None]).any(axis=(0, 1))
    with np.errstate(invalid="ignore"):
        tie_norm = (_near(np.abs(r64["norm"]), 1.0, e["norm"]) & np.isfinite(r64["norm"])).any(axis=(0, 1))
        tap = r64["tap"]
        tie_tap = (_near(tap, np.round(tap), e["tap"]) & close).any(axis=(0, 1))
    decision = tie_s | tie_norm
    return {"decision": decision, "block": _dilate(decision | tie_clamp), "tap": tie_tap, "e": {k: v * TIE / tie for k, v in e.items()},
            "share": float((decision | tie_clamp | tie_tap).mean())}


def ulp32(v):
    return float(np.spacing(f32(abs(float(v)))))


def bar(e_ref, t64):
    """max(4 e_ref, one fp32 ulp of the tensor's largest magnitude)."""
    t = np.asarray(t64, dtype=np.float64)
    big = np.abs(t[np.isfinite(t)]).max() if np.isfinite(t).any() else 0.0
    return max(MARGIN * e_ref, ulp32(big))


def compare(name, got, r64, r32, keep=None, truth=None):
    """(deviation of got from truth, e_ref = deviation of r32 from r64, bound) of tensor `name` over the elements `keep` (bool);
    asserts the NaN pattern first.  truth: default r64."""
    g, a, b = (np.asarray(t, dtype=np.float64) for t in (got, r64[name], r32[name]))
    tr = a if truth is None else np.asarray(truth[name], dtype=np.float64)
    keep = np.ones(a.shape, dtype=bool) if keep is None else np.broadcast_to(keep, a.shape)
    assert np.array_equal(np.isnan(g) & keep, np.isnan(tr) & keep), f"{name}: NaN pattern differs"
    fin = keep & np.isfinite(a) & np.isfinite(tr)
    assert np.isfinite(g[fin]).all(), f"{name}: not finite where fp64 is"
    e_ref = _dev(b[fin], a[fin])
    return _dev(g[fin], tr[fin]), e_ref, bar(e_ref, tr[fin])


# ---- the smoothness loss --------------------------------------------------------------------------------------------------------
def smooth_reference(depth, guide=None, dtype=torch.float64, upstream=1.0):
    """(loss, d_depth) in `dtype` on the CPU: mean |dx depth| exp(-mean_C |dx guide|) + the same along y."""
    d = torch.from_numpy(np.ascontiguousarray(depth)).to(dtype).requires_grad_(True)
    tx, ty = (d[:, :-1] - d[:, 1:]).abs(), (d[:-1, :] - d[1:, :]).abs()
    if guide is not None:
        g = torch.from_numpy(np.ascontiguousarray(guide)).to(dtype)
        g = g[None] if g.dim() == 2 else g
        tx = tx * torch.exp(-(g[:, :, :-1] - g[:, :, 1:]).abs().mean(dim=0))
        ty = ty * torch.exp(-(g[:, :-1, :] - g[:, 1:, :]).abs().mean(dim=0))
    loss = tx.mean() + ty.mean()
    (loss * upstream).backward()
    return loss.detach().numpy(), d.grad.numpy()

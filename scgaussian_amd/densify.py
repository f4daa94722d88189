"""GaussianModel.densify_and_prune and reset_opacity on the GPU (csrc/densify.hip): three launches around one host read.

The reference's densification (scene/gaussian_model.py:758-930, train.py:195-200) is about sixty small torch operators, a dozen
boolean-mask indexings that each read a count back, four concatenations of every parameter and three re-keyings of every optimizer
state entry.  Its rule decides every Gaussian from that Gaussian alone, so here it is classify / scan / scatter:

    from scgaussian_amd import densify, optim
    optim.install(gaussians)                       # after gaussians.training_setup(opt)
    densify.install(gaussians)                     # gaussians.densify_and_prune / .reset_opacity now run here (train.py:197, 200)

The rule is the reference's, quirks included: a split ray-bound Gaussian stays and has its RAW log-scale row divided by 1.6; only
background rows are ever removed; `max_screen_size` merely switches the world-size term on (max_radii2D has been zeroed by the time
the reference looks at it).  What the kernels do not take raises ScgError — there is no torch fall-back.
"""
from __future__ import annotations

import ctypes as C
import functools

import torch

from . import _lib

# (model attribute, parameter-group name) of the two optimizers (scene/gaussian_model.py:491-509)
RAY_ATTRS = ("_zval", "_rayo", "_rayd", "_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation")
BG_GROUPS = (("bg_xyz", "bg_xyz", (3,)), ("bg_features_dc", "bg_f_dc", (1, 3)), ("bg_features_rest", "bg_f_rest", (15, 3)),
             ("bg_opacity", "bg_opacity", (1,)), ("bg_scaling", "bg_scaling", (3,)), ("bg_rotation", "bg_rotation", (4,)))
_RAY_SHAPES = {"_zval": (1,), "_rayo": (3,), "_rayd": (3,), "_features_dc": (1, 3), "_features_rest": (15, 3), "_opacity": (1,),
               "_scaling": (3,), "_rotation": (4,)}
_FIELDS = ("xyz", "features_dc", "features_rest", "opacity", "scaling", "rotation")       # ScgDensifyTensors, in BG_GROUPS order


def _err(msg: str):
    return _lib.ScgError("densify: " + msg)


def _check(name: str, t, rows: int, tail, dev) -> torch.Tensor:
    if not torch.is_tensor(t):
        raise _err(f"{name} is not a tensor")
    if t.device != dev:
        raise _err(f"{name} is on {t.device}, the model on {dev}")
    if t.dtype != torch.float32:
        raise _err(f"{name} must be fp32, not {t.dtype}")
    if rows == 0 and t.shape[0] == 0:              # the reference's empty background set is torch.empty(0)
        return t
    if tuple(t.shape) != (rows,) + tuple(tail):
        raise _err(f"{name} has shape {tuple(t.shape)}, expected {(rows,) + tuple(tail)}")
    if not t.is_contiguous():
        raise _err(f"{name} must be contiguous")
    return t


def _group(opt, name: str, param):
    """(group, state or None) of the group called `name`, which must hold exactly `param`."""
    if opt is None:
        raise _err("the model has no optimizer (call training_setup first)")
    for g in opt.param_groups:
        if len(g["params"]) != 1:
            raise _err(f"group {g.get('name')!r} has {len(g['params'])} parameters; the reference's optimizers have one per group")
    for g in opt.param_groups:
        if g.get("name") == name:
            if g["params"][0] is not param:
                raise _err(f"group {name!r} does not hold the model's tensor of that name")
            st = opt.state.get(param)
            if not st or "exp_avg" not in st:
                return g, None
            return g, st
    raise _err(f"no parameter group named {name!r}")


def _moments(name: str, st, like: torch.Tensor):
    if st is None:
        return None, None
    m, v = st["exp_avg"], st["exp_avg_sq"]
    for what, t in (("exp_avg", m), ("exp_avg_sq", v)):
        if not t.is_cuda or t.device != like.device or t.dtype != torch.float32 or not t.is_contiguous() or t.shape != like.shape:
            raise _err(f"{what} of {name} must be a contiguous fp32 CUDA tensor shaped like its parameter")
    return m, v


class _Model:
    """The validated tensors of one call."""

    def __init__(self, g):
        for a in RAY_ATTRS + tuple(b[0] for b in BG_GROUPS):
            if not hasattr(g, a):
                raise _err(f"the model has no attribute {a}")
        z = g._zval
        self.stream = _lib.stream_of(z, "densify: the model")
        self.dev = dev = z.device
        self.nr = nr = z.shape[0]
        self.ray = {a: _check(a, getattr(g, a), nr, _RAY_SHAPES[a], dev) for a in RAY_ATTRS}
        self.nb = nb = g.bg_xyz.shape[0]
        self.bg = {a: _check(a, getattr(g, a), nb, tail, dev) for a, _n, tail in BG_GROUPS}
        self.P = nr + nb
        m = _lib.ScgModel()
        m.ray.count, m.bg.count = nr, nb
        for a in RAY_ATTRS:
            setattr(m.ray, a.lstrip("_"), self.ray[a].data_ptr() if nr else None)
        for a, f in zip((b[0] for b in BG_GROUPS), _FIELDS):
            setattr(m.bg, f, self.bg[a].data_ptr() if nb else None)
        self.c = m


def _forget(opt) -> None:
    fn = getattr(opt, "tensors_replaced", None)
    if fn is not None:
        fn()


@torch.no_grad()
def densify_and_prune(gaussians, max_grad, min_opacity, extent, max_screen_size, noise=None) -> None:
    """The reference's GaussianModel.densify_and_prune(max_grad, min_opacity, extent, max_screen_size) on `gaussians`, any object
    with the reference model's attribute names (both optimizers torch.optim.Adam or optim.ArenaAdam).

    The background tensors, their moments and the three statistics tensors are replaced by new objects (re-keyed in
    `optimizer_bg` once per group); the ray-bound tensors keep their identity — `_scaling` and the moments of the ray optimizer's
    "scaling" group are edited in place.  One host read (the four section sizes); no empty_cache().

    noise: fp32 device tensor (2, P, 3), the unit normal sample of (copy, source index) for the children of a split.  Default:
    torch.randn on the device's default generator, drawn for every source without a host read (so replicas that share the
    generator state stay identical).  The reference draws torch.normal for the selected rows only, so its stream of random
    numbers differs from this one; the distribution is the same."""
    max_grad, min_opacity, extent = float(max_grad), float(min_opacity), float(extent)
    if not max_grad > 0:
        raise _err(f"max_grad = {max_grad} must be > 0")
    md = _Model(gaussians)
    dev, nr, nb, P = md.dev, md.nr, md.nb, md.P
    accum = _check("xyz_gradient_accum", gaussians.xyz_gradient_accum, P, (1,), dev)
    denom = _check("denom", gaussians.denom, P, (1,), dev)
    _check("max_radii2D", gaussians.max_radii2D, P, (), dev)
    if noise is None:
        noise = torch.randn(2, P, 3, device=dev, dtype=torch.float32)
    else:
        _check("noise", noise, 2, (P, 3), dev)
    _sg, sc_state = _group(gaussians.optimizer, "scaling", md.ray["_scaling"])
    sc_m, sc_v = _moments("_scaling", sc_state, md.ray["_scaling"])
    groups = []
    for a, name, _tail in BG_GROUPS:
        g, st = _group(gaussians.optimizer_bg, name, md.bg[a])
        groups.append((a, g, st) + _moments(a, st, md.bg[a]))

    lib = _lib.load()
    ws_bytes = lib.scg_densify_workspace_bytes(P)
    if ws_bytes == 0:
        raise _err(f"{P} Gaussians are more than the kernels take")
    ws = torch.empty(ws_bytes // 4, dtype=torch.int32, device=dev)
    big = 0.2 * extent if max_screen_size else -1.0
    _lib.check(lib.scg_densify_classify(C.byref(md.c), accum.data_ptr() or None, denom.data_ptr() or None, max_grad, min_opacity,
                                        float(gaussians.percent_dense) * extent, big, ws.data_ptr(), ws_bytes, md.stream),
               "scg_densify_classify")
    kept, clones, children, _ = (int(x) for x in ws[:4].tolist())                          # the one host read
    rows = kept + clones + 2 * children

    a = _lib.ScgDensifyScatter()
    a.out_rows = rows
    new = {}
    for (attr, _g, st, m, v), field, (_a, _n, tail) in zip(groups, _FIELDS, BG_GROUPS):
        p = torch.empty((rows,) + tail, dtype=torch.float32, device=dev)
        nm = nv = None
        if st is not None:
            nm, nv = torch.empty_like(p), torch.empty_like(p)
            setattr(a.in_exp_avg, field, m.data_ptr() or None)
            setattr(a.in_exp_avg_sq, field, v.data_ptr() or None)
        new[attr] = (p, nm, nv)
        if rows:
            setattr(a.out, field, p.data_ptr())
            if nm is not None:
                setattr(a.out_exp_avg, field, nm.data_ptr())
                setattr(a.out_exp_avg_sq, field, nv.data_ptr())
    n_accum = torch.empty((nr + rows, 1), dtype=torch.float32, device=dev)
    n_denom = torch.empty((nr + rows, 1), dtype=torch.float32, device=dev)
    n_radii = torch.empty((nr + rows,), dtype=torch.float32, device=dev)
    a.accum, a.denom, a.max_radii2D = (t.data_ptr() or None for t in (n_accum, n_denom, n_radii))
    if nr:
        a.ray_scaling = md.ray["_scaling"].data_ptr()
        if sc_m is not None:
            a.ray_scaling_exp_avg, a.ray_scaling_exp_avg_sq = sc_m.data_ptr(), sc_v.data_ptr()
    a.noise = noise.data_ptr() or None
    _lib.check(lib.scg_densify_scatter(C.byref(md.c), C.byref(a), ws.data_ptr(), ws_bytes, md.stream), "scg_densify_scatter")

    # hand over: one re-keying per background group (cat_tensors_to_optimizer's, once instead of three times)
    opt = gaussians.optimizer_bg
    for attr, g, st, _m, _v in groups:
        p, nm, nv = new[attr]
        old = g["params"][0]
        param = torch.nn.Parameter(p.requires_grad_(True))
        if st is not None:
            st["exp_avg"], st["exp_avg_sq"] = nm, nv
            del opt.state[old]
            g["params"][0] = param
            opt.state[param] = st
        else:
            opt.state.pop(old, None)
            g["params"][0] = param
        setattr(gaussians, attr, param)
    gaussians.xyz_gradient_accum, gaussians.denom, gaussians.max_radii2D = n_accum, n_denom, n_radii
    _forget(opt)
    if hasattr(gaussians, "__dict__"):
        gaussians.__dict__.pop("_scg_model_args", None)            # the render path's cache holds the old tensors alive


@torch.no_grad()
def reset_opacity(gaussians) -> None:
    """The reference's GaussianModel.reset_opacity(): both raw opacity tensors become logit(min(sigmoid(x), 0.01)) IN PLACE (the
    tensors keep their identity) and the moments of both opacity groups are zeroed, in one launch."""
    md = _Model(gaussians)
    _g, st = _group(gaussians.optimizer, "opacity", md.ray["_opacity"])
    rm, rv = _moments("_opacity", st, md.ray["_opacity"])
    bm = bv = None
    if md.nb:
        _g, st = _group(gaussians.optimizer_bg, "bg_opacity", md.bg["bg_opacity"])
        bm, bv = _moments("bg_opacity", st, md.bg["bg_opacity"])
    _lib.check(_lib.load().scg_reset_opacity(md.nr, md.ray["_opacity"].data_ptr() or None, _lib.ptr(rm), _lib.ptr(rv), md.nb,
                                             md.bg["bg_opacity"].data_ptr() or None, _lib.ptr(bm), _lib.ptr(bv), md.stream),
               "scg_reset_opacity")


def install(gaussians) -> None:
    """Bind densify_and_prune and reset_opacity as methods of this model instance under the reference's names, so that
    train.py:197 and :200 run unchanged: the companion of optim.install(gaussians)."""
    gaussians.densify_and_prune = functools.partial(densify_and_prune, gaussians)
    gaussians.reset_opacity = functools.partial(reset_opacity, gaussians)

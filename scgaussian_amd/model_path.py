"""The rasterizer fed with the reference MODEL's raw parameter tensors (ABI 10: scg_forward_model / scg_backward_model).

The reference's render() (gaussian_renderer/__init__.py:20-118) turns the model into the operator's activated inputs on every
call: `get_xyz` = cat(rayo + rayd * zval, bg_xyz) three times (:28 twice, :55), `get_features` = cat(cat(f_dc, bg_f_dc),
cat(f_rest, bg_f_rest), dim=1) — a 192 B / Gaussian copy (:85; scene/gaussian_model.py:134-142) —, sigmoid / exp / normalize +
cat for opacity / scaling / rotation (:57, :67-68; scene/gaussian_model.py:105-152): 67 torch launches per training step forward
and backward around a 6-launch rasterizer step, measured at 0.70 ms per step against 0.25 ms for the bare operator at 200 k
Gaussians (bench.py `render_glue`, round 6).  Here the two geometry kernels read the raw tensors where they lie and write the
gradients of the RAW parameters into one flat arena: activations, their derivatives and the concatenations happen in registers.

    color, radii, depth, alpha = rasterize_model(settings, means2D, zval, rayo, rayd, features_dc, features_rest, opacity,
                                                 scaling, rotation, bg_xyz, bg_features_dc, ..., bg_rotation)

`render.render()` takes this path by itself for a model that carries these tensors (reference attribute names `_zval`,
`_features_dc`, ..., `bg_xyz`, ... or ply_io.RayBoundModel's) with the reference's default pipe; everything else goes through the
getters as before.  The gradient arena puts `features_rest` / `bg_features_rest` LAST: the other ten tensors' gradients are one
contiguous span, which parallel.GradBucket all-reduces in place at every SH degree.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch

from . import _counts, _grads, _lib
from . import rasterizer as R
from ._lib import ScgModel, ScgModelGrads, check

# order of the operator's tensor arguments (behind means2D) = order of the gradients backward returns
_RAY = ("zval", "rayo", "rayd", "features_dc", "features_rest", "opacity", "scaling", "rotation")
_BG = ("bg_xyz", "bg_features_dc", "bg_features_rest", "bg_opacity", "bg_scaling", "bg_rotation")
ARG_NAMES = _RAY + _BG
# segments of the gradient arena: the two large SH tensors last (see the module docstring); rayo / rayd are constants
_ARENA_ORDER = ("zval", "opacity", "scaling", "rotation", "features_dc", "bg_xyz", "bg_opacity", "bg_scaling", "bg_rotation",
                "bg_features_dc", "features_rest", "bg_features_rest")


class _ModelArgs:
    """ScgModel plus the tensors whose storage it points at (kept alive for the call and saved for backward)."""

    def __init__(self, tensors: dict):
        t = tensors
        self.tensors = tuple(t[n] for n in ARG_NAMES)
        nr, nb = int(t["zval"].shape[0]), int(t["bg_xyz"].shape[0])
        self.n_ray, self.n_bg, self.P = nr, nb, nr + nb
        self.device = (t["zval"] if nr else t["bg_xyz"]).device
        m = ScgModel()
        m.ray.count, m.bg.count = nr, nb
        if nr:
            for f, n in (("zval", "zval"), ("rayo", "rayo"), ("rayd", "rayd"), ("features_dc", "features_dc"),
                         ("features_rest", "features_rest"), ("opacity", "opacity"), ("scaling", "scaling"),
                         ("rotation", "rotation")):
                setattr(m.ray, f, t[n].data_ptr())
        if nb:
            for f, n in (("xyz", "bg_xyz"), ("features_dc", "bg_features_dc"), ("features_rest", "bg_features_rest"),
                         ("opacity", "bg_opacity"), ("scaling", "bg_scaling"), ("rotation", "bg_rotation")):
                setattr(m.bg, f, t[n].data_ptr())
        self.c = m
        self.ref = C.byref(m)
        # the gradient arena's segments (_grads.layout): the trainable tensors of the non-empty sets
        self.grad_items = tuple((n, t[n].shape) for n in _ARENA_ORDER if t[n].shape[0])

    def grad_outputs(self, into, d_means2D_out):
        """What rasterizer._backward_view writes one view's gradients to: _grad_arena + the view's own dL/dmeans2D."""
        out = dict(_grad_arena(self, into))
        out["means2D"] = d_means2D_out if d_means2D_out is not None else \
            torch.empty((self.P, 3), dtype=torch.float32, device=self.device)
        return out


def _usable(t: torch.Tensor, device, align16: bool) -> bool:
    return (isinstance(t, torch.Tensor) and t.dtype == torch.float32 and t.device == device and t.is_contiguous()
            and (t.numel() == 0 or not align16 or t.data_ptr() % 16 == 0))


def supported(tensors: dict, settings=None) -> bool:
    """True when the model path can take these tensors as they are: fp32, contiguous, one CUDA device, the reference's shapes
    ((n,1) zval / opacity, (n,3) rays / scaling / positions, (n,4) rotation, (n,1,3) + (n,15,3) SH), 16-byte aligned where the
    kernels use 16-byte accesses — and, with `settings`, an image the tile-first binning takes.  Anything else: the getters."""
    try:
        z, bx = tensors["zval"], tensors["bg_xyz"]
        nr, nb = int(z.shape[0]), int(bx.shape[0])
        if nr + nb == 0:
            return False
        dev = (z if nr else bx).device
        if dev.type != "cuda":
            return False
        shapes = {"zval": (nr, 1), "rayo": (nr, 3), "rayd": (nr, 3), "features_dc": (nr, 1, 3), "features_rest": (nr, 15, 3),
                  "opacity": (nr, 1), "scaling": (nr, 3), "rotation": (nr, 4), "bg_xyz": (nb, 3), "bg_features_dc": (nb, 1, 3),
                  "bg_features_rest": (nb, 15, 3), "bg_opacity": (nb, 1), "bg_scaling": (nb, 3), "bg_rotation": (nb, 4)}
        for n, shp in shapes.items():
            t = tensors[n]
            if shp[0] == 0:
                if t.shape[0] != 0:
                    return False
                continue
            if tuple(t.shape) != shp or not _usable(t, dev, n.endswith(("features_dc", "features_rest", "rotation"))):
                return False
        return settings is None or _accepts(nr + nb, settings)
    except (KeyError, AttributeError, IndexError):
        return False


_ACCEPTS = {}                             # (P, W, H) -> the tile-first binning takes the model path's first-render bound


def _accepts(P: int, settings) -> bool:
    key = (P, int(settings.image_width), int(settings.image_height))
    v = _ACCEPTS.get(key)
    if v is None:
        if len(_ACCEPTS) > 256:
            _ACCEPTS.clear()
        v = _ACCEPTS[key] = _lib.load().scg_binning_accepts_bound(_counts.first_sight_capacity(P), key[1], key[2],
                                                                  _lib.BINNING_AUTO) == 1
    return v


_ATTRS = None


def model_for(pc, settings=None) -> Optional[_ModelArgs]:
    """The _ModelArgs of `pc` when the model path can render it (tensors_of + supported), else None.  The answer is remembered ON
    the model object and reused while its fourteen tensors are the same objects at the same addresses (a training loop renders
    the same parameters thousands of times between two densifications; the checks cost as much host time as the forward's
    launches at the reference's scene size): validated per call by identity + data_ptr, rebuilt after any change."""
    global _ATTRS
    cached = pc.__dict__.get("_scg_model_args") if hasattr(pc, "__dict__") else None
    if cached is not None:
        attrs, args = cached
        ok = True
        for a, n, t, ptr_ in zip(attrs, ARG_NAMES, args.tensors, args.ptrs):
            if a is None:                                    # (a stand-in for a set the model did not have: still without it?)
                if isinstance(getattr(pc, n, None), torch.Tensor):
                    ok = False
                    break
                continue
            if getattr(pc, a, None) is not t or t.data_ptr() != ptr_:
                ok = False
                break
        if ok and args.n_ray == args.tensors[0].shape[0] and args.n_bg == args.tensors[8].shape[0]:
            return args if (settings is None or _accepts(args.P, settings)) else None
    t = tensors_of(pc)
    if t is None or not supported(t):
        return None
    args = _ModelArgs(t)
    args.ptrs = tuple(x.data_ptr() for x in args.tensors)
    # which attribute of pc each tensor came from (None: an empty stand-in tensors_of made up for a model without a bg set)
    attrs = []
    for n, x in zip(ARG_NAMES, args.tensors):
        found = None
        for a in (_REFERENCE_ATTRS.get(n) or (n,)):
            if getattr(pc, a, None) is x:
                found = a
                break
        attrs.append(found)
    try:
        pc.__dict__["_scg_model_args"] = (tuple(attrs), args)
    except (AttributeError, TypeError):
        pass
    return args if (settings is None or _accepts(args.P, settings)) else None


def _grad_arena(model: _ModelArgs, into):
    """{name: gradient tensor} for the trainable tensors of the non-empty sets, all views of ONE flat arena (pooled: _grads.py),
    + "_pooled" and "_c" (the ScgModelGrads struct).  `into`: an earlier call's result — reused."""
    if into is not None:
        return into
    lay = _grads.layout(model.grad_items)
    arena, pooled = _grads._take_arena("model", lay, lay[3], model.device, R.ARENA_POOL)
    out = _grads.carve(arena, lay)
    out["_pooled"] = pooled
    # the struct of raw pointers: a pooled arena's segments stay where they are — built once per arena
    g = pooled.cstruct if pooled is not None else None
    if g is None:
        g = ScgModelGrads()
        base, off = arena.data_ptr(), 0
        for n, sz in zip(lay[0], lay[1]):
            if n.startswith("bg_"):
                setattr(g.bg, n[3:], base + 4 * off)
            else:
                setattr(g.ray, n, base + 4 * off)
            off += sz
        if pooled is not None:
            pooled.cstruct = g
    out["_c"] = g
    return out


def _node_grads(g, d_means2D):
    """A node's gradients in forward argument order (means2D, ARG_NAMES, settings, model); all None when no view reached the loss."""
    if g is None:
        return (None,) * (len(ARG_NAMES) + 3)
    return (d_means2D,) + tuple(g.get(n) for n in ARG_NAMES) + (None, None)


class _RasterizeModel(torch.autograd.Function):
    @staticmethod
    def forward(ctx, means2D, *args):
        *tensors, raster_settings, model = args
        ctx.model = model if model is not None else _ModelArgs(dict(zip(ARG_NAMES, tensors)))
        return R._views_forward(ctx, (raster_settings,), ctx.model, any(ctx.needs_input_grad))[0]

    @staticmethod
    def backward(ctx, *grads):
        return _node_grads(*R._views_backward(ctx.states, ctx.model, ctx.saved_tensors[-1:], grads, False))


def rasterize_model(raster_settings, means2D: torch.Tensor, _args: Optional[_ModelArgs] = None, **tensors):
    """(color (3,H,W), radii (P,) int32, depth (1,H,W), alpha (1,H,W)) of the model given by its raw tensors (keyword
    arguments named as in ARG_NAMES; `means2D` (P,3): the screen-space gradient slot, reference gaussian_renderer/__init__.py:28).
    Differentiable with respect to every tensor but rayo / rayd.  `_args`: the validated _ModelArgs of these tensors
    (model_for), in place of the keyword arguments."""
    R._require_cuda(means2D)
    ts = _args.tensors if _args is not None else tuple(tensors[n] for n in ARG_NAMES)
    apply = _RasterizeModel.apply
    if R._camera_wants_grad((raster_settings,)):
        from . import camera_grad                            # (it imports this module)
        apply = camera_grad.apply_model
    return apply(means2D, *ts, raster_settings, _args)


class _RasterizeModelViews(torch.autograd.Function):
    """K views of one model in ONE autograd node (BASELINE cfg5's "multi-view batched step", rasterizer._RasterizeViews on the
    model path): forward = the K views one after the other; backward = per view blend backward + geometry backward, the second and
    later views ADDING their raw-parameter gradients to the first one's in the kernel (scg_backward_model `accumulate`), so the
    node returns the gradient of the SUM over views from one arena — one exchange per K views.  Outputs, flat: color_0, radii_0,
    depth_0, alpha_0, color_1, ...; means2D is (K, P, 3)."""

    @staticmethod
    def forward(ctx, means2D, *args):
        *tensors, settings_list, model = args
        ctx.model = model if model is not None else _ModelArgs(dict(zip(ARG_NAMES, tensors)))
        return R._views_forward(ctx, settings_list, ctx.model, any(ctx.needs_input_grad))[0]

    @staticmethod
    def backward(ctx, *grads):
        return _node_grads(*R._views_backward(ctx.states, ctx.model, ctx.saved_tensors[-len(ctx.states):], grads, True))


def rasterize_model_views(settings_list, means2D: torch.Tensor, _args: Optional[_ModelArgs] = None, **tensors):
    """[(color, radii, depth, alpha)] * K for the K views `settings_list` of one model (raw tensors as in rasterize_model);
    `means2D` is (K, P, 3): one screen-space gradient slot per view.  One autograd node: the views' gradients are summed in the
    kernels and land in one arena."""
    R._require_cuda(means2D)
    K = len(settings_list)
    if means2D.dim() != 3 or means2D.shape[0] != K:
        raise ValueError(f"means2D must be ({K}, P, 3): one screen-space gradient slot per view")
    ts = _args.tensors if _args is not None else tuple(tensors[n] for n in ARG_NAMES)
    apply = _RasterizeModelViews.apply
    if R._camera_wants_grad(settings_list):
        from . import camera_grad                            # (it imports this module)
        apply = camera_grad.apply_model_views
    flat = apply(means2D, *ts, list(settings_list), _args)
    return [tuple(flat[4 * k: 4 * k + 4]) for k in range(K)]


def activate(**tensors):
    """The model's activated getters in ONE launch (scg_model_activate): (xyz (P,3), opacity (P,1), scaling (P,3), rotation (P,4))
    as reference scene/gaussian_model.py:105-152 computes them, by the device functions the geometry kernels use.  No autograd."""
    model = _ModelArgs({n: tensors[n].detach() for n in ARG_NAMES})
    dev = model.device
    P = model.P
    out = [torch.empty((P, k), dtype=torch.float32, device=dev) for k in (3, 1, 3, 4)]
    with R._on_device(dev):
        check(_lib.load().scg_model_activate(model.ref, *(o.data_ptr() for o in out), R._stream(dev)), "scg_model_activate")
    return tuple(out)


# ---- the reference model's attribute names -> ARG_NAMES -------------------------------------------------------------------
_REFERENCE_ATTRS = {"zval": ("_zval", "zval"), "rayo": ("_rayo", "rayo"), "rayd": ("_rayd", "rayd"),
                    "features_dc": ("_features_dc", "features_dc"), "features_rest": ("_features_rest", "features_rest"),
                    "opacity": ("_opacity", "opacity"), "scaling": ("_scaling", "scaling"), "rotation": ("_rotation", "rotation")}


def tensors_of(pc) -> Optional[dict]:
    """The raw tensors of a reference GaussianModel (scene/gaussian_model.py:452-468: `_zval`, `_rayo`, `_rayd`, `_features_dc`,
    `_features_rest`, `_opacity`, `_scaling`, `_rotation`, `bg_xyz`, `bg_features_dc`, ...) or of a ply_io.RayBoundModel (the same
    names without the underscore), keyed by ARG_NAMES; None when `pc` does not carry them."""
    out = {}
    for name, cands in _REFERENCE_ATTRS.items():
        t = None
        for a in cands:
            t = getattr(pc, a, None)
            if isinstance(t, torch.Tensor):
                break
        if not isinstance(t, torch.Tensor):
            return None
        out[name] = t
    dev = out["zval"].device
    for name in _BG:
        t = getattr(pc, name, None)
        if not isinstance(t, torch.Tensor):                       # a model without a background set (hasattr(self, "bg_xyz") false)
            k = {"bg_xyz": (0, 3), "bg_features_dc": (0, 1, 3), "bg_features_rest": (0, 15, 3), "bg_opacity": (0, 1),
                 "bg_scaling": (0, 3), "bg_rotation": (0, 4)}[name]
            t = torch.empty(k, dtype=torch.float32, device=dev)
        out[name] = t
    return out

"""The rasterizer's gradient with respect to the camera: dL/dviewmatrix, dL/dprojmatrix, dL/dcampos (libscg_camgrad.so,
include/camgrad/scg_camgrad.h states the rule).

    dV, dPM, dcampos = camera_backward(settings, inputs, radii, dsplats)        # the plain call, on one view's gradient records

`GaussianRasterizationSettings.viewmatrix / projmatrix / campos` are attributes of a non-tensor argument of the rasterizer's autograd
nodes.  When one of them requires grad (and grad mode is on) the four public routes — GaussianRasterizer / rasterize_gaussians,
GaussianRasterizerViews, model_path.rasterize_model(_views) and with them render.render(_views) — go through the sibling nodes
below, which take those tensors as inputs of their own (3 per view) next to the usual ones.  A sibling node IS the usual node: it
calls that node's forward and backward (the K-view core of rasterizer.py, the same launches) and arms every view's saved state with
`camera_pass`; rasterizer._backward_view calls it right behind the view's geometry backward, while the view's gradient records —
a tensor on the staged path, a raw pointer into the forward's workspace on the one-call paths — are still in its hands: two more
launches per view, no host read, capturable.  With no camera tensor requiring grad none of this runs: the usual nodes, the same
launches, the same bits.

Conventions (oracle/torch_rasterizer.py D1-D4 as they bear on the camera): the matrices are the flat transposed ones the rasterizer
reads; a view-space component under an active 1.3 tanfov clamp is a constant (D2), so is the cull (D3) and every integer (D4); the
alpha clamp is straight-through (D1: it is in the records already).  The fourth column of the view matrix and the third of the
projection matrix are never read: their gradients are exact zeros.  Not covered: gradients with respect to tanfovx / tanfovy
(intrinsics arrive only through projmatrix), and the background colour.

The frame cache (_frames.py) and the per-camera hints (_cameras.py) see DETACHED aliases of the three tensors: same storage, same
address, same version counter, hence the same keys as without requires_grad and no graph kept alive by a cached frame.  A camera
whose matrices are recomputed every step (pose.CameraPose) names itself with tag_camera, so no step reads the device.
"""
from __future__ import annotations

import functools

import torch

from . import _lib_camgrad, model_path
from . import rasterizer as R
from ._frames import _f32c, _stream
from ._lib_camgrad import CAMGRAD_NO_CAMPOS, CAMGRAD_OUT_FLOATS, CAMGRAD_SUMS, CAMGRAD_BLOCK, check

_CAMERA_FIELDS = ("viewmatrix", "projmatrix", "campos")


def _launch(H, W, tanfovx, tanfovy, mod, deg, view, proj, campos, inputs, radii, records: int, dev, want_campos: bool, out=None,
            partials=None):
    """The library call on torch's current stream of `dev`.  Returns the (35,) fp32 output tensor.  out / partials: the caller's
    buffers in place of fresh ones."""
    lib = _lib_camgrad.load()
    model = None if isinstance(inputs, (tuple, list)) else inputs
    P = int(radii.shape[0])
    with R._on_device(dev):
        n_partial = (P + CAMGRAD_BLOCK - 1) // CAMGRAD_BLOCK * CAMGRAD_SUMS
        if out is None:
            out = torch.empty((CAMGRAD_OUT_FLOATS,), dtype=torch.float32, device=dev)
        if partials is None:
            partials = torch.empty((n_partial,), dtype=torch.float32, device=dev)
        for t, n, what in ((out, CAMGRAD_OUT_FLOATS, "out"), (partials, n_partial, "partials")):
            if t.dtype != torch.float32 or t.device != dev or not t.is_contiguous() or t.numel() < n:
                raise R._lib.ScgError(f"camera_backward: {what} must be a contiguous fp32 tensor of at least {n} elements on {dev}")
        flags = 0 if want_campos else CAMGRAD_NO_CAMPOS
        scalars = (int(H), int(W), float(tanfovx), float(tanfovy), float(mod), int(deg))
        tail = (radii.data_ptr() if P else None, records if P else None, partials.data_ptr() if P else None, out.data_ptr(), flags,
                _stream(dev))
        if model is None:
            shs = inputs[2]
            check(lib.scg_camgrad_backward(*scalars, shs.shape[1] if shs is not None else 0, P, view.data_ptr(), proj.data_ptr(),
                                           campos.data_ptr(), *(None if t is None else t.data_ptr() for t in inputs), *tail),
                  "scg_camgrad_backward")
        else:
            check(lib.scg_camgrad_backward_model(*scalars, P, view.data_ptr(), proj.data_ptr(), campos.data_ptr(), model.ref, *tail),
                  "scg_camgrad_backward_model")
    return out


def camera_backward(settings, inputs, radii, dsplats, want_campos: bool = True, out=None, partials=None):
    """(dL/dviewmatrix (4,4), dL/dprojmatrix (4,4), dL/dcampos (3,)) of one view, fp32 on the device, from the gradient records
    `dsplats` ((P, 16) tensor or raw device pointer) its blend backward left.  `inputs`: the operator's 7-tuple (means3D,
    opacities, shs, colors_precomp, scales, rotations, cov3D_precomp) or a model_path._ModelArgs; `radii` as the forward returned
    them.  Two launches on the current stream, nothing read back.  out (35 floats) / partials (27 floats per 256 Gaussians): buffers
    of the caller's in place of fresh ones (every word read is written first: they need no clearing)."""
    model = None if isinstance(inputs, (tuple, list)) else inputs
    dev = radii.device
    if dev.type != "cuda":
        raise R._lib.ScgError("camera_backward needs tensors on a ROCm GPU ('cuda' device); there is no CPU path")
    if model is None:
        inputs = tuple(_f32c(t, dev) for t in inputs)
    view, proj, campos = (_f32c(getattr(settings, n), dev) for n in _CAMERA_FIELDS)
    if radii.dtype != torch.int32 or not radii.is_contiguous():
        raise R._lib.ScgError("camera_backward: radii must be the contiguous int32 tensor the forward returned")
    keep = None if isinstance(dsplats, int) else _f32c(dsplats, dev)           # (held until the launches are queued)
    records = dsplats if isinstance(dsplats, int) else (None if keep is None else keep.data_ptr())
    out = _launch(settings.image_height, settings.image_width, settings.tanfovx, settings.tanfovy, settings.scale_modifier,
                  settings.sh_degree, view, proj, campos, inputs, radii, records, dev, want_campos, out, partials)
    return out[0:16].view(4, 4), out[16:32].view(4, 4), out[32:35]


# ---- routing ---------------------------------------------------------------------------------------------------------------------
def _camera_pass(want_campos, state, inputs, radii, records, dev):
    """What rasterizer._backward_view calls behind a view's geometry backward: the camera pass on that view's records."""
    fr = state["frame"]
    view, proj, campos = fr.keep[0:3]                        # the very tensors the view's forward read
    c = fr.c
    state["camera_grads"] = _launch(c.height, c.width, c.tanfovx, c.tanfovy, c.scale_modifier, c.sh_degree, view, proj, campos,
                                    inputs, radii, records, dev, want_campos)


def _detached(st):
    """`st` with detached aliases of the three camera tensors (the camera's tag_camera name goes along)."""
    def alias(t):
        d = t.detach()
        tag = getattr(t, "_scg_camera_id", None)
        if tag is not None:
            d._scg_camera_id = tag
        return d
    return st._replace(**{n: alias(getattr(st, n)) for n in _CAMERA_FIELDS})


def _camera_tensors(settings_list):
    return tuple(getattr(st, n) for st in settings_list for n in _CAMERA_FIELDS)


def _arm(ctx, n_base: int, cams):
    """Arm the K saved states of a node whose forward just ran; `cams`: its 3K camera inputs, at positions n_base.. of its inputs."""
    ctx.cam_meta = tuple((t.shape, t.dtype, t.device) for t in cams)
    for k, state in enumerate(ctx.states):
        state["camera_pass"] = functools.partial(_camera_pass, bool(ctx.needs_input_grad[n_base + 3 * k + 2]))


def _camera_grads(ctx):
    """The 3K camera gradients in the callers' shapes and dtypes; None for a view that did not reach the loss."""
    out = []
    for k, state in enumerate(ctx.states):
        g = state.pop("camera_grads", None)
        parts = (None, None, None) if g is None else (g[0:16], g[16:32], g[32:35])
        for p, (shape, dtype, device) in zip(parts, ctx.cam_meta[3 * k: 3 * k + 3]):
            out.append(None if p is None else p.reshape(shape).to(device=device, dtype=dtype))
    return tuple(out)


class _RasterizeGaussiansCam(torch.autograd.Function):
    """rasterizer._RasterizeGaussians + (viewmatrix, projmatrix, campos) as inputs."""

    @staticmethod
    def forward(ctx, *args):
        *base, settings, vm, pm, cp = args
        outs = R._RasterizeGaussians.forward(ctx, *base, _detached(settings))
        _arm(ctx, 9, (vm, pm, cp))
        return outs

    @staticmethod
    def backward(ctx, *grads):
        return R._RasterizeGaussians.backward(ctx, *grads) + _camera_grads(ctx)


class _RasterizeViewsCam(torch.autograd.Function):
    """rasterizer._RasterizeViews + 3K camera tensors as inputs."""

    @staticmethod
    def forward(ctx, *args):
        base, settings_list, cams = args[:8], args[8], args[9:]
        outs = R._RasterizeViews.forward(ctx, *base, [_detached(st) for st in settings_list])
        _arm(ctx, 9, cams)
        return outs

    @staticmethod
    def backward(ctx, *grads):
        return R._RasterizeViews.backward(ctx, *grads) + _camera_grads(ctx)


_N_MODEL = 1 + len(model_path.ARG_NAMES) + 2                 # means2D, the fourteen tensors, settings, model


class _RasterizeModelCam(torch.autograd.Function):
    """model_path._RasterizeModel + (viewmatrix, projmatrix, campos) as inputs."""

    @staticmethod
    def forward(ctx, *args):
        base, cams = list(args[:_N_MODEL]), args[_N_MODEL:]
        base[-2] = _detached(base[-2])
        outs = model_path._RasterizeModel.forward(ctx, *base)
        _arm(ctx, _N_MODEL, cams)
        return outs

    @staticmethod
    def backward(ctx, *grads):
        return model_path._RasterizeModel.backward(ctx, *grads) + _camera_grads(ctx)


class _RasterizeModelViewsCam(torch.autograd.Function):
    """model_path._RasterizeModelViews + 3K camera tensors as inputs."""

    @staticmethod
    def forward(ctx, *args):
        base, cams = list(args[:_N_MODEL]), args[_N_MODEL:]
        base[-2] = [_detached(st) for st in base[-2]]
        outs = model_path._RasterizeModelViews.forward(ctx, *base)
        _arm(ctx, _N_MODEL, cams)
        return outs

    @staticmethod
    def backward(ctx, *grads):
        return model_path._RasterizeModelViews.backward(ctx, *grads) + _camera_grads(ctx)


# What the four public routes call in place of the usual node's `apply` (same arguments, same outputs).
def apply_gaussians(*args):
    return _RasterizeGaussiansCam.apply(*args, *_camera_tensors((args[8],)))


def apply_views(*args):
    return _RasterizeViewsCam.apply(*args, *_camera_tensors(args[8]))


def apply_model(*args):
    return _RasterizeModelCam.apply(*args, *_camera_tensors((args[-2],)))


def apply_model_views(*args):
    return _RasterizeModelViewsCam.apply(*args, *_camera_tensors(args[-2]))

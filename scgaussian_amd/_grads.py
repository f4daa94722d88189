"""The gradient arena of a backward: its segment layout, the pool that keeps arenas from step to step, and the promise a kept
arena carries about its SH gradients.  One owner for the operator's tensor path (rasterizer._backward_view) and the model path
(model_path._grad_arena); the module switches stay attributes of `rasterizer` and are passed in (`pool`).

A backward writes every parameter gradient into one flat fp32 arena and autograd keeps views of it as the .grad tensors
(data-parallel training all-reduces the arena in place instead of packing / unpacking a bucket, parallel.GradBucket).  The arenas
of a layout are pooled: one is handed out again once nobody outside the pool references its storage any more (the previous step's
.grad tensors are gone: optimizer.zero_grad(set_to_none=True), p.grad = None).  What that buys: the arena REMEMBERS that its
SH-coefficient gradients above the active degree hold zeros — written by the kernel the first time — and the next backward is told
to leave them alone (SCG_BACKWARD_SH_TAIL_ZERO): at degree 0 the geometry backward stores 12 instead of 192 bytes of SH gradient
per Gaussian (the reference trains 1 000 iterations at degree 0 and 1 000 at degree 1, train.py:129).  The promise holds while
(a) nobody but the pool and this step's autograd references the storage and (b) no torch operation wrote through any view of it
since (the views share the arena's version counter: zero_grad(set_to_none=False), an in-place all-reduce or clip bump it) —
otherwise the kernel writes the zeros again.  It is DECIDED before a backward's launch (sh_tail_flag) and RECORDED only after the
library call has returned success (commit_promise); a call that failed leaves an arena nobody knows anything about
(invalidate_promise).  A view that ADDS to the arena (`into`) moves the zeros up to its own degree when that is the higher one.

The pool keeps, per (path, device), the arenas of the two most recently used layouts: a densification changes the Gaussian
count and with it the layout — the arenas of the count before last go back to torch's allocator at once.
"""
from __future__ import annotations

import math

import torch

from ._lib import BACKWARD_SH_TAIL_ZERO

# Order of the segments in the tensor path's arena.  The SH gradients come LAST of the usual five: the other four (11 floats per
# Gaussian) are then one contiguous span, which parallel.GradBucket all-reduces in place when only the active SH coefficients
# of a degree-limited step are exchanged (round 5).
_GRAD_ORDER = ("means3D", "opacities", "scales", "rotations", "shs", "colors_precomp", "cov3D_precomp")
_GRAD_SLOTS = tuple(zip(_GRAD_ORDER, (0, 1, 4, 5, 2, 3, 6)))     # ... with the position of each in the `inputs` 7-tuple

_LAYOUTS = {}                            # ((name, shape), ...) -> (names, sizes, shapes, total)
_ARENA_POOLS = {}                        # (path, device index) -> [(layout, [_PooledArena])], least recently used layout first
_ARENA_POOL_LAYOUTS = 2                  # layouts kept per (path, device): the current one and the one before
_ARENA_POOL_DEPTH = 3                    # arenas kept per layout (a step holds one; gradient accumulation over two steps: two)
_use_count = getattr(torch._C, "_storage_Use_Count", None)


def layout(items):
    """(names, sizes, shapes, total) of the arena that holds one fp32 segment per (name, shape) of `items` (a tuple), in that
    order: sizes in floats, padded to 16 bytes.  Depends on the shapes only: looked up, not rebuilt per step."""
    lay = _LAYOUTS.get(items)
    if lay is None:
        if len(_LAYOUTS) > 64:
            _LAYOUTS.clear()
        sizes = [(math.prod(shp) + 3) // 4 * 4 for _, shp in items]
        lay = _LAYOUTS[items] = (tuple(n for n, _ in items), sizes, tuple(tuple(shp) for _, shp in items), max(sum(sizes), 4))
    return lay


def carve(arena, lay, out=None) -> dict:
    """{name: the segment of `arena` as a tensor of the parameter's shape} for a layout() (added to `out` when given)."""
    names, sizes, shapes, total = lay
    used = sum(sizes)
    out = {} if out is None else out
    for n, v, sz, shp in zip(names, (arena if total == used else arena[:used]).split_with_sizes(sizes), sizes, shapes):
        count = math.prod(shp)
        out[n] = (v if sz == count else v[:count]).view(shp)
    return out


class _PooledArena:
    __slots__ = ("arena", "storage", "version", "zero_from", "cstruct")

    def __init__(self, total, dev):
        self.arena = torch.empty((total,), dtype=torch.float32, device=dev)
        self.storage = self.arena.untyped_storage()
        self.version = -1
        self.zero_from = None            # SH coefficients >= this index hold zeros (None: unknown)
        self.cstruct = None              # model_path: the ScgModelGrads struct of this arena's segments

    def free(self) -> bool:
        return _use_count(self.storage._cdata) == 2          # the arena tensor and the wrapper above, nobody else


def _take_arena(path, key, total, dev, pool=True):
    """(arena tensor, pooled record or None) for the layout `key` (the layout() itself: found again by identity, step after
    step, without hashing it) of `path` ("tensors" / "model").  Not pooled: the switch is off, no use-count query in this torch,
    or a stream capture is in progress (a captured step's buffers belong to its graph's memory pool and are replayed in place)."""
    if not pool or _use_count is None or (dev.type == "cuda" and torch.cuda.is_current_stream_capturing()):
        return torch.empty((total,), dtype=torch.float32, device=dev), None
    held = _ARENA_POOLS.get((path, dev.index))
    if held is None:
        held = _ARENA_POOLS[(path, dev.index)] = []
    if held and (held[-1][0] is key or held[-1][0] == key):  # the usual case: the layout of the step before
        arenas = held[-1][1]
    else:
        for i, (k, arenas) in enumerate(held):
            if k == key:
                held.append(held.pop(i))                     # (most recently used last)
                break
        else:
            arenas = []
            del held[: len(held) + 1 - _ARENA_POOL_LAYOUTS]  # the least recently used layout's arenas leave the pool
            held.append((key, arenas))
    for pa in arenas:
        if pa.free():
            return pa.arena, pa
    pa = _PooledArena(total, dev)
    if len(arenas) < _ARENA_POOL_DEPTH:
        arenas.append(pa)
    return pa.arena, pa


def sh_tail_flag(pa, n_active: int) -> int:
    """SCG_BACKWARD_SH_TAIL_ZERO when the pooled arena is known to hold zeros in every SH coefficient >= n_active, else 0.
    Decides only: what the backward leaves behind is recorded by commit_promise once the launch has succeeded."""
    if pa is None or pa.zero_from is None or pa.zero_from > n_active or pa.version != pa.arena._version:
        return 0
    return BACKWARD_SH_TAIL_ZERO


def commit_promise(pa, n_active: int, accumulated: bool):
    """After a backward whose library call returned success.  One that WROTE the arena left values below n_active and zeros
    (kept or written) from there on.  One that ADDED to it (`into`) left non-zero values below its own n_active: the zeros
    begin at the higher of the two — if they were known, and no torch operation wrote the arena in between."""
    if pa is None:
        return
    if not accumulated:
        pa.zero_from, pa.version = n_active, pa.arena._version
    elif pa.zero_from is not None:
        pa.zero_from = max(pa.zero_from, n_active) if pa.version == pa.arena._version else None


def invalidate_promise(pa):
    """A backward failed: nothing is known about what the arena holds."""
    if pa is not None:
        pa.zero_from = None


def _grad_outputs(inputs, into, d_means2D_out, dev, pool=True):
    """Output tensors of a tensor-path backward: every parameter gradient a view of ONE flat fp32 arena (16-byte aligned
    segments) + "_pooled", the arena's pooled record — or, when `into` is the result of an earlier backward over the same inputs,
    those very tensors (the kernel then ADDS to them: views-per-step accumulation).  dL/dmeans2D belongs to the view: always a
    tensor of its own."""
    d_means2D = d_means2D_out if d_means2D_out is not None else torch.empty_like(inputs[0])
    if into is not None:
        out = dict(into)
    else:
        lay = layout(tuple([(n, inputs[i].shape) for n, i in _GRAD_SLOTS if inputs[i] is not None]))
        arena, pooled = _take_arena("tensors", lay, lay[3], dev, pool)
        out = carve(arena, lay, dict.fromkeys(_GRAD_ORDER))
        out["_pooled"] = pooled
    out["means2D"] = d_means2D
    return out


def grad_arena(params):
    """The flat fp32 tensor that holds every `p.grad` of the latest rasterizer backward, when they all live in ONE
    storage (a backward writes every parameter gradient into one allocation and autograd keeps those views as
    `.grad` when it was None) and TILE a range of it; else None.  The range starts at the first of the given gradients
    and ends behind the last: a subset of the parameters (only the opacities, say) yields only its own span, and a subset
    with another parameter's gradient in between yields None — an all-reduce of the result never touches a gradient
    that was not asked for.  Nothing is registered anywhere: the arena is rebuilt from the gradients' shared storage, so
    it lives exactly as long as a gradient does."""
    if not params or params[0].grad is None:
        return None
    st = params[0].grad.untyped_storage()
    base = st.data_ptr()
    begin, end, covered = None, 0, 0
    for p in params:
        g = p.grad
        if g is None or g.dtype != torch.float32 or not g.is_contiguous() or g.untyped_storage().data_ptr() != base:
            return None
        off = g.storage_offset()
        begin = off if begin is None else min(begin, off)
        end = max(end, off + g.numel())
        covered += g.numel()
    # segments are padded to 16 bytes (<= 3 floats each): anything more between them is somebody else's memory
    if end * 4 > st.nbytes() or (end - begin) - covered > 3 * len(params):
        return None
    return torch.empty((0,), dtype=torch.float32, device=params[0].grad.device).set_(st, begin, (end - begin,))

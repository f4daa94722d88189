"""Host-side mirror of the reference's rasterizer operator API, on top of the C-ABI HIP library.

Mirrors (names, argument meaning, error behaviour) the package the reference imports at
gaussian_renderer/__init__.py:15 and uses at :38-53 and :100-108:

    GaussianRasterizationSettings(image_height, image_width, tanfovx, tanfovy, bg, scale_modifier,
                                  viewmatrix, projmatrix, sh_degree, campos, prefiltered, debug)
    GaussianRasterizer(raster_settings)(means3D, means2D, opacities, shs=None, colors_precomp=None,
                                        scales=None, rotations=None, cov3D_precomp=None)
        -> (color (3,H,W), radii (P,) int32, depth (1,H,W), alpha (1,H,W))

PyTorch is plumbing here (device memory, the current stream, autograd graph edges); every stage of the
computation runs in hand-written HIP kernels behind include/scg_raster.h.  There is no fallback path.

What lives where: this module owns the operator — the forwards and the backward as sequences of library calls (forward_fused: mode,
capacity look-up, _launch_forward per attempt, overflow retry), the module switches, the K-view core of the four autograd nodes.
The capacity policy with its tables, pinned partial sums, workspace plans and count words: _counts.py; frames and per-camera launch
hints: _frames.py; the gradient arena: _grads.py; camera identity: _cameras.py; the stage timer: _timing.py; option and flag bits: _lib.py;
the gradients with respect to the camera (sibling nodes of the four, the pass _backward_view calls for them): camera_grad.py.

Concurrency: the operator is re-entrant per device and stream, like the upstream extension — every forward takes its own
pinned scratch (the partial sums of num_rendered) from a per-device pool, so two threads, each on its own stream, may be
inside a forward at the same time (round 5; before, the second one raised).  The host-side hint tables (capacities, tile
costs) are plain dictionaries updated under the GIL: a concurrent update costs a hint, never a result.  Forward and
backward may run on different threads (autograd's device thread) and on any stream; several forwards may be
outstanding before their backwards run (each keeps its own saved state).  The inputs are saved with
ctx.save_for_backward: modifying one in place between forward and backward raises autograd's version-counter error,
as it does with the reference's operator.
"""
from __future__ import annotations

import contextlib
import ctypes as C
from typing import Callable, NamedTuple, Optional

import torch
import torch.nn as nn

from . import _counts, _grads, _lib, _timing
# (names this module does not use itself are what bench.py, tests and tools read here)
from ._cameras import _CAM_KEYS, _camera_key, tag_camera                                               # noqa: F401
from ._counts import (_OVERFLOW, _QUARANTINE, _SPEC_STATE, _CountWord, _capacity_for, _count_word, _next_capacity,      # noqa: F401
                      _settle_camera, _settle_word, _spec_state, overflow_stats, settle_counts)
from ._frames import _CAM_HINTS, _FRAME_CACHE, _f32c, _frame_for, _stream                              # noqa: F401
# _sh_tail_promise is the DECISION about the promise a kept gradient arena carries about its SH tails: the backward of both paths
# looks it up here at call time (tests spy on it)
from ._grads import _grad_outputs, grad_arena, sh_tail_flag as _sh_tail_promise                        # noqa: F401
from ._lib import (BACKWARD_ACCUMULATE, BINNING_AUTO, DEBUG_SEPARATE_HIST, DEBUG_SEPARATE_SORT, DSPLAT_FLOATS,
                   FORWARD_ARM_PARTIAL_SUMS, FORWARD_NO_BACKWARD_STATE, FORWARD_RARE_8WAVE, FORWARD_SKIP_RARE_SORT,
                   FORWARD_SPLIT_LONG_LISTS, SPLAT_FLOATS, TILE, check, ptr)                           # noqa: F401
from ._timing import StageTimer, set_stage_timer                                                       # noqa: F401


class GaussianRasterizationSettings(NamedTuple):
    image_height: int
    image_width: int
    tanfovx: float
    tanfovy: float
    bg: torch.Tensor
    scale_modifier: float
    viewmatrix: torch.Tensor
    projmatrix: torch.Tensor
    sh_degree: int
    campos: torch.Tensor
    prefiltered: bool
    debug: bool


def _kernel_inputs(dev, *tensors):
    """The operator's seven inputs (means3D, opacities, shs, colors_precomp, scales, rotations, cov3D_precomp) as the kernels read
    them (_f32c; None for an absent or empty one) + M, the SH coefficients per Gaussian."""
    inputs = tuple([_f32c(t, dev) for t in tensors])
    return inputs, (inputs[2].shape[1] if inputs[2] is not None else 0)


# ---- module switches (round 5: no environment variables in the product — tests and the same-process A/B tool
# tools/ab_inproc.py flip these attributes; a caller never needs to) ------------------------------------------------------
# Order the blend kernels' tiles by what they cost the last time the same camera was rendered (False: by list length always).
TILE_COST_HINT = True
# ... and the blend backward's (tile, quadrant) waves by how long each took in the camera's previous backward
# (ScgFrame.bwd_cost_in; False: they follow the tiles' order)
BWD_ORDER_HINT = True
# Skip the launch of the rare-size sort kernel while the previous render of the same camera found no list beyond the forward
# blend's own sort (scg_raster.h SCG_FORWARD_SKIP_RARE_SORT; False: always launch it).
SKIP_IDLE_RARE_SORT = True
# ... and partition the lists beyond 4 096 entries (kSort8Max) by depth first when that render found very long ones
# (SCG_FORWARD_SPLIT_LONG_LISTS; False: one workgroup sorts each long list as before)
SPLIT_LONG_LISTS = True
# ... sorted, like the other lists beyond the forward blend's own sort, by 8-wave workgroups three per compute unit
# (SCG_FORWARD_RARE_8WAVE; False: the 16-wave rare-size kernel, one workgroup per compute unit, as on a first render)
RARE_8WAVE = True


def _frame_switches():
    """What _frames needs of the switches, read per forward: cost buffers exist, bwd_cost_in is handed over, long words wanted."""
    return TILE_COST_HINT, BWD_ORDER_HINT, SKIP_IDLE_RARE_SORT or RARE_8WAVE


def _rare_options(words) -> int:
    """scg_forward option bits from what the camera's previous render left in ScgFrame.long_lists_out."""
    if words is None or words[0] < 0:
        return 0                                             # nothing known yet: the rare-size kernel as in the staged calls
    if words[0] == 0:
        return FORWARD_SKIP_RARE_SORT if SKIP_IDLE_RARE_SORT else 0
    # very long lists (beyond 16 384 entries): split everything beyond 4 096 by depth + 8-wave work-list sort; without them the
    # 16-wave rare-size kernel finishes its handful of lists in one round (measured: 30 %-clustered scene 64.6 vs 73.3 us)
    if RARE_8WAVE and SPLIT_LONG_LISTS and words[1] > 0:
        return FORWARD_RARE_8WAVE | FORWARD_SPLIT_LONG_LISTS
    return 0


class _on_device:
    """`with torch.cuda.device(dev)` only when dev is not already the current device (the common case skips it)."""

    def __init__(self, device):
        self.ctx = None
        if device.index is not None and torch._C._cuda_getDevice() != device.index:
            self.ctx = torch.cuda.device(device)

    def __enter__(self):
        if self.ctx is not None:
            self.ctx.__enter__()

    def __exit__(self, *a):
        if self.ctx is not None:
            self.ctx.__exit__(*a)


def _require_cuda(t: torch.Tensor):
    if not t.is_cuda:
        raise _lib.ScgError("scgaussian_amd rasterizer needs tensors on a ROCm GPU ('cuda' device); "
                            "there is no CPU path in the product (the CPU oracle lives under oracle/, tests only)")


_ELEMENT_SIZE = {torch.float32: 4, torch.int32: 4, torch.uint8: 1, torch.int64: 8}


class _Arena:
    """One device allocation carved into aligned sub-buffers addressed by raw pointer (internal state never
    becomes a tensor unless a caller asks for a view): fewer torch allocations / tensor objects per call."""

    def __init__(self, sizes, device):
        self.offsets = []
        off = 0
        for nbytes in sizes:
            self.offsets.append(off)
            off += (int(nbytes) + 255) // 256 * 256
        self.buf = torch.empty((max(off, 256),), dtype=torch.uint8, device=device)
        self.base = self.buf.data_ptr()

    def ptr(self, i: int) -> int:
        return self.base + self.offsets[i]

    def view(self, i: int, shape, dtype) -> torch.Tensor:
        n = 1
        for d in shape:
            n *= int(d)
        nbytes = n * _ELEMENT_SIZE[dtype]
        return self.buf[self.offsets[i]: self.offsets[i] + nbytes].view(dtype).view(shape)


# what the speculation cost so far (speculation_stats(); bench.py `moving_scene`): forwards on the one-call path, how many of them
# had to be repeated because num_rendered exceeded the capacity, forwards that took the staged path (first sight of a shape, images
# beyond the tile-first binning), and how many one-call forwards had a launch-order hint of their camera's previous render
_SPEC_STATS = {"one_call_forwards": 0, "overflow_retries": 0, "staged_forwards": 0, "tile_cost_hints": 0, "bwd_order_hints": 0}


def speculation_stats(reset: bool = False) -> dict:
    """Counters of the speculative launch since the process started (or the last reset): see _SPEC_STATS."""
    out = dict(_SPEC_STATS)
    if reset:
        for k in _SPEC_STATS:
            _SPEC_STATS[k] = 0
    return out


SPECULATIVE_LAUNCH = True       # module switch (tests flip it to cover both paths)
# scg_forward lets the forward blend sort the tiles' lists itself and the geometry kernel build the binning stage's slice
# histograms; False passes the library's A/B bits (csrc/scg_debug.h: SCG_DEBUG_SEPARATE_SORT / _HIST — not part of the public
# header) so that the suite can hold the fused kernels against the separate ones bit for bit
FUSED_SORT = True
FUSED_HIST = True
# scg_forward's partial sums of num_rendered are collected by watching the pinned words (SCG_FORWARD_ARM_PARTIAL_SUMS) instead
# of waiting on an event recorded behind the geometry kernel (module switch for same-process A/B runs)
EVENTLESS_WAIT = True


def forward_stages(settings: GaussianRasterizationSettings, means3D, opacities, shs=None, colors_precomp=None,
                   scales=None, rotations=None, cov3D_precomp=None, want_keys: bool = False,
                   timer: Optional[Callable] = None, binning_algo: int = BINNING_AUTO, capacity_hint: Optional[int] = None,
                   prepare_backward: bool = False):
    """Run the forward stages through the C ABI and return every intermediate (used by the autograd
    function and, with want_keys=True, by the parity tests).

    Host/GPU overlap: the binning buffers are sized by num_rendered, which only the GPU knows.  Instead of
    stalling on that read, stages 2-3 are enqueued at once with an upper-bound guess (1.25 x the largest count seen
    for this problem shape); num_rendered travels to pinned host memory on the same stream and is checked after
    the launches.  A guess that was too small (rare) re-runs stages 2-3 with the exact size.  `capacity_hint`
    overrides the guess (tests)."""
    _require_cuda(means3D)
    lib = _lib.load()
    _SPEC_STATS["staged_forwards"] += 1
    timer = timer or _timing.ACTIVE
    dev = means3D.device
    spec = _spec_state(dev)
    inputs, M = _kernel_inputs(dev, means3D, opacities, shs, colors_precomp, scales, rotations, cov3D_precomp)
    means3D, opacities, shs, colors_precomp, scales, rotations, cov3D_precomp = inputs
    P = 0 if means3D is None else means3D.shape[0]
    fr = _frame_for(settings, P, M, dev, True, None, _frame_switches())
    H, W = fr.H, fr.W
    with _on_device(dev):
        stream = _stream(dev)
        # per-Gaussian state: [0] splats  [1] rects  [2] depth_keys  [3] clamped  [4] geometry scratch  [5] num_rendered
        gscratch = lib.scg_geometry_scratch_bytes(P)
        ga = _Arena([P * SPLAT_FLOATS * 4, P * 8, P * 4, P, gscratch, 4], dev)
        radii = torch.empty((P,), dtype=torch.int32, device=dev)
        guess = capacity_hint if capacity_hint is not None else _counts.lookup_shape(spec, P, W, H)
        speculative = (SPECULATIVE_LAUNCH or capacity_hint is not None) and guess is not None and P > 0 and \
            not want_keys and \
            lib.scg_binning_accepts_bound(int(guess), W, H, binning_algo) == 1
        pinned = spec.take(gscratch) if speculative else None
        with timer("geometry_forward"):
            # speculative: partial sums of num_rendered go straight to pinned host memory, no on-device total
            check(lib.scg_geometry_forward(fr.ref, ptr(means3D), ptr(opacities), ptr(shs), ptr(colors_precomp),
                                           ptr(scales), ptr(rotations), ptr(cov3D_precomp), ga.ptr(0), ptr(radii),
                                           ga.ptr(3), ga.ptr(1), ga.ptr(2), None if speculative else ga.ptr(5),
                                           pinned.ptr if speculative else ga.ptr(4), gscratch, stream),
                  "scg_geometry_forward")
        if speculative:
            pinned.torch_event().record()
            R = None
            cap = int(guess)
        else:
            nr = ga.view(5, (1,), torch.int32)
            R = int(nr.item()) & 0xFFFFFFFF          # the one host read of the path (sizes the binning buffers)
            cap = R

        img = torch.empty((5, H, W), dtype=torch.float32, device=dev)          # one allocation, three views
        color, depth, alpha = img[0:3], img[3:4], img[4:5]

        # gradient records of the coming backward: cleared by the forward blend kernel (no memset launch later)
        dsplats = torch.empty((P, DSPLAT_FLOATS), dtype=torch.float32, device=dev) if prepare_backward and P > 0 else None

        def bin_and_blend(capacity):
            # [0] point_list  [1] ranges  [2] final_T  [3] n_contrib  [4] binning scratch  [5] keys (debug)
            scratch_bytes = lib.scg_binning_scratch_bytes(P, capacity, W, H, binning_algo)
            ba = _Arena([capacity * 4, lib.scg_ranges_words(W, H) * 4, H * W * 4, H * W * 4, scratch_bytes,
                         capacity * 8 if want_keys else 0], dev)
            with timer("binning"):
                check(lib.scg_binning(fr.ref, capacity, ga.ptr(1), ga.ptr(2), ba.ptr(0), ba.ptr(1),
                                      ba.ptr(5) if want_keys else None, binning_algo, ba.ptr(4), scratch_bytes, stream),
                      "scg_binning")
            with timer("blend_forward"):
                check(lib.scg_blend_forward(fr.ref, ba.ptr(1), ba.ptr(0), ga.ptr(0), ptr(color), ptr(depth), ptr(alpha),
                                            ba.ptr(2), ba.ptr(3), ptr(dsplats), stream), "scg_blend_forward")
            return ba

        ba = bin_and_blend(cap)
        # everything that does not need num_rendered is done BEFORE the wait: what follows the wait sits on the
        # critical path of a training step (the GPU has ~0.13 ms of forward queued, the host needs longer than that
        # to get from here to the launch of the backward)
        out = _LazyViews(dict(color=color, depth=depth, alpha=alpha, radii=radii, num_rendered=R, dsplats_zeroed=dsplats,
                              arenas=(ga, ba), capacity=cap, n_tiles=fr.n_tiles, hw=(H, W), P=P, frame=fr,
                              ptrs=dict(splats=ga.ptr(0), clamped=ga.ptr(3), point_list=ba.ptr(0), ranges=ba.ptr(1),
                                        final_T=ba.ptr(2), n_contrib=ba.ptr(3)),
                              inputs=inputs),
                         want_keys)
        if speculative:
            pinned.torch_event().synchronize()
            R = int(pinned.np[: (P + 255) // 256].sum(dtype="int64"))
            spec.give_back(pinned)
            if R > cap:                              # the guess was too small: lists were clipped, run again
                ba = bin_and_blend(R)
                cap = R
                out["arenas"] = (ga, ba)
                out["capacity"] = cap
                out["ptrs"].update(point_list=ba.ptr(0), ranges=ba.ptr(1), final_T=ba.ptr(2), n_contrib=ba.ptr(3))
            out["num_rendered"] = R
        if capacity_hint is None:
            _counts.commit_shape(spec, P, W, H, R)
    return out


class _LazyViews(dict):
    """forward_stages result: internal buffers become tensors only when somebody indexes them (tests, tools)."""

    _SPECS = {
        "splats": (0, 0, lambda d: (d["P"], SPLAT_FLOATS), torch.float32),
        "rects": (0, 1, lambda d: (d["P"], 2), torch.int32),
        "depth_keys": (0, 2, lambda d: (d["P"],), torch.int32),
        "clamped": (0, 3, lambda d: (d["P"],), torch.uint8),
        "point_list": (1, 0, lambda d: (d["num_rendered"],), torch.int32),
        "ranges": (1, 1, lambda d: (d["n_tiles"], 2), torch.int32),
        "final_T": (1, 2, lambda d: d["hw"], torch.float32),
        "n_contrib": (1, 3, lambda d: d["hw"], torch.int32),
        "keys_sorted": (1, 5, lambda d: (d["num_rendered"],), torch.int64),
    }

    def __init__(self, d, want_keys):
        super().__init__(d)
        self._want_keys = want_keys

    def __missing__(self, k):
        spec = self._SPECS.get(k)
        if spec is None or (k == "keys_sorted" and not self._want_keys):
            if k == "keys_sorted":
                return None
            raise KeyError(k)
        arena_i, slot, shape_fn, dtype = spec
        v = dict.__getitem__(self, "arenas")[arena_i].view(slot, shape_fn(self), dtype)
        self[k] = v
        return v


ARENA_POOL = True                        # module switch (tests / A-B runs): keep gradient arenas from step to step (_grads.py)


def _backward_view(state, inputs, radii, dL_dcolor, dL_ddepth, dL_dalpha, timer: Optional[Callable] = None, into=None,
                   d_means2D_out=None, want_dsplats: bool = False):
    """One view's backward (stages 4-5) on the path its forward took, which `state` tells: a forward_stages result ("ptrs":
    scg_blend_backward + scg_geometry_backward), a forward_fused state (scg_backward) or, with `inputs` a model_path._ModelArgs
    in place of the 7-tuple of contiguous fp32 input tensors, the model path's (scg_backward_model).  Returns {name: gradient}
    — views of one flat arena, _grads.py — + "means2D".  `into`: the dict an earlier view's call returned for the same inputs:
    this view's parameter gradients are ADDED to it in the kernel.  `want_dsplats`: the gradient records as out["dsplats"] (the
    staged path, where they are a tensor)."""
    lib = _lib.load()
    if not state.get("has_backward_state", True):
        raise _lib.ScgError("this forward ran without backward state (prepare_backward=False -> scg_forward's "
                            "SCG_FORWARD_NO_BACKWARD_STATE: final_T / n_contrib were not written): it cannot be differentiated")
    model = None if isinstance(inputs, (tuple, list)) else inputs
    dev, P = (inputs[0].device, inputs[0].shape[0]) if model is None else (model.device, model.P)
    fr = state["frame"]
    if fr.hints is not None and fr.hints.bcost is not None:
        fr.hints.bwritten = True                             # (this backward records its quadrants' times: the next forward's hint)
    dL_dcolor = _f32c(dL_dcolor, dev)
    if dL_dcolor is None:
        dL_dcolor = torch.zeros((3, fr.H, fr.W), dtype=torch.float32, device=dev)
    dL_ddepth = _f32c(dL_ddepth, dev)
    dL_dalpha = _f32c(dL_dalpha, dev)
    timer = timer or _timing.ACTIVE
    staged = "ptrs" in state
    with _on_device(dev):
        stage_ev = timer.stage_events("backward") if isinstance(timer, StageTimer) and not staged else None
        stream = _stream(dev)
        # the gradient records the forward blend cleared: usable once (a tensor on the staged path, a raw pointer into
        # state["ws"] on the one-call paths); a second backward over one forward takes records of its own
        dsplats = state.get("dsplats_zeroed")
        state["dsplats_zeroed"] = None
        prezeroed = dsplats is not None
        if dsplats is None:
            dsplats = torch.empty((P, DSPLAT_FLOATS), dtype=torch.float32, device=dev)
        records = dsplats if isinstance(dsplats, int) else dsplats.data_ptr()
        out = _grad_outputs(inputs, into, d_means2D_out, dev, ARENA_POOL) if model is None else \
            model.grad_outputs(into, d_means2D_out)
        # the pooled arena's promise about its SH tails: decided here, recorded once the library call has returned success
        pa, n_active = out.get("_pooled"), (fr.c.sh_degree + 1) ** 2
        flags = BACKWARD_ACCUMULATE if into is not None else _sh_tail_promise(pa, n_active)
        try:
            if model is not None:
                check(lib.scg_backward_model(fr.ref, model.ref, radii.data_ptr(), state["cap"], state["ws"].data_ptr(),
                                             dL_dcolor.data_ptr(), ptr(dL_ddepth), ptr(dL_dalpha), records, int(prezeroed),
                                             C.byref(out["_c"]), out["means2D"].data_ptr(), flags, stage_ev, stream),
                      "scg_backward_model")
            else:
                grads = (out["means3D"].data_ptr(), out["means2D"].data_ptr(), out["opacities"].data_ptr(), ptr(out["shs"]),
                         ptr(out["colors_precomp"]), ptr(out["scales"]), ptr(out["rotations"]), ptr(out["cov3D_precomp"]))
                in_ptrs = tuple(None if t is None else t.data_ptr() for t in inputs)
                if staged:
                    sp = state["ptrs"]
                    with timer("blend_backward"):
                        check(lib.scg_blend_backward(fr.ref, sp["ranges"], sp["point_list"], sp["splats"], sp["final_T"],
                                                     sp["n_contrib"], ptr(dL_dcolor), ptr(dL_ddepth), ptr(dL_dalpha), records,
                                                     int(prezeroed), stream), "scg_blend_backward")
                    with timer("geometry_backward"):
                        check(lib.scg_geometry_backward(fr.ref, *in_ptrs, radii.data_ptr(), sp["clamped"], records, *grads,
                                                        flags, stream), "scg_geometry_backward")
                else:
                    check(lib.scg_backward(fr.ref, *in_ptrs, radii.data_ptr(), state["cap"], state["ws"].data_ptr(),
                                           dL_dcolor.data_ptr(), ptr(dL_ddepth), ptr(dL_dalpha), records, int(prezeroed), *grads,
                                           flags, stage_ev, stream), "scg_backward")
        except BaseException:
            _grads.invalidate_promise(pa)
            raise
        _grads.commit_promise(pa, n_active, into is not None)
    camera_pass = state.get("camera_pass")
    if camera_pass is not None:
        # a node that also differentiates the camera (camera_grad.py) armed this view: its pass runs here, behind the geometry
        # backward, while the view's gradient records are in this function's hands
        camera_pass(state, inputs, radii, records, dev)
    if want_dsplats:
        out["dsplats"] = dsplats
    return out


def backward_stages(settings: GaussianRasterizationSettings, inputs, saved, dL_dcolor, dL_ddepth, dL_dalpha,
                    want_dsplats: bool = False, timer: Optional[Callable] = None, into=None, d_means2D_out=None):
    """Blend backward + geometry backward through the C ABI (_backward_view).  `inputs` is the 7-tuple of contiguous fp32
    input tensors, `saved` the forward state: {"ptrs": raw device pointers of splats / clamped / point_list /
    ranges / final_T / n_contrib, "arenas": the allocations that own them, "radii": tensor} — a forward_stages
    result can be passed as is (its cleared gradient records are used up).  `into`, `want_dsplats`: see _backward_view."""
    if saved.get("frame") is None:
        shs = inputs[2]
        saved["frame"] = _frame_for(settings, inputs[0].shape[0], shs.shape[1] if shs is not None else 0, inputs[0].device)
    return _backward_view(saved, inputs, saved["radii"], dL_dcolor, dL_ddepth, dL_dalpha, timer, into, d_means2D_out,
                          want_dsplats)


# ---------------------------------------------------------------------------------------------------------------------
# a forward that never reads the host (round 6; SURVEY §8b "or none, if the caller passes a capacity and the kernel reports
# overflow"; ScgFrame.num_rendered_out)
# ---------------------------------------------------------------------------------------------------------------------
# The default forward spins on the pinned partial sums of num_rendered before it returns (scg_wait_num_rendered): it hands back
# a result that is known to be complete, and it cannot be captured in a hipGraph.  With NO_HOST_READ (or whenever torch's current
# stream is capturing) the forward is launched with the capacity the camera's earlier renders established and returns at once;
# the binning stage leaves the count it found in one pinned word (ScgFrame.num_rendered_out) and the binding looks at that word
# the NEXT time it renders the camera (or when somebody asks: settle_counts()): a count beyond the capacity means that render's
# lists were clipped (its images and gradients miss the tail of the tile order) — it is counted in overflow_stats(), the camera's
# capacity is raised, and the next render is complete again: one step late, as the reference's own loop would notice a bad
# iteration one `loss.item()` late (train.py:176).  graph_step.CapturedStep builds on this: forward + backward captured once
# and replayed, the word checked before every replay, the step re-captured with room for the count after an overflow.
NO_HOST_READ = False


@contextlib.contextmanager
def no_host_read(enabled: bool = True):
    """`with no_host_read():` — every forward inside is launched without waiting for num_rendered (see NO_HOST_READ)."""
    global NO_HOST_READ
    prev, NO_HOST_READ = NO_HOST_READ, bool(enabled)
    try:
        yield
    finally:
        NO_HOST_READ = prev


# ---------------------------------------------------------------------------------------------------------------------
# the fast path: ONE C-ABI call per direction (include/scg_raster.h scg_forward / scg_backward)
# ---------------------------------------------------------------------------------------------------------------------
def _launch_forward(lib, fr, P, dev, model, in_ptrs, plan, cap, outs, pinned, ev, cw, prepare_backward, stage_ev, stream):
    """ONE attempt of forward_fused at capacity `cap`: the workspace, the option word, where the count goes, the library call.
    `outs`: the addresses of radii, colour, depth, alpha; `pinned`: this forward's pinned partial sums — None for a forward that
    does not read the host, whose count arrives in the count word `cw`.  Returns (workspace, address of the cleared gradient
    records or None)."""
    # the gradient records of the coming backward (cleared by the forward blend) live behind the workspace in the same
    # allocation: one torch.empty less per step (they are only ever addressed by raw pointer); without a host read the geometry
    # kernel's partial sums of num_rendered go to device memory behind the records: nobody reads them — the count comes from
    # the binning stage, ScgFrame.num_rendered_out
    ds_bytes = (P * DSPLAT_FLOATS * 4 + 64) if prepare_backward else 0
    ws = torch.empty((plan.total + ds_bytes + (plan.partial_bytes + 256 if pinned is None else 0),), dtype=torch.uint8, device=dev)
    wp = ws.data_ptr()
    dsplats = ((wp + plan.total + 63) & ~63) if prepare_backward else None       # 64-byte aligned records
    # num_rendered without an event (ABI 9): the pinned words are armed by scg_forward and watched by scg_wait_num_rendered — no
    # barrier packet behind the geometry kernel, no event wake-up
    options = (0 if FUSED_SORT else DEBUG_SEPARATE_SORT) | (0 if FUSED_HIST else DEBUG_SEPARATE_HIST) | \
        (0 if prepare_backward else FORWARD_NO_BACKWARD_STATE) | _rare_options(fr.long_np) | \
        (FORWARD_ARM_PARTIAL_SUMS if (ev is None and pinned is not None) else 0)
    if fr.long_np is not None and fr.long_np[0] >= 0 and not plan.sorts_in_blend(lib, options):
        # nobody writes the words in this frame: what an earlier, sparser frame of the camera left there is stale
        fr.long_np[:] = -1
        options &= ~(FORWARD_SKIP_RARE_SORT | FORWARD_RARE_8WAVE | FORWARD_SPLIT_LONG_LISTS)
    if pinned is None:
        fr.c.num_rendered_out = cw.ptr
        sums = (wp + plan.total + ds_bytes + 255) & ~255
    else:
        fr.c.num_rendered_out = None
        sums = pinned.ptr
    try:
        if model is None:
            check(lib.scg_forward(fr.ref, *in_ptrs, cap, wp, plan.total, *outs, sums, ev, dsplats, options, stage_ev, stream),
                  "scg_forward")
        else:
            check(lib.scg_forward_model(fr.ref, model.ref, cap, wp, plan.total, *outs, sums, ev, dsplats, options, stage_ev,
                                        stream), "scg_forward_model")
    finally:
        fr.c.num_rendered_out = None
    return ws, dsplats


def forward_fused(settings: GaussianRasterizationSettings, means3D, opacities, shs, colors_precomp, scales, rotations,
                  cov3D_precomp, prepare_backward: bool, timer: Optional[Callable] = None, model=None):
    """Stages 1-3 in one library call, laid out in one workspace allocation, enqueued without a host read: the capacity
    (upper bound of num_rendered) comes from the previous calls of this camera or problem shape (_counts.lookup).  Returns None
    when the fast path does not apply (no capacity known yet, image too large for the tile-first binning): the caller then takes
    the staged path, which also establishes the capacity.  Otherwise (color, radii, depth, alpha, state).
    `model` (model_path._ModelArgs): the reference model's raw parameter tensors in place of the seven activated inputs
    (scg_forward_model); a model's first render starts from a generous bound instead of the staged path."""
    dev = means3D.device if model is None else model.device
    spec = _spec_state(dev)
    P = means3D.shape[0] if model is None else model.P
    H, W = int(settings.image_height), int(settings.image_width)
    cam = _camera_key(settings.viewmatrix)   # the content of the view matrix: an address can be recycled for another camera
    ckey = (W, H, cam)
    # a forward that must not read the host: asked for (NO_HOST_READ) or inside a stream capture (a host read cannot be captured)
    capturing = torch.cuda.is_current_stream_capturing()
    no_read = NO_HOST_READ or capturing
    if spec.pending:
        _settle_camera(spec, ckey)                           # counts of this camera's earlier no-host-read renders that have arrived
    cap = _counts.lookup(spec, P, W, H, cam, capturing, model is not None or no_read)
    if cap is None or P == 0 or not SPECULATIVE_LAUNCH:
        if capturing:
            raise _lib.ScgError("a rasterizer forward inside a stream capture needs the one-call path (P > 0, SPECULATIVE_LAUNCH)")
        return None
    lib = _lib.load()
    plan = spec.plan(lib, P, W, H, cap)
    if not plan.accepts:
        if capturing:
            raise _lib.ScgError("a rasterizer forward inside a stream capture needs the tile-first binning "
                                "(scg_binning_accepts_bound): this image / capacity takes the staged path, which reads the host")
        return None
    pinned = None if no_read else spec.take(plan.partial_bytes)   # this forward's pinned words (returned once num_rendered is read)
    cw = taken = None                        # the count word of a forward that does not read the host; `taken`: not filed yet
    try:
        if model is None:
            inputs, M = _kernel_inputs(dev, means3D, opacities, shs, colors_precomp, scales, rotations, cov3D_precomp)
            in_ptrs = tuple(None if t is None else t.data_ptr() for t in inputs)
        else:
            inputs, M, in_ptrs = model.tensors, 16, None
        fr = _frame_for(settings, P, M, dev, True, cam, _frame_switches())
        _SPEC_STATS["one_call_forwards"] += 1
        if fr.c.tile_cost_in:
            _SPEC_STATS["tile_cost_hints"] += 1
        if fr.c.bwd_cost_in:
            _SPEC_STATS["bwd_order_hints"] += 1
        timer = timer or _timing.ACTIVE
        with _on_device(dev):
            stage_ev = timer.stage_events("forward") if isinstance(timer, StageTimer) else None
            stream = _stream(dev)
            ev = None if (EVENTLESS_WAIT or no_read) else pinned.event_handle()
            img = torch.empty((5, H, W), dtype=torch.float32, device=dev)          # colour | depth | alpha
            radii = torch.empty((P,), dtype=torch.int32, device=dev)
            ip, hw4 = img.data_ptr(), H * W * 4
            outs = (radii.data_ptr(), ip, ip + 3 * hw4, ip + 4 * hw4)
            while True:
                if no_read:
                    cw = taken = _count_word(cap, P, ckey, dev.index)
                ws, dsplats = _launch_forward(lib, fr, P, dev, model, in_ptrs, plan, cap, outs, pinned, ev, cw,
                                              prepare_backward, stage_ev, stream)
                if no_read:
                    # launched, not waited for: the count is looked at when this camera is rendered next (or by settle_counts /
                    # the captured step that owns the word)
                    _counts.file_word(spec, cw, ckey, capturing)
                    taken = R = None
                    break
                R = lib.scg_wait_num_rendered(ev, pinned.ptr, P)
                if R < 0:
                    check(int(R), "scg_wait_num_rendered")
                if R <= cap:
                    _counts.commit(spec, P, W, H, cam, _next_capacity(cap, R), R)
                    break
                # the bound was too small (rare: the scene grew by > 12 % since this camera's last render): lists were
                # clipped, run again with room for the real count
                _SPEC_STATS["overflow_retries"] += 1
                cap = _capacity_for(R)
                plan = spec.plan(lib, P, W, H, cap)
                if not plan.accepts:                 # the larger bound no longer fits the tile-first binning:
                    _counts.forget(spec, P, W, H, cam)           # the staged path (global sort) takes over
                    spec.give_back(pinned)
                    return None
                stage_ev = None
        # "num_rendered": None for a forward that did not read the host ("count_word": where its count arrives)
        state = {"ws": ws, "cap": cap, "plan": plan, "frame": fr, "dsplats_zeroed": dsplats, "num_rendered": R,
                 "inputs": inputs, "has_backward_state": bool(prepare_backward), "count_word": cw}
        if pinned is not None:
            spec.give_back(pinned)               # (num_rendered has been read: no kernel writes these words any more)
        return img[0:3], radii, img[3:4], img[4:5], state
    except BaseException:
        # kernels of the failed call may still be writing ws / img / radii and the pinned words: let them finish before Python
        # frees the buffers, and keep the pinned block out of circulation for good (dropping the reference hands it
        # back to torch's caching host allocator); a count word nobody was handed goes back (a failed capture launched nothing)
        try:
            if not capturing:
                torch.cuda.current_stream(dev).synchronize()
        except Exception:                        # noqa: BLE001 - the original error matters more
            pass
        if pinned is not None:
            _QUARANTINE.append(pinned)
        if taken is not None:
            _counts.release([taken])
        raise


def _forward_view(settings: GaussianRasterizationSettings, inputs, needs_grad: bool):
    """One view's forward for the autograd Functions: the one-call path, else — on the tensor path — the staged one, which also
    establishes the capacity.  `inputs`: the operator's (means3D, opacities, shs, colors_precomp, scales, rotations,
    cov3D_precomp) or a model_path._ModelArgs.  Returns (color, radii, depth, alpha, the inputs as the kernels read them, the
    state _backward_view takes)."""
    model = None if isinstance(inputs, tuple) else inputs
    fused = forward_fused(settings, *(inputs if model is None else (None,) * 7), needs_grad, model=model)
    if fused is not None:
        color, radii, depth, alpha, state = fused
        return color, radii, depth, alpha, state.pop("inputs"), state
    if model is not None:
        raise _lib.ScgError("the model path needs the tile-first binning (scg_binning_accepts_bound): check "
                            "model_path.supported(tensors, settings) first and render through the getters otherwise")
    st = forward_stages(settings, *inputs, prepare_backward=needs_grad)
    # raw pointers into the two arenas (kept alive by the reference to `arenas`)
    state = {"ptrs": st["ptrs"], "arenas": st["arenas"], "dsplats_zeroed": st["dsplats_zeroed"], "frame": st["frame"]}
    return st["color"], st["radii"], st["depth"], st["alpha"], st["inputs"], state


# ---- the K-view core of the four autograd nodes (_RasterizeGaussians and _RasterizeViews here, model_path's _RasterizeModel and
# _RasterizeModelViews); a single-view node is K = 1 without a screen-space gradient slot per view -------------------------------
def _views_forward(ctx, settings_list, inputs, needs_grad):
    """The K views one after the other (_forward_view, `inputs` as there), each with its own state in ctx.states.  Returns
    (color_0, radii_0, depth_0, alpha_0, color_1, ...) and the inputs as the kernels read them."""
    outs, states, kin = [], [], None
    for st_ in settings_list:
        color, radii, depth, alpha, kin, state = _forward_view(st_, inputs, needs_grad)
        states.append(state)
        outs += [color, radii, depth, alpha]
    ctx.states = states
    ctx.inputs_present = tuple(t is not None for t in kin)
    # the inputs (geometry_backward recomputes the forward chain from them) and radii go through autograd's saved
    # tensors: an in-place update between forward and backward trips the version counter instead of silently
    # pairing new parameter values with the splats / radii of the old ones
    if needs_grad:
        ctx.save_for_backward(*[t for t in kin if t is not None], *outs[1::4])
    ctx.mark_non_differentiable(*outs[1::4])
    ctx.set_materialize_grads(False)       # missing output gradients arrive as None, not as zero-filled tensors
    return tuple(outs), kin


def _views_backward(states, inputs, radii_all, grads, per_view_slots):
    """Per view blend backward + geometry backward (_backward_view; `grads`: the flat output gradients).  Returns ({name: gradient},
    dL/dmeans2D).  `per_view_slots`: means2D is (K, P, 3) and the second and later views ADD their parameter gradients to the
    first one's in the kernel (`into`); (None, None) when no view reached the loss.  Otherwise K = 1 and dL/dmeans2D is (P, 3)."""
    if not per_view_slots:
        g = _backward_view(states[0], inputs, radii_all[0], grads[0], grads[2], grads[3])
        return g, g["means2D"]
    K = len(states)
    dev, P = (inputs[0].device, inputs[0].shape[0]) if isinstance(inputs, tuple) else (inputs.device, inputs.P)
    # the library writes a view's (P, 3) slot completely (zeros for culled Gaussians): no fill launch over K x P x 12 bytes;
    # only the slot of a view whose outputs did not reach the loss is cleared here
    d_means2D = torch.empty((K, P, 3), dtype=torch.float32, device=dev)
    acc = None
    for k in range(K):
        g_color, _, g_depth, g_alpha = grads[4 * k: 4 * k + 4]
        if g_color is None and g_depth is None and g_alpha is None:
            d_means2D[k].zero_()
            continue                                             # this view's outputs did not reach the loss
        acc = _backward_view(states[k], inputs, radii_all[k], g_color, g_depth, g_alpha, into=acc, d_means2D_out=d_means2D[k])
    return (acc, d_means2D) if acc is not None else (None, None)


def _saved_views(ctx):
    """(the seven kernel inputs, None for an absent one; the K radii) of a tensor-path node's forward."""
    saved = ctx.saved_tensors                                # raises if an input was modified in place since forward
    it = iter(saved)
    return tuple(next(it) if present else None for present in ctx.inputs_present), saved[len(saved) - len(ctx.states):]


def _caller_grads(ctx, g, d_means2D):
    """A tensor-path node's gradients in forward argument order, in the callers' shapes (ctx.shapes)."""
    means_shape, means2d_shape, sh_shape, opac_shape = ctx.shapes

    def _shape(t, shape):
        return t if (t is None or t.shape == shape) else t.reshape(shape)
    return (_shape(g["means3D"], means_shape), _shape(d_means2D, means2d_shape), _shape(g["shs"], sh_shape),
            g["colors_precomp"], _shape(g["opacities"], opac_shape), g["scales"], g["rotations"], g["cov3D_precomp"])


def _camera_wants_grad(settings_list) -> bool:
    """A camera tensor of one of these settings requires grad (and grad mode is on): the call goes through camera_grad.py's nodes."""
    if not torch.is_grad_enabled():
        return False
    for st in settings_list:
        if getattr(st.viewmatrix, "requires_grad", False) or getattr(st.projmatrix, "requires_grad", False) or \
                getattr(st.campos, "requires_grad", False):
            return True
    return False


class _RasterizeGaussians(torch.autograd.Function):
    @staticmethod
    def forward(ctx, means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, raster_settings):
        _require_cuda(means3D)
        ctx.raster_settings = raster_settings
        ctx.shapes = (means3D.shape, means2D.shape, None if sh is None else sh.shape, opacities.shape)
        # inputs that are not fp32 (converted for the kernels): their gradients are cast back in backward
        odd = tuple(None if (t is None or t.dtype == torch.float32) else t.dtype
                    for t in (means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp))
        ctx.odd_dtypes = odd if any(d is not None for d in odd) else None
        return _views_forward(ctx, (raster_settings,), (means3D, opacities, sh, colors_precomp, scales, rotations, cov3Ds_precomp),
                              any(ctx.needs_input_grad))[0]

    @staticmethod
    def backward(ctx, grad_color, grad_radii, grad_depth, grad_alpha):
        inputs, radii = _saved_views(ctx)
        try:
            g, d_means2D = _views_backward(ctx.states, inputs, radii, (grad_color, grad_radii, grad_depth, grad_alpha), False)
        except Exception:
            if ctx.raster_settings.debug:
                names = ("means3D", "opacities", "shs", "colors_precomp", "scales", "rotations", "cov3D_precomp")
                _debug_dump(DEBUG_SNAPSHOT_BW, "backward", ctx.raster_settings,
                            dict(zip(names, inputs), radii=radii[0], grad_color=grad_color, grad_depth=grad_depth,
                                 grad_alpha=grad_alpha))
            raise
        grads = _caller_grads(ctx, g, d_means2D)
        if ctx.odd_dtypes is not None:
            grads = tuple(t if (t is None or d is None) else t.to(d) for t, d in zip(grads, ctx.odd_dtypes))
        return grads + (None,)


def _none_if_empty(t):
    return None if (t is None or (isinstance(t, torch.Tensor) and t.numel() == 0)) else t


def _exactly_one_of(shs, colors_precomp, scales, rotations, cov3D_precomp):
    """The five optional inputs, None for an absent or empty one — or upstream's error when the combination is not a render."""
    shs, colors_precomp, scales, rotations, cov3D_precomp = map(_none_if_empty, (shs, colors_precomp, scales, rotations, cov3D_precomp))
    if (shs is None) == (colors_precomp is None):
        raise Exception("Please provide excatly one of either SHs or precomputed colors!")
    if ((scales is None or rotations is None) and cov3D_precomp is None) or \
            ((scales is not None or rotations is not None) and cov3D_precomp is not None):
        raise Exception("Please provide exactly one of either scale/rotation pair or precomputed 3D covariance!")
    return shs, colors_precomp, scales, rotations, cov3D_precomp


DEBUG_SNAPSHOT_FW = "snapshot_fw.dump"     # file names of upstream's debug dumps [UPSTREAM-RECALL]
DEBUG_SNAPSHOT_BW = "snapshot_bw.dump"


def _debug_dump(path, what, raster_settings, tensors):
    """`debug=True` (arguments/__init__.py:68 --debug -> gaussian_renderer/__init__.py:50): when a library call fails,
    the arguments of the failing call are saved with torch.save before the error is re-raised — what upstream's extension
    does with its snapshot_fw.dump / snapshot_bw.dump [UPSTREAM-RECALL] — so the failure can be replayed off line."""
    try:
        cpu = {k: (v.detach().cpu() if isinstance(v, torch.Tensor) else v) for k, v in tensors.items()}
        cpu["raster_settings"] = tuple(v.detach().cpu() if isinstance(v, torch.Tensor) else v for v in raster_settings)
        torch.save(cpu, path)
        print(f"\nAn error occured in {what}. Writing {path} for debugging.")
    except Exception as e:                                   # noqa: BLE001 - the original error matters more
        print(f"\nAn error occured in {what}; the debug snapshot could not be written ({e}).")


def rasterize_gaussians(means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp,
                        raster_settings):
    args = (means3D, means2D, _none_if_empty(sh), _none_if_empty(colors_precomp), opacities, _none_if_empty(scales),
            _none_if_empty(rotations), _none_if_empty(cov3Ds_precomp), raster_settings)
    apply = _RasterizeGaussians.apply
    if _camera_wants_grad((raster_settings,)):
        from . import camera_grad                            # (it imports this module)
        apply = camera_grad.apply_gaussians
    if not raster_settings.debug:
        return apply(*args)
    try:
        return apply(*args)
    except Exception:
        _debug_dump(DEBUG_SNAPSHOT_FW, "forward", raster_settings,
                    dict(means3D=means3D, means2D=means2D, sh=args[2], colors_precomp=args[3], opacities=opacities,
                         scales=args[5], rotations=args[6], cov3Ds_precomp=args[7]))
        raise


class GaussianRasterizer(nn.Module):
    """Drop-in for the module constructed at reference gaussian_renderer/__init__.py:53."""

    def __init__(self, raster_settings: GaussianRasterizationSettings):
        super().__init__()
        self.raster_settings = raster_settings

    def markVisible(self, positions: torch.Tensor) -> torch.Tensor:
        """Upstream's frustum-culling helper ([UPSTREAM-RECALL]; not called by the reference): True for points whose
        view-space z exceeds the 0.2 near cut the geometry stage applies (the same single test — DESIGN decision D3)."""
        with torch.no_grad():
            vm = self.raster_settings.viewmatrix.to(positions.device, torch.float32)      # row-vector convention
            z = positions[:, 0] * vm[0, 2] + positions[:, 1] * vm[1, 2] + positions[:, 2] * vm[2, 2] + vm[3, 2]
            return z > 0.2

    def forward(self, means3D, means2D, opacities, shs=None, colors_precomp=None, scales=None, rotations=None,
                cov3D_precomp=None):
        shs, colors_precomp, scales, rotations, cov3D_precomp = _exactly_one_of(shs, colors_precomp, scales, rotations, cov3D_precomp)
        return rasterize_gaussians(means3D, means2D, shs, colors_precomp, opacities, scales, rotations, cov3D_precomp,
                                   self.raster_settings)


# ---------------------------------------------------------------------------------------------------------------------
# K views of the same Gaussians in ONE autograd node (BASELINE cfg5: "multi-view batched step")
# ---------------------------------------------------------------------------------------------------------------------
class _RasterizeViews(torch.autograd.Function):
    """forward: the K views one after the other (each with its own saved state); backward: per view blend backward +
    geometry backward, the second and later views ADDING their parameter gradients to the first one's in the kernel
    (scg_backward `accumulate`), so the node returns the gradient of the SUM over views from one flat arena — no add pass
    per view over 236 bytes per Gaussian, one chain-rule pass through whatever produced the inputs, one gradient
    exchange per K views (parallel.GradBucket.reduce_grads all-reduces that arena in place).
    Outputs, flat: color_0, radii_0, depth_0, alpha_0, color_1, ...; means2D is (K, P, 3): one screen-space gradient slot
    per view (the densification statistics are per view, scene/gaussian_model.py:932-934)."""

    @staticmethod
    def forward(ctx, means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, settings_list):
        _require_cuda(means3D)
        ctx.shapes = (means3D.shape, means2D.shape, None if sh is None else sh.shape, opacities.shape)
        return _views_forward(ctx, settings_list, (means3D, opacities, sh, colors_precomp, scales, rotations, cov3Ds_precomp),
                              any(ctx.needs_input_grad))[0]

    @staticmethod
    def backward(ctx, *grads):
        acc, d_means2D = _views_backward(ctx.states, *_saved_views(ctx), grads, True)
        return (None,) * 9 if acc is None else _caller_grads(ctx, acc, d_means2D) + (None,)


class GaussianRasterizerViews(nn.Module):
    """K views of one set of Gaussians per call — the batched multi-view step of BASELINE cfg5; no counterpart in the
    reference, whose train.py:143 renders one view per iteration.  Same keyword arguments as GaussianRasterizer, except
    that `means2D` is (K, P, 3) (a screen-space gradient slot per view); returns a list of K
    (color, radii, depth, alpha) tuples.  The loss may use any subset of the views."""

    def __init__(self, raster_settings_list):
        super().__init__()
        self.raster_settings_list = list(raster_settings_list)

    def forward(self, means3D, means2D, opacities, shs=None, colors_precomp=None, scales=None, rotations=None,
                cov3D_precomp=None):
        shs, colors_precomp, scales, rotations, cov3D_precomp = _exactly_one_of(shs, colors_precomp, scales, rotations, cov3D_precomp)
        K = len(self.raster_settings_list)
        if means2D.dim() != 3 or means2D.shape[0] != K:
            raise ValueError(f"means2D must be ({K}, P, 3): one screen-space gradient slot per view")
        apply = _RasterizeViews.apply
        if _camera_wants_grad(self.raster_settings_list):
            from . import camera_grad                        # (it imports this module)
            apply = camera_grad.apply_views
        flat = apply(means3D, means2D, shs, colors_precomp, opacities, scales, rotations, cov3D_precomp, self.raster_settings_list)
        return [tuple(flat[4 * k: 4 * k + 4]) for k in range(K)]

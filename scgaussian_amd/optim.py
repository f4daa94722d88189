"""The training loop's gradient consumers on the GPU: the optimizer step and the densification statistics.

The reference steps two torch.optim.Adam per iteration (train.py:203-208; twelve parameter groups, scene/gaussian_model.py:486-515)
and accumulates the densification statistics with four indexed torch ops (train.py:191-192, gaussian_model.py:932-934).  At its
scene size those consume more host time than the whole captured render + loss + backward.  Here each is ONE launch:

    from scgaussian_amd import optim
    optim.install(gaussians)                       # after gaussians.training_setup(opt): both optimizers become ArenaAdam
    ...
    optim.densification_stats(gaussians.max_radii2D, gaussians.xyz_gradient_accum, gaussians.denom,
                              viewspace_point_tensor.grad, radii)

ArenaAdam IS a torch.optim.Adam (same param_groups with their names, same state keys step / exp_avg / exp_avg_sq, state_dict
interchangeable with torch's), so the reference's state surgery (update_learning_rate, replace_tensor_to_optimizer,
_prune_optimizer, cat_tensors_to_optimizer) works on it unchanged.  What the kernel does not take (CPU or non-fp32 tensors, sparse
gradients, amsgrad, weight decay, maximize, differentiable, tensor learning rates, more than 16 parameters per device) goes to
torch's own step.
"""
from __future__ import annotations

from typing import Dict, List, Optional

import torch

from . import _lib

MAX_SEGMENTS = _lib.ADAM_MAX_SEGMENTS
_LR_RING = 4                                   # pinned staging slots of sync_hyperparameters()


def _row_len(p: torch.Tensor) -> int:
    """Row length of the SH-tail skip: the SH rest block (P, 15, 3) -> 45; 0 for every other tensor."""
    return p[0].numel() if (p.dim() == 3 and p.shape[1] > 1 and p.shape[0] > 0) else 0


def _moment_record(p, st):
    m, v = st["exp_avg"], st["exp_avg_sq"]
    return (id(p), id(m), m.data_ptr(), m._version, id(v), v.data_ptr(), v._version)


class SlotPolicy:
    """When a row segment's watermark can be trusted (host-only bookkeeping, one per device).

    After every launch the moments of each slot are recorded (object, data_ptr, _version of exp_avg and exp_avg_sq, and the
    parameter).  A slot whose record differs at the next step — the moments were replaced (densification, load_state_dict), edited
    in place by torch, or the slot now holds another parameter — is launched with SCG_ADAM_FORCE_FULL, which re-derives its
    watermark from scratch."""

    def __init__(self):
        self.records: List[Optional[tuple]] = [None] * MAX_SEGMENTS

    def force_flags(self, slots) -> List[bool]:
        """slots: [(param, state, row_len)] in launch order."""
        return [rl > 0 and self.records[i] != _moment_record(p, st) for i, (p, st, rl) in enumerate(slots)]

    def record(self, slots) -> None:
        for i, (p, st, rl) in enumerate(slots):
            self.records[i] = _moment_record(p, st) if rl > 0 else None
        for i in range(len(slots), MAX_SEGMENTS):
            self.records[i] = None

    def invalidate(self) -> None:
        self.records = [None] * MAX_SEGMENTS


class _Device:
    """Per-device launch state of one ArenaAdam: workspace (ticket + watermarks), cached segment tables, the learning-rate table a
    captured step reads, and its pinned staging ring."""

    def __init__(self, device: torch.device):
        self.device = device
        nbytes = _lib.load().scg_adam_workspace_bytes(MAX_SEGMENTS)
        self.ws = torch.zeros(nbytes // 4, dtype=torch.int32, device=device)          # zeroed once, kept
        self.lr_table = torch.zeros(MAX_SEGMENTS, dtype=torch.float64, device=device)
        self.policy = SlotPolicy()
        self.tables: Dict[tuple, tuple] = {}                                           # key -> (ctypes array, slots)
        self.synced = None                                                             # (slot -> group index, lrs) last synced
        self.ring = None                                                               # [(pinned tensor, event or None)]
        self.ring_next = 0
        self.last_slots = []                                                           # slots of the latest launch


class ArenaAdam(torch.optim.Adam):
    """torch.optim.Adam whose step is one scg_adam_step launch per device (no host synchronisation, capturable in a graph).

    The arithmetic is torch's single-tensor Adam in torch's order; step counters live on the device (as torch's capturable Adam
    keeps them).  Inside a stream capture the learning rates are read at replay time from a device table: call
    `sync_hyperparameters()` eagerly before capturing and after every change of a group's lr between replays."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, *, foreach=None,
                 maximize=False, capturable=False, differentiable=False, fused=None, **kw):
        # capturable=True: load_state_dict / torch's own lazy state creation keep `step` on the device
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, foreach=foreach,
                         maximize=maximize, capturable=True, differentiable=differentiable, fused=fused, **kw)
        self._dev: Dict[int, _Device] = {}
        self.fallback_steps = 0                     # steps that went to torch's implementation (visible to tests)

    # ---- construction helpers --------------------------------------------------------------------------------------------
    @classmethod
    def from_optimizer(cls, opt: torch.optim.Adam) -> "ArenaAdam":
        """The same groups (names, lrs, options) and the same state tensors (moved, not copied; CPU step counters go to the
        parameter's device)."""
        d = dict(opt.defaults)
        d.pop("capturable", None)
        d.pop("params", None)
        groups = []
        for g in opt.param_groups:
            ng = {k: v for k, v in g.items() if k != "capturable"}
            ng["params"] = list(g["params"])
            groups.append(ng)
        new = cls(groups, **d)
        for p, st in opt.state.items():
            st = dict(st)
            if "step" in st and torch.is_tensor(st["step"]) and p.is_cuda:
                st["step"] = st["step"].to(device=p.device, dtype=torch.float32)
            new.state[p] = st
        return new

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        for g in self.param_groups:                 # a torch checkpoint's groups say capturable=False: ours stay capturable
            g["capturable"] = True
        for p, st in self.state.items():
            s = st.get("step")
            if torch.is_tensor(s) and p.is_cuda and (s.device != p.device or s.dtype != torch.float32):
                st["step"] = s.to(device=p.device, dtype=torch.float32)
        for d in self._dev.values():
            d.policy.invalidate()
            d.tables.clear()

    def __setstate__(self, state):
        super().__setstate__(state)
        self.__dict__.setdefault("_dev", {})
        self.__dict__.setdefault("fallback_steps", 0)

    # ---- what the kernel takes -------------------------------------------------------------------------------------------
    @staticmethod
    def _group_supported(g) -> bool:
        return (not g["amsgrad"] and g["weight_decay"] == 0 and not g["maximize"] and not g["differentiable"]
                and not torch.is_tensor(g["lr"]) and not any(torch.is_tensor(b) for b in g["betas"]))

    def _collect(self):
        """{device index: [(group index, param, grad, state)]} of the params that have a gradient, or None when anything must
        go to torch's step."""
        per: Dict[int, list] = {}
        for gi, g in enumerate(self.param_groups):
            ok = self._group_supported(g)
            for p in g["params"]:
                gr = p.grad
                if gr is None:
                    continue
                if not ok or not p.is_cuda or p.dtype != torch.float32 or gr.dtype != torch.float32 or gr.is_sparse \
                        or gr.device != p.device or gr.shape != p.shape or not p.is_contiguous() or not gr.is_contiguous():
                    return None
                st = self.state.get(p)
                if st:
                    m, v, s = st.get("exp_avg"), st.get("exp_avg_sq"), st.get("step")
                    if m is None or v is None or s is None or not torch.is_tensor(s) or s.device != p.device \
                            or s.dtype != torch.float32 or m.dtype != torch.float32 or v.dtype != torch.float32 \
                            or not m.is_contiguous() or not v.is_contiguous() or m.shape != p.shape or v.shape != p.shape:
                        return None
                per.setdefault(p.device.index, []).append((gi, p, gr, st))
        if any(len(v) > MAX_SEGMENTS for v in per.values()):
            return None
        return per

    # ---- step ------------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        per = self._collect()
        if per is None:
            self._fallback()
            return loss
        capturing = torch.cuda.is_current_stream_capturing()
        for idx, items in per.items():
            self._launch(idx, items, capturing)
        return loss

    def _fallback(self):
        self.fallback_steps += 1
        saved = [g["capturable"] for g in self.param_groups]
        for g in self.param_groups:                 # torch's capturable path takes device tensors only
            g["capturable"] = all(p.is_cuda for p in g["params"])
        try:
            super().step()
        finally:
            for g, c in zip(self.param_groups, saved):
                g["capturable"] = c
        for d in self._dev.values():                # torch moved the moments: no watermark can be trusted
            d.policy.invalidate()

    def _device(self, idx: int) -> _Device:
        d = self._dev.get(idx)
        if d is None:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("ArenaAdam: step once eagerly (or call sync_hyperparameters()) before capturing its step")
            d = self._dev[idx] = _Device(torch.device("cuda", idx))
        return d

    def _state_for(self, p, capturing: bool):
        st = self.state[p]
        if not st:
            if capturing:
                raise RuntimeError("ArenaAdam: the optimizer state must exist before a capture (step once eagerly)")
            st["step"] = torch.zeros((), dtype=torch.float32, device=p.device)
            st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        return st

    def _table(self, d: _Device, items, capturing: bool):
        """The cached ctypes segment table of this set of tensors (revalidated by identity + data_ptr of param, grad and both
        moments) and its slots [(param, state, row_len)]."""
        sts = [self._state_for(p, capturing) for (_gi, p, _gr, _st) in items]
        key = tuple((gi, id(p), p.data_ptr(), id(gr), gr.data_ptr(), id(st["exp_avg"]), st["exp_avg"].data_ptr(),
                     id(st["exp_avg_sq"]), st["exp_avg_sq"].data_ptr(), st["step"].data_ptr())
                    for (gi, p, gr, _), st in zip(items, sts))
        ent = d.tables.get(key)
        if ent is None:
            arr = (_lib.ScgAdamSegment * len(items))()
            slots = []
            for k, ((gi, p, gr, _), st) in enumerate(zip(items, sts)):
                s = arr[k]
                s.param, s.grad = p.data_ptr(), gr.data_ptr()
                s.exp_avg, s.exp_avg_sq, s.step = st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(), st["step"].data_ptr()
                s.numel = p.numel()
                s.row_len = _row_len(p)
                slots.append((p, st, s.row_len))
            if len(d.tables) >= 16:                 # one table per captured view is typical; keep the cache small
                d.tables.pop(next(iter(d.tables)))
            ent = d.tables[key] = (arr, slots, [gi for (gi, _p, _g, _s) in items])
        return ent

    def _launch(self, idx: int, items, capturing: bool):
        d = self._device(idx)
        arr, slots, gis = self._table(d, items, capturing)
        groups = self.param_groups
        force = d.policy.force_flags(slots)
        for k, gi in enumerate(gis):
            g = groups[gi]
            s = arr[k]
            b1, b2 = g["betas"]
            s.lr, s.beta1, s.beta2, s.eps = g["lr"], b1, b2, g["eps"]
            s.flags = _lib.ADAM_FORCE_FULL if force[k] else 0
        lr_table = None
        if capturing:
            lrs = [float(groups[gi]["lr"]) for gi in gis]
            if d.synced != (tuple(gis), tuple(lrs)):
                raise RuntimeError("ArenaAdam: call sync_hyperparameters() before capturing (the captured step reads its "
                                   "learning rates from a device table) and capture with the gradients of all parameters")
            lr_table = d.lr_table.data_ptr()
        lib = _lib.load()
        stream = torch.cuda.current_stream(d.device).cuda_stream
        _lib.check(lib.scg_adam_step(arr, len(slots), lr_table, d.ws.data_ptr(), d.ws.numel() * 4, stream), "scg_adam_step")
        d.policy.record(slots)
        d.last_slots = slots

    # ---- captured steps --------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def sync_hyperparameters(self) -> None:
        """Refresh the device table of learning rates that a captured step() reads from param_groups (eagerly: between replays,
        and before the capture).  The table follows the order of the parameters in param_groups: a captured step must have the
        gradients of all of them.  The copy is enqueued on the current stream; the pinned staging slot it reads is not rewritten
        before that copy has run."""
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("ArenaAdam.sync_hyperparameters() runs eagerly, not inside a capture")
        per: Dict[int, list] = {}                   # the layout of a step in which every parameter has a gradient
        for gi, g in enumerate(self.param_groups):
            for p in g["params"]:
                if p.is_cuda:
                    per.setdefault(p.device.index, []).append(gi)
        for idx, gis in per.items():
            if len(gis) > MAX_SEGMENTS:             # torch's step takes those
                continue
            d = self._device(idx)
            lrs = [float(self.param_groups[gi]["lr"]) for gi in gis]
            if d.ring is None:
                d.ring = [[torch.zeros(MAX_SEGMENTS, dtype=torch.float64).pin_memory(), None] for _ in range(_LR_RING)]
            slot = d.ring[d.ring_next]
            d.ring_next = (d.ring_next + 1) % _LR_RING
            if slot[1] is not None:
                slot[1].synchronize()               # the copy that last read this staging slot has run
            slot[0][: len(lrs)] = torch.tensor(lrs, dtype=torch.float64)
            d.lr_table.copy_(slot[0], non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(torch.cuda.current_stream(d.device))
            slot[1] = ev
            d.synced = (tuple(gis), tuple(lrs))

    def tensors_replaced(self) -> None:
        """The caller replaced parameters or moments wholesale (densify.densify_and_prune): drop the cached segment tables, which
        would keep the old tensors alive, and trust no watermark at the next step."""
        for d in self._dev.values():
            d.policy.invalidate()
            d.tables.clear()
            d.last_slots = []

    # ---- test access -----------------------------------------------------------------------------------------------------
    def live_columns(self) -> Dict[torch.Tensor, int]:
        """{row-segment parameter: its watermark after the latest step} (reads the device: tests and diagnostics only)."""
        out = {}
        for d in self._dev.values():
            words = d.ws.cpu()
            for k, (p, _st, rl) in enumerate(d.last_slots):
                if rl > 0:
                    out[p] = int(words[32 + k])
        return out


def install(gaussians) -> None:
    """Replace `gaussians.optimizer` (and `gaussians.optimizer_bg` when the model has one) by ArenaAdam, keeping groups and
    state: the two lines a reference training script adds after `gaussians.training_setup(opt)` are
    `from scgaussian_amd import optim; optim.install(gaussians)`."""
    for name in ("optimizer", "optimizer_bg"):
        opt = getattr(gaussians, name, None)
        if opt is not None and not isinstance(opt, ArenaAdam):
            setattr(gaussians, name, ArenaAdam.from_optimizer(opt))


def densification_stats(max_radii2D: torch.Tensor, xyz_gradient_accum: torch.Tensor, denom: torch.Tensor,
                        means2D_grad: torch.Tensor, radii: torch.Tensor) -> None:
    """In place, one launch, for the Gaussians with radii > 0 (render()'s visibility_filter):
    max_radii2D = max(max_radii2D, radii); xyz_gradient_accum += |means2D_grad[:, :2]|; denom += 1
    (reference train.py:191-192 and gaussian_model.py:932-934).  The results are the tensors the reference keeps, so
    parallel.reduce_densification_stats exchanges them as before."""
    P = radii.numel()
    for name, t in (("max_radii2D", max_radii2D), ("xyz_gradient_accum", xyz_gradient_accum), ("denom", denom)):
        if not t.is_cuda or t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != P:
            raise _lib.ScgError(f"densification_stats: {name} must be a contiguous fp32 CUDA tensor of {P} elements")
    if not radii.is_cuda or radii.dtype != torch.int32 or not radii.is_contiguous():
        raise _lib.ScgError("densification_stats: radii must be a contiguous int32 CUDA tensor")
    g = means2D_grad
    if not g.is_cuda or g.dtype != torch.float32 or g.dim() != 2 or g.shape[0] != P or g.shape[1] < 2 or g.stride(1) != 1:
        raise _lib.ScgError("densification_stats: means2D_grad must be an fp32 CUDA tensor (P, >= 2) with unit column stride")
    dev = radii.device
    if any(t.device != dev for t in (max_radii2D, xyz_gradient_accum, denom, g)):
        raise _lib.ScgError("densification_stats: all tensors must be on one device")
    if P == 0:
        return
    stream = torch.cuda.current_stream(dev).cuda_stream
    _lib.check(_lib.load().scg_densify_stats(P, radii.data_ptr(), g.data_ptr(), g.stride(0), xyz_gradient_accum.data_ptr(),
                                             denom.data_ptr(), max_radii2D.data_ptr(), stream), "scg_densify_stats")

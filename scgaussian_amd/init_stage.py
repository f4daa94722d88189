"""The reference's ray-depth init stage (train.py:49-95) on the GPU: all match pairs, any number of Adam steps per launch.

The reference runs 2 000 Adam iterations on the per-match ray depths `z_val` against GaussianModel.get_matchloss_from_base
(scene/gaussian_model.py:175-239), keeps per match the depth of its smallest loss term, and `create_from_pcd` then keeps the
matches whose smallest term is below 0.1.  Here the whole stage is four launches (one per learning-rate segment):

    from scgaussian_amd.init_stage import InitStage
    from scgaussian_amd import seed
    stage = InitStage.from_view_gs(gaussians.view_gs)          # instead of gaussians.training_setup_init()
    seed.install(gaussians, stage)                             # gaussians.create_from_pcd now runs in csrc/seed.hip (seed.py)
    stage.run_schedule(2000, halve_at=(500, 1000, 1500))       # instead of the loop of train.py:57-93
    stage.load_best(gaussians.view_gs)                         # instead of gaussians.load_z_val(best_state_dict)
    gaussians.create_from_pcd(stage.min_loss_state())          # train.py:102 unchanged: the stage's arena is read in place

A caller who keeps the reference's loop and its torch Adam replaces the body of get_matchloss_from_base by
`match_loss_from_base(view_gs, stage)`: one launch forward, none backward.

There is no CPU path: launching on CPU tensors raises ScgError.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _arena, _lib
from ._lib import check, ptr

BETAS = (0.9, 0.999)                            # training_setup_init: torch.optim.Adam(l_init, lr=0.0, eps=1e-15)
EPS = 1e-15
MAX_STEPS = _lib.INIT_STAGE_MAX_STEPS
_SEG_DTYPE = np.dtype(_lib.ScgInitSegment)      # the device table's record: the ctypes struct's fields, offsets and size
_GROUP = 64                                     # elements per workgroup (one wave): the row length of the partial sums is ceil(N / 64)


def _current_stream(t: torch.Tensor) -> int:
    return _lib.stream_of(t, "the init stage")


class InitStage:
    """The arena of all ordered view pairs (a -> b) of a reference `view_gs` dictionary and the state of its optimisation.

    segments: [(key_a, key_b, offset, M)] in arena order.  z, exp_avg, exp_avg_sq, best_z, min_loss: flat fp32 (N)."""

    def __init__(self, segments, table, rays_o, rays_d, uv_t, wgt, z, empty, lr, loss_scale, record_losses=True):
        self.segments: List[Tuple[object, object, int, int]] = segments
        self.table = table                       # uint8 device tensor holding the ScgInitSegment records
        self.rays_o, self.rays_d, self.uv_t, self.wgt, self.z = rays_o, rays_d, uv_t, wgt, z
        self.exp_avg, self.exp_avg_sq = torch.zeros_like(z), torch.zeros_like(z)
        self.best_z, self.min_loss = torch.zeros_like(z), torch.zeros_like(z)
        self.empty_pairs: List[Tuple[object, object]] = empty        # ordered pairs without a valid match: their loss is NaN
        self.lr, self.loss_scale = float(lr), float(loss_scale)
        self.record_losses = record_losses
        self.iteration = 0                       # iterations run so far = the global index of the next one
        self._partials: List[torch.Tensor] = []  # one (n, W) tensor per launch

    # ---- packing ---------------------------------------------------------------------------------------------------------
    @classmethod
    def from_view_gs(cls, view_gs: Dict, lr: float = 0.5, loss_scale: float = 5.0, record_losses: bool = True) -> "InitStage":
        keys, pairs = _arena.walk(view_gs)
        segments, recs, empty = [], [], []
        rays_o, rays_d, uv_t, wgt, z = [], [], [], [], []
        for a, b, off, M, info in pairs:
            back = view_gs[b]["match_infos"][a]
            zv = info["z_val"].detach()
            if back["uv"].shape[0] != M or zv.shape[0] != M:
                raise _lib.ScgError(f"init stage: pair ({a}, {b}) has {zv.shape[0]} depths but {back['uv'].shape[0]} partner matches")
            valid = ((info["blender_mask"].detach().float() * back["blender_mask"].detach().float()) > 0).float()
            count = float(valid.sum())
            if count == 0:
                empty.append((a, b))
            first = a if keys.index(a) < keys.index(b) else b      # the reference normalises by the earlier view's size
            rec = np.zeros((), dtype=_SEG_DTYPE)
            rec["offset"], rec["count"] = off, M
            rec["width"], rec["height"] = float(view_gs[first]["width"]), float(view_gs[first]["height"])
            rec["intr"] = view_gs[b]["intr"].detach().float().cpu().numpy().reshape(9)
            rec["w2c"] = view_gs[b]["w2c"].detach().float().cpu().numpy()[:3].reshape(12)
            recs.append(rec)
            segments.append((a, b, off, M))
            rays_o.append(info["rays_o"].detach().float().reshape(M, 3))
            rays_d.append(info["rays_d"].detach().float().reshape(M, 3))
            uv_t.append(back["uv"].detach().float().reshape(M, 2))
            wgt.append(valid / count if count > 0 else valid)
            z.append(zv.float().reshape(M))
        if not segments:
            raise _lib.ScgError("init stage: view_gs holds no match pair")
        dev = pairs[0][4]["z_val"].device
        table = _arena.upload_table(np.stack(recs), dev)
        cat = lambda ts: torch.cat([t.to(dev) for t in ts]).contiguous()           # noqa: E731
        return cls(segments, table, cat(rays_o), cat(rays_d), cat(uv_t), cat(wgt), cat(z), empty, lr, loss_scale, record_losses)

    @classmethod
    def from_mono(cls, setup, lr: float = 0.5, loss_scale: float = 5.0, record_losses: bool = True) -> "InitStage":
        """The stage over the arena of a mono.MonoSetup, read in place: rays_o, rays_d, uv_t, wgt and z are the setup's own
        tensors (z is what its view_gs holds as z_val), the segment records were formed from the host constants and uploaded with
        the setup's inputs.  One host read: the pairs' counts, for empty_pairs."""
        return cls(list(setup.segments), setup.init_table, setup.rays_o, setup.rays_d, setup.uv_t, setup.wgt, setup.z,
                   setup.empty_pairs(), lr, loss_scale, record_losses)

    @property
    def N(self) -> int:
        return self.z.numel()

    def z_views(self) -> Dict:
        """{a: {b: (M,1) view into the flat z}}."""
        return _arena.nested(self.segments, self.z, True)

    def install(self, view_gs: Dict) -> None:
        """Put the (M,1) views of the flat z back into view_gs as nn.Parameters (they share the arena's memory), so the
        reference's create_from_pcd and get_z_val read the stage's depths unchanged."""
        for a, b, off, M in self.segments:
            view_gs[a]["match_infos"][b]["z_val"] = torch.nn.Parameter(self.z[off:off + M].view(M, 1), requires_grad=True)

    # ---- launches --------------------------------------------------------------------------------------------------------
    def _launch(self, z, first_iter, n_steps, lr, loss_scale, loss_state, grad, partials):
        lib = _lib.load()
        stream = _current_stream(z)
        state = (self.exp_avg, self.exp_avg_sq, self.best_z, self.min_loss) if n_steps > 0 else (None,) * 4
        check(lib.scg_init_stage_run(ptr(self.table), len(self.segments), self.N, ptr(self.rays_o), ptr(self.rays_d),
                                     ptr(self.uv_t), ptr(self.wgt), ptr(z), *(ptr(t) for t in state), first_iter, n_steps,
                                     float(lr), BETAS[0], BETAS[1], EPS, float(loss_scale), ptr(loss_state), ptr(grad),
                                     ptr(partials), 0 if partials is None else partials.numel() * 4, stream),
              "scg_init_stage_run")

    def run(self, n: int) -> None:
        """n iterations at the current learning rate: one launch (one per 4 096 iterations)."""
        if n < 0:
            raise ValueError("n must be >= 0")
        while n > 0:
            k = min(n, MAX_STEPS)
            partials = None
            if self.record_losses:
                partials = torch.empty((k, (self.N + _GROUP - 1) // _GROUP), dtype=torch.float32, device=self.z.device)
            self._launch(self.z, self.iteration, k, self.lr, self.loss_scale, None, None, partials)
            if partials is not None:
                self._partials.append(partials)
            self.iteration += k
            n -= k

    def run_schedule(self, total: int = 2000, halve_at: Sequence[int] = (500, 1000, 1500)) -> None:
        """`total` iterations; the learning rate is halved BEFORE the iteration whose global index is in halve_at
        (train.py:59-60).  One launch per learning-rate segment."""
        pos, end = self.iteration, self.iteration + total
        for h in sorted(set(int(h) for h in halve_at)):
            if not pos <= h < end:
                continue
            if h > pos:
                self.run(h - pos)
            self.lr *= 0.5
            pos = h
        if end > pos:
            self.run(end - pos)

    def evaluate(self, z: Optional[torch.Tensor] = None, loss_scale: Optional[float] = None):
        """(loss_state (N), gradient of loss_scale * matchloss w.r.t. z (N), partial sums (W)) at `z` (default: the stage's own
        depths).  Changes no state."""
        z = self.z if z is None else z
        if z.shape != self.z.shape or z.dtype != torch.float32 or not z.is_contiguous() or z.device != self.z.device:
            raise _lib.ScgError("init stage: z must be a contiguous fp32 tensor of the arena's shape on its device")
        loss_state, grad = torch.empty_like(self.z), torch.empty_like(self.z)
        partials = torch.empty(((self.N + _GROUP - 1) // _GROUP,), dtype=torch.float32, device=self.z.device)
        self._launch(z, 0, 0, 0.0, self.loss_scale if loss_scale is None else loss_scale, loss_state, grad, partials)
        return loss_state, grad, partials

    # ---- results ---------------------------------------------------------------------------------------------------------
    def partials(self) -> torch.Tensor:
        """(iterations, W) on the CPU: row k, summed, is the match loss of iteration k over the pairs that have a valid match."""
        W = (self.N + _GROUP - 1) // _GROUP
        if not self._partials:
            return torch.zeros((0, W), dtype=torch.float32)
        return torch.cat([p.cpu() for p in self._partials])

    def losses(self) -> torch.Tensor:
        """One scalar per iteration run so far, equal to loss_scale * matchloss (the reference's `loss`): the workgroups' partial
        sums added in workgroup order.  NaN when a pair has no valid match, as the mean over nothing is."""
        if not self.record_losses:
            raise _lib.ScgError("init stage: losses were not recorded (record_losses=False)")
        total = torch.zeros(self.partials().shape[0], dtype=torch.float64)
        for col in self.partials().double().unbind(1):               # a fixed order
            total = total + col
        out = (total.float() * self.loss_scale)
        if self.empty_pairs:
            out = out + float("nan")
        return out

    def best_state_dict(self) -> Dict:
        """{a: {b: (M,1)}}: per match the depth at which its loss term was smallest (the reference's best_state_dict)."""
        return _arena.nested(self.segments, self.best_z, True)

    def min_loss_state(self) -> Dict:
        """{a: {b: (M)}}: that smallest term (the reference's min_loss_state, what create_from_pcd thresholds at 0.1)."""
        return _arena.nested(self.segments, self.min_loss, False)

    def load_best(self, view_gs: Optional[Dict] = None) -> None:
        """What load_z_val(best_state_dict) does: the depths become the best ones (and, given view_gs, are installed)."""
        self.z.copy_(self.best_z)
        if view_gs is not None:
            self.install(view_gs)


class _MatchLossFromBase(torch.autograd.Function):
    @staticmethod
    def forward(ctx, stage: InitStage, *zs):
        flat = [z.detach().float().reshape(-1) for z in zs]
        z = stage.z if _is_arena(stage, zs) else torch.cat(flat).contiguous()
        loss_state, grad, partials = stage.evaluate(z, loss_scale=1.0)
        ctx.grad = grad
        ctx.meta = [(t.shape, t.dtype) for t in zs]
        loss = partials.sum()
        if stage.empty_pairs:
            loss = loss + float("nan")
        ctx.mark_non_differentiable(loss_state)
        return loss, loss_state

    @staticmethod
    def backward(ctx, g, _g_state):
        out, off = [], 0
        for shape, dtype in ctx.meta:
            n = int(np.prod(shape))
            out.append((ctx.grad[off:off + n] * g).reshape(shape).to(dtype))
            off += n
        return (None, *out)


def _is_arena(stage: InitStage, zs) -> bool:
    return _arena.is_arena(stage.z, zs, stage.segments)


def match_loss_from_base(view_gs: Dict, stage: Optional[InitStage] = None):
    """Drop-in for the body of GaussianModel.get_matchloss_from_base: returns (match_loss, loss_state) with loss_state in the
    reference's nested {key: {key1: (M)}} shape; match_loss is differentiable w.r.t. the z_val tensors of view_gs.  `stage`: the
    packed arena of this view_gs (InitStage.from_view_gs), built here when absent — pass it when calling in a loop."""
    if stage is None:
        stage = InitStage.from_view_gs(view_gs, record_losses=False)
    zs = [view_gs[a]["match_infos"][b]["z_val"] for a, b, _off, _M in stage.segments]
    for z, (a, b, _off, M) in zip(zs, stage.segments):
        if z.numel() != M:
            raise _lib.ScgError(f"init stage: z_val of pair ({a}, {b}) has {z.numel()} elements, the packed arena {M}")
    loss, flat = _MatchLossFromBase.apply(stage, *zs)
    return loss, _arena.nested(stage.segments, flat, False)

"""The ScgFrame a library call is handed, and what a camera's previous render left for its next one.

A _Frame is the ctypes struct plus the tensors it points at, cached by content (_frame_for).  A _CamHints record, per (camera, image
size, device), holds the launch-order hints (per-tile costs, the blend backward's per-quadrant times, the pinned long-list words): a
hint never changes a result, only which kernels are launched and in which order tiles start.  The module switches live in
rasterizer.py, which reads them per forward and passes in the three that matter here (`switches`: cost buffers exist, bwd_cost_in is
handed over, long words are wanted).
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch

from ._cameras import _camera_key
from ._lib import TILE, ScgFrame, ptr


def _stream(device) -> int:
    """Raw hipStream_t of torch's current stream on `device` (the C call behind torch.cuda.current_stream)."""
    return torch._C._cuda_getCurrentRawStream(device.index if device.index is not None else torch.cuda.current_device())


def _f32c(t: Optional[torch.Tensor], device) -> Optional[torch.Tensor]:
    if t is None or t.numel() == 0:
        return None
    if t.dtype == torch.float32 and t.device == device and t.is_contiguous():     # the usual case: nothing to do
        return t
    if t.device != device:
        if not t.is_cuda and device.type == "cuda" and t.numel() <= 64:
            # a camera's matrices / background handed over in host memory (a caller that builds a camera per frame): through a
            # pinned block and an asynchronous copy — a pageable-memory upload would wait for everything queued on the stream
            return t.detach().to(torch.float32).contiguous().pin_memory().to(device, non_blocking=True)
        t = t.to(device)
    if t.dtype != torch.float32:
        t = t.float()
    return t.contiguous()


class _Frame:
    """ScgFrame plus the tensors whose storage it points at (kept alive for the call)."""

    def __init__(self, settings, P: int, M: int, device):
        self.keep = [_f32c(settings.viewmatrix, device), _f32c(settings.projmatrix, device),
                     _f32c(settings.campos, device), _f32c(settings.bg, device)]
        if any(k is None for k in self.keep[:3]):
            raise ValueError("viewmatrix / projmatrix / campos must be non-empty tensors")
        self.vm_src = settings.viewmatrix        # the caller's tensor: what names the camera (host content / tag_camera / content)
        self.c = ScgFrame(P=int(P), sh_degree=int(settings.sh_degree), sh_coeffs=int(M),
                          width=int(settings.image_width), height=int(settings.image_height),
                          tanfovx=float(settings.tanfovx), tanfovy=float(settings.tanfovy),
                          scale_modifier=float(settings.scale_modifier),
                          prefiltered=int(bool(settings.prefiltered)), debug=int(bool(settings.debug)),
                          viewmatrix=ptr(self.keep[0]), projmatrix=ptr(self.keep[1]), campos=ptr(self.keep[2]),
                          bg=ptr(self.keep[3]))
        self.H, self.W = int(settings.image_height), int(settings.image_width)
        self.n_tiles = ((self.W + TILE - 1) // TILE) * ((self.H + TILE - 1) // TILE)
        # what the previous render of this CAMERA left for the next one (launch-order hint, long-list counts): shared by every
        # frame of the camera — a frame is (camera, background, ...): a training loop with random backgrounds
        # (reference train.py:141) builds a new frame per iteration, its hints must not start from nothing each time
        self.hints = None
        self.cam_key = None              # identity of the camera (content of its view matrix, _camera_key): set at the first forward
        self.ref = C.byref(self.c)

    @property
    def long_np(self):
        """The camera's two ScgFrame.long_lists_out words as a numpy view (None before the first forward / when switched off)."""
        return None if self.hints is None else self.hints.long_np

    def next_forward(self, device, cam_key, switches):
        """Called once per forward: what the previous render of this camera recorded becomes the hint, the other buffer
        receives this render's costs.  `cam_key`: the camera's key when the caller holds it already (None: looked up here)."""
        # (the camera's record moves to the recently-used end of its table, and one that was evicted meanwhile — its pinned words
        # belong to another camera now — is replaced)
        self.cam_key = cam = cam_key if cam_key is not None else _camera_key(self.vm_src)
        h = self.hints = _hints_for(cam, self.W, self.H, device, self.n_tiles, switches[0], switches[2])
        if h.cost is not None:
            cur = _stream(device)
            if cur not in h.streams:
                h.streams.add(cur)
                ts = torch.cuda.current_stream(device)
                for t in (*h.cost, *h.bcost):
                    t.record_stream(ts)
        self.c.long_lists_out = h.long_ptr
        if h.cost is not None:
            self.c.tile_cost_in = h.cost[h.cur].data_ptr() if h.cost_valid else None
            h.cur ^= 1
            self.c.tile_cost_out = h.cost[h.cur].data_ptr()
            h.cost_valid = True
            # the blend backward's own order (ScgFrame.bwd_cost_in / _out, per quadrant): the buffer the camera's latest
            # BACKWARD wrote becomes the hint; it is swapped only when a backward ran since (renders in between keep it)
            if h.bwritten:
                h.bcur ^= 1
                h.bwritten, h.bvalid = False, True
            self.c.bwd_cost_in = h.bcost[h.bcur ^ 1].data_ptr() if (h.bvalid and switches[1]) else None
            self.c.bwd_cost_out = h.bcost[h.bcur].data_ptr()
        else:                            # (a cached frame whose camera's record was made with TILE_COST_HINT off)
            self.c.tile_cost_in = self.c.tile_cost_out = self.c.bwd_cost_in = self.c.bwd_cost_out = None


class _CamHints:
    """Per (camera, image size, device): two buffers of per-tile costs swapped at every forward (ScgFrame.tile_cost_in /
    _out) and the two pinned words of ScgFrame.long_lists_out (ABI 8: the number of tiles whose list is longer than the
    forward blend sorts itself / longer than 16 384 entries; -1: no render has completed yet).  Not per Gaussian count: the
    buffers are per TILE, and a record that died at every densification would leave the camera without history each time."""
    __slots__ = ("cost", "cur", "cost_valid", "long_np", "long_ptr", "slot", "bcost", "bcur", "bwritten", "bvalid", "streams")


_CAM_HINTS = {}                                  # (camera content, W, H, device) -> _CamHints, least recently used first
_CAM_HINTS_MAX = 1024


def _hints_for(cam_key, W, H, device, n_tiles, cost=True, long_words=True):
    key = (cam_key, W, H, device.index)
    h = _CAM_HINTS.pop(key, None)
    if h is None:
        if len(_CAM_HINTS) >= _CAM_HINTS_MAX:                    # the least recently used quarter goes; their pinned words are
            for k in list(_CAM_HINTS)[: _CAM_HINTS_MAX // 4]:    # handed out again (a render of theirs finished long ago: the
                _release_long_words(_CAM_HINTS.pop(k))           # records in use sit at the other end of the table)
        h = _CamHints()
        h.cost = [torch.zeros(n_tiles, dtype=torch.int32, device=device) for _ in range(2)] if cost else None
        h.cur, h.cost_valid = 0, False
        # ... and two of per-QUADRANT times of the blend backward's waves (4 words per tile)
        h.bcost = [torch.zeros(4 * n_tiles, dtype=torch.int32, device=device) for _ in range(2)] if cost else None
        h.bcur, h.bwritten, h.bvalid = 0, False, False
        # raw streams these buffers have been used on: the one they were allocated on + every other one, each told to the caching
        # allocator once (Tensor.record_stream), so that an evicted record's memory is not handed out while a kernel of another
        # stream still writes it (the operator is re-entrant per stream since round 5)
        h.streams = {_stream(device)}
        h.long_np = h.long_ptr = h.slot = None
        if long_words:
            h.slot, h.long_np, h.long_ptr = _long_words()
    _CAM_HINTS[key] = h                                          # (re-inserted: most recently used last)
    return h


_FRAME_CACHE = {}
# ScgFrame.long_lists_out words come from ONE pinned allocation per process (a pinned allocation per camera would cost a render
# loop over hundreds of distinct cameras ~50 us each): one slot of two words per live hint record (_CAM_HINTS), returned to
# the free list when the record is evicted.  The words are a HINT (which sort kernels to launch) — a wrong one costs time,
# never a result (the forward blend sorts a list nobody sorted for it,
# tests/test_gpu_parity.py::test_skipped_rare_sort_launch_...).
_LONG_POOL = None
_LONG_FREE = []


def _long_words():
    """(slot index, numpy view of the slot's two words, device-visible address of the slot)."""
    global _LONG_POOL
    if _LONG_POOL is None:
        t = torch.full((2 * (_CAM_HINTS_MAX + 1),), -1, dtype=torch.int32).pin_memory()
        _LONG_POOL = (t, t.numpy(), t.data_ptr())
        _LONG_FREE.extend(range(_CAM_HINTS_MAX, -1, -1))
    _t, arr, base = _LONG_POOL
    if not _LONG_FREE:                   # records that left the table without passing _release_long_words (a cleared table)
        used = {h.slot for h in _CAM_HINTS.values()}
        _LONG_FREE.extend(i for i in range(_CAM_HINTS_MAX, -1, -1) if i not in used)
    i = _LONG_FREE.pop()
    view = arr[2 * i: 2 * i + 2]
    view[:] = -1                         # "no render of this camera has completed yet"
    return i, view, base + 8 * i


def _release_long_words(h):
    if h.slot is not None:
        _LONG_FREE.append(h.slot)
        h.slot = h.long_np = h.long_ptr = None


def _frame_for(settings, P: int, M: int, device, forward: bool = False, cam_key=None, switches=(True, True, True)) -> _Frame:
    """ScgFrame structs are cached by what they contain (pointers + scalars): building the ctypes struct costs more
    host time than some of the kernels it describes take.  Only frames whose four small tensors are used as they
    are (fp32, contiguous, on the device) are cached — the cached frame keeps them alive, so their addresses cannot be
    recycled, and their CONTENT is read by the kernels at launch time, not here.  `forward`: a forward is about to be launched."""
    small = (settings.viewmatrix, settings.projmatrix, settings.campos, settings.bg)
    for t in small:
        if not (isinstance(t, torch.Tensor) and t.dtype == torch.float32 and t.device == device and t.is_contiguous()
                and t.numel() > 0):
            return _Frame(settings, P, M, device)
    key = (small[0].data_ptr(), small[1].data_ptr(), small[2].data_ptr(), small[3].data_ptr(),
           settings.image_height, settings.image_width, settings.tanfovx, settings.tanfovy,
           settings.scale_modifier, settings.sh_degree, settings.prefiltered, settings.debug, P, M, device.index)
    fr = _FRAME_CACHE.get(key)
    if fr is None:
        if len(_FRAME_CACHE) > 256:
            _FRAME_CACHE.clear()
        fr = _FRAME_CACHE[key] = _Frame(settings, P, M, device)
    if forward:
        fr.next_forward(device, cam_key, switches)
    return fr

"""The capacity policy, the per-device state it lives in, and the counts of renders launched without a host read.

A forward is launched with a CAPACITY — an upper bound of num_rendered, the number of (Gaussian, tile) instances — and learns the
real count either at once (the default: the host waits for the geometry stage's partial sums) or LATER: with rasterizer.no_host_read()
/ inside a stream capture the binning stage leaves its count in a pinned word (ScgFrame.num_rendered_out) that is looked at the next
time the camera is rendered.  This module owns the per-device _SpecState and every access to its two capacity tables (lookup,
lookup_shape, commit, commit_shape, forget: nothing outside this file touches `hint` / `cam_hint`), what a forward takes from the
state (_PinnedSums, _Plan), and the pinned count words with what a count that has arrived does to the camera's capacity
(_settle_word -> commit; file_word, release, settle_replayed, capture_record: how the words are pooled is known here only).
rasterizer.py decides in which mode a forward runs, launches it and repeats one that overflowed.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import threading

import torch

from . import _lib
from ._lib import check

_SPEC_STATE = {}                         # device index -> _SpecState
_TABLE_MAX, _TABLE_TRIM = 1024, 128      # a capacity table beyond _TABLE_MAX entries loses its _TABLE_TRIM oldest


def _capacity_for(R: int) -> int:
    """Upper bound of num_rendered to lay point_list out for, given the latest count: ~12-25 % head room, quantised to
    1/16 of its magnitude so that the value (and the cached workspace plan keyed by it) stays put from step to step."""
    need = int(R * 1.125) + 4096
    g = 1 << max(12, need.bit_length() - 4)
    return (need + g - 1) // g * g


def _next_capacity(cur, R: int) -> int:
    """Keep the capacity in use while the count sits comfortably inside it; otherwise re-derive it from the count."""
    if cur is not None and R + (R >> 5) <= cur <= 2 * R + 65536:
        return cur
    return _capacity_for(R)


def first_sight_capacity(P: int) -> int:
    """The bound of a render nothing is known about: too small is repaired by the overflow retry or the camera's next render."""
    return _capacity_for(4 * P)


def lookup(spec, P, W, H, cam, capturing=False, allow_first_sight=False):
    """The capacity to launch camera `cam` (_camera_key) with; None: nothing is known, the staged path establishes it.
    Remembered per CAMERA (views of one scene can differ by more than 2x in num_rendered: a bound shared by all of them would
    shrink after the cheap view and overflow on the expensive one, every other step), keyed WITHOUT the Gaussian count:
    densification changes P every ~100 iterations and must not put hundreds of cameras back on the shared fallback — after a
    change of P the camera's last num_rendered is rescaled by the ratio of the counts.  A camera seen for the first time starts
    from the latest bound of any camera of this shape, or (`allow_first_sight`: model path, no host read) from 4 P."""
    ent = spec.cam_hint.get((W, H, cam))
    if ent is not None:
        cap, R_c, P_c = ent
        if P_c != P:
            cap = _capacity_for(int(R_c * (P / max(P_c, 1))) + 1)
        if capturing:                                        # a captured step keeps its capacity for every replay: more head room
            cap = max(cap, _capacity_for(int(R_c * (P / max(P_c, 1)) * 1.25) + 1))
        return cap
    cap = spec.hint.get((P, W, H))
    return first_sight_capacity(P) if (cap is None and allow_first_sight) else cap


def lookup_shape(spec, P, W, H):
    """The latest bound of ANY camera of this shape (the staged forward's guess), or None."""
    return spec.hint.get((P, W, H))


def commit(spec, P, W, H, cam, cap, R):
    """The next render of this camera, and of a new camera of this shape, starts from `cap` (derived from the count `R`).  The
    camera's entry is re-inserted: the tables' order is the eviction order, the trim never takes the entry just written."""
    spec.hint[(P, W, H)] = cap
    ckey = (W, H, cam)
    spec.cam_hint.pop(ckey, None)
    spec.cam_hint[ckey] = (cap, R, P)
    for table in (spec.hint, spec.cam_hint):
        if len(table) > _TABLE_MAX:
            for k in list(table)[:_TABLE_TRIM]:
                del table[k]


def commit_shape(spec, P, W, H, R):
    """The staged forward's update: it knows the exact count and no camera."""
    spec.hint[(P, W, H)] = _next_capacity(spec.hint.get((P, W, H)), R)


def forget(spec, P, W, H, cam):
    """The bound this camera needs no longer fits the tile-first binning: its next render takes the staged path."""
    spec.cam_hint.pop((W, H, cam), None)
    spec.hint.pop((P, W, H), None)


class _SpecState:
    """Per-device state of the speculative launch: the two capacity tables (read and written by the policy functions above
    only), pinned host memory for the partial sums of num_rendered, the workspace plans, the pending count words."""

    def __init__(self, device):
        self.hint = {}                   # (P, W, H) -> capacity: the latest bound of ANY camera of this shape
        self.cam_hint = {}               # (W, H, camera) -> (capacity, num_rendered, P it was taken at)
        # pinned host scratch of the forwards IN FLIGHT on this device: one _PinnedSums per forward, taken from / returned to a
        # free list (round 5: the operator is re-entrant — two threads, each on its own stream, may be inside a forward at the
        # same time, as with the upstream extension; one shared scratch made the second one raise)
        self.free = []
        self.pool_lock = threading.Lock()
        self.plans = {}                  # (P, W, H, capacity) -> _Plan
        self.pending = {}                # (W, H, camera) -> [_CountWord]: no-host-read renders whose count nobody has looked at yet

    def take(self, nbytes: int) -> "_PinnedSums":
        """Pinned host memory used as the geometry stage's scratch for ONE forward: the kernel writes its per-workgroup
        partial sums of num_rendered straight to the host, so the speculative path needs neither a total kernel nor a D2H
        copy.  give_back() when the count has been read."""
        with self.pool_lock:
            ps = self.free.pop() if self.free else None
        if ps is None or ps.nbytes < nbytes:
            ps = _PinnedSums(nbytes)
        return ps

    def give_back(self, ps: "_PinnedSums"):
        with self.pool_lock:
            if len(self.free) < 8:
                self.free.append(ps)

    def plan(self, lib, P, W, H, cap):
        key = (P, W, H, cap)
        pl = self.plans.get(key)
        if pl is None:
            if len(self.plans) > 64:
                self.plans.clear()
            pl = self.plans[key] = _Plan(lib, P, W, H, cap)
        return pl


class _PinnedSums:
    """The pinned words one forward's geometry kernel writes its partial sums of num_rendered to, and the events of the paths
    that wait on one (the staged path; the one-call path with EVENTLESS_WAIT off)."""
    __slots__ = ("t", "np", "ptr", "nbytes", "event", "raw_event")

    def __init__(self, nbytes: int):
        self.t = torch.zeros(((nbytes + 3) // 4 + 1024,), dtype=torch.int32).pin_memory()
        self.np = self.t.numpy()
        self.ptr = self.t.data_ptr()
        self.nbytes = self.t.numel() * 4
        self.event = None                # torch.cuda.Event of the staged path
        self.raw_event = None            # hipEvent_t (timing disabled) of the one-call path

    def torch_event(self):
        if self.event is None:
            self.event = torch.cuda.Event()
        return self.event

    def event_handle(self):
        if self.raw_event is None:
            h = C.c_void_p()
            check(_lib.load().scg_event_create(C.byref(h), 0), "scg_event_create")
            self.raw_event = h.value
        return self.raw_event


class _Plan:
    """Workspace layout of one (P, W, H, capacity): byte offsets reported by the library, looked up once."""

    __slots__ = ("total", "final_T", "n_contrib", "point_list", "ranges", "splats", "rects", "depth_keys", "clamped",
                 "partial_bytes", "accepts", "fused", "_shape")

    def __init__(self, lib, P, W, H, cap):
        L = _lib.ScgWorkspaceLayout()
        check(lib.scg_workspace_layout(P, cap, W, H, C.byref(L)), "scg_workspace_layout")
        self.total = int(L.total)
        for k in ("final_T", "n_contrib", "point_list", "ranges", "splats", "rects", "depth_keys", "clamped"):
            setattr(self, k, int(getattr(L, k)))
        self.partial_bytes = int(L.partial_words) * 4
        self.accepts = lib.scg_binning_accepts_bound(cap, W, H, _lib.BINNING_AUTO) == 1
        # ScgFrame.long_lists_out is written by the forward blend that sorts its own tiles; a frame whose sort is a kernel of
        # its own (the library's A/B bit, FUSED_SORT = False) leaves the words alone (fused[options]: which one runs)
        self.fused = {}
        self._shape = (cap, W, H)

    def sorts_in_blend(self, lib, options: int) -> bool:
        v = self.fused.get(options)
        if v is None:
            v = self.fused[options] = lib.scg_forward_sorts_in_blend(*self._shape, options) == 1
        return v


def _spec_state(device) -> _SpecState:
    key = device.index if device.index is not None else torch.cuda.current_device()
    st = _SPEC_STATE.get(key)
    if st is None:
        st = _SPEC_STATE[key] = _SpecState(device)
    return st


_COUNT_ARMED = 0xFFFFFFFF                # "the binning stage of this render has not written its count yet"
_COUNT_POOL = None                       # one pinned allocation of count words per process
_COUNT_FREE = []
_COUNT_SLOTS = 4096
_OVERFLOW = {"renders": 0, "overflows": 0, "settled": 0}
_ANON_CAPTURED = []                      # count words of forwards captured by somebody else's graph (kept: the graph writes them)
_CAPTURE_RECORD = None                   # graph_step's record of the forwards captured right now (None: no capture of ours)
_QUARANTINE = []                         # pinned blocks of forwards that failed after their launch (never handed out again)


class _CountWord:
    """One pinned word that a render's binning stage overwrites with num_rendered + what the binding needs to judge it later."""
    __slots__ = ("slot", "np", "ptr", "cap", "P", "key", "device_index", "captured")

    def value(self):
        v = int(self.np[0])
        return None if v == _COUNT_ARMED else v


def _count_pool():
    """The process's pinned count words (allocated at the first use — graph_step asks BEFORE it starts a capture: a pinned
    allocation inside a capture is not allowed)."""
    global _COUNT_POOL
    if _COUNT_POOL is None:
        t = torch.full((_COUNT_SLOTS,), -1, dtype=torch.int32).pin_memory()
        _COUNT_POOL = (t, t.numpy().view("uint32"), t.data_ptr())
        _COUNT_FREE.extend(range(_COUNT_SLOTS - 1, -1, -1))
    return _COUNT_POOL


def _count_word(cap, P, key, device_index) -> _CountWord:
    _count_pool()
    if not _COUNT_FREE:                                      # every slot is waiting for its render: let the device catch up
        torch.cuda.synchronize()
        settle_counts()
        if not _COUNT_FREE:
            raise _lib.ScgError("no_host_read: more than %d renders (or captured steps) hold a count word" % _COUNT_SLOTS)
    _t, arr, base = _COUNT_POOL
    w = _CountWord()
    w.slot = _COUNT_FREE.pop()
    w.np = arr[w.slot: w.slot + 1]
    w.np[0] = _COUNT_ARMED
    w.ptr = base + 4 * w.slot
    w.cap, w.P, w.key, w.device_index, w.captured = int(cap), int(P), key, device_index, False
    return w


@contextlib.contextmanager
def capture_record():
    """`with capture_record() as words:` — the count words of the forwards captured inside are filed into `words`."""
    global _CAPTURE_RECORD
    prev, _CAPTURE_RECORD = _CAPTURE_RECORD, []
    try:
        yield _CAPTURE_RECORD
    finally:
        _CAPTURE_RECORD = prev


def file_word(spec, cw: _CountWord, ckey, capturing: bool):
    """Who looks at a launched forward's word later: the capture's owner (nobody's: settle_counts) or the camera's next render."""
    _OVERFLOW["renders"] += 1
    if capturing:
        cw.captured = True
        (_CAPTURE_RECORD if _CAPTURE_RECORD is not None else _ANON_CAPTURED).append(cw)
    else:
        spec.pending.setdefault(ckey, []).append(cw)


def release(words):
    """Give the words' slots back (nothing writes them any more: a graph that is gone, a forward the library rejected)."""
    _COUNT_FREE.extend(w.slot for w in words)


def settle_replayed(w: _CountWord):
    """A word that a graph's replays write: None while no count has arrived, else the latest count, settled; the word is re-armed."""
    R = w.value()
    if R is not None:
        w.np[0] = _COUNT_ARMED
        spec = _SPEC_STATE.get(w.device_index if w.device_index is not None else torch.cuda.current_device())
        if spec is not None:
            _settle_word(spec, w, R)
    return R


def _settle_word(spec, w: _CountWord, R: int):
    """The count of a render that was launched without a host read has arrived: the camera's capacity follows it."""
    _OVERFLOW["settled"] += 1
    if R > w.cap:
        _OVERFLOW["overflows"] += 1
    W, H, cam = w.key
    ent = spec.cam_hint.get(w.key)
    cur = ent[0] if (ent is not None and ent[2] == w.P) else w.cap
    commit(spec, w.P, W, H, cam, _next_capacity(max(cur, w.cap) if R <= w.cap else None, R), R)


def _settle_camera(spec, key):
    """Look (without waiting) at the count words of this camera's earlier no-host-read renders, oldest first."""
    q = spec.pending.get(key)
    if not q:
        return
    while q:
        w = q[0]
        R = w.value()
        if R is None:
            break
        q.pop(0)
        _settle_word(spec, w, R)
        _COUNT_FREE.append(w.slot)
    if not q:
        spec.pending.pop(key, None)


def settle_counts(device=None) -> dict:
    """Look at every outstanding count word (after a synchronisation of the caller's all of them have arrived) and return
    overflow_stats().  Never waits."""
    for idx, spec in list(_SPEC_STATE.items()):
        if device is not None and torch.device(device).index not in (None, idx):
            continue
        for key in list(spec.pending):
            _settle_camera(spec, key)
    for w in _ANON_CAPTURED:                                 # words a foreign graph's replays write: the latest count, once each
        settle_replayed(w)
    return overflow_stats()


def overflow_stats() -> dict:
    """{"renders": forwards launched without a host read, "settled": of those, counts looked at so far, "overflows": of those,
    renders whose lists were clipped (their result was incomplete; the next render of the camera had room again)}."""
    return dict(_OVERFLOW)

"""StageTimer, and the slot (ACTIVE, set_stage_timer) for the one that every rasterizer call without a timer of its own uses."""
from __future__ import annotations

import contextlib
import ctypes as C
from typing import Callable, Optional

import torch

from . import _lib
from ._lib import check


def _no_timer(name: str):
    return contextlib.nullcontext()


ACTIVE: Callable = _no_timer


def set_stage_timer(timer: Optional[Callable]):
    """Install a StageTimer used by every rasterizer call that does not pass its own (bench.py); None removes it."""
    global ACTIVE
    ACTIVE = timer if timer is not None else _no_timer


class StageTimer:
    """Optional per-stage timing with events recorded on the stream the kernels are launched on (torch's
    current stream).  Usage: t = StageTimer(); forward_stages(..., timer=t); t.summary() after a sync.

    The one-call entry points (scg_forward / scg_backward) record their stages' events themselves
    (include/scg_raster.h ScgStageEvents): `stage_events()` hands them a struct of raw hipEvent_t pairs from this
    timer's pool, so the per-stage times of the REAL fast path are measured, not those of a staged replay."""

    FORWARD = ("geometry_forward", "binning", "blend_forward")
    BACKWARD = ("blend_backward", "geometry_backward")

    def __init__(self, only=None):
        self.events = {}
        self.raw = {}                                            # name -> [(begin handle, end handle)]
        self.only = set(only) if only is not None else None      # restrict to these stages (less event traffic)
        self._pool = []
        self._raw_pool = {}                                      # device index -> [hipEvent_t]: an event belongs to a device
        self._structs = []                                       # keeps the ctypes structs alive until summary()

    def _event(self):
        if not self._pool:                                       # created in batches, off the per-stage path
            self._pool = [torch.cuda.Event(enable_timing=True) for _ in range(256)]
        return self._pool.pop()

    def _raw_event(self, dev):
        pool = self._raw_pool.setdefault(dev, [])
        if not pool:                                             # created on the CURRENT device: callers are inside
            lib = _lib.load()                                    # `with _on_device(dev)`
            for _ in range(256):
                h = C.c_void_p()
                check(lib.scg_event_create(C.byref(h), 1), "scg_event_create")
                pool.append(h.value)
        return pool.pop()

    def stage_events(self, direction: str):
        """ScgStageEvents (by reference) for one scg_forward ('forward') / scg_backward ('backward') call, or None."""
        names = self.FORWARD if direction == "forward" else self.BACKWARD
        wanted = [i for i, n in enumerate(names) if self.only is None or n in self.only]
        if not wanted:
            return None
        ev = _lib.ScgStageEvents()
        dev = torch._C._cuda_getDevice()
        for i in wanted:
            a, b = self._raw_event(dev), self._raw_event(dev)
            ev.begin[i], ev.end[i] = a, b
            self.raw.setdefault(names[i], []).append((a, b, dev))
        self._structs.append(ev)
        return C.byref(ev)

    def __call__(self, name: str):
        if self.only is not None and name not in self.only:
            return contextlib.nullcontext()
        return self._timed(name)

    @contextlib.contextmanager
    def _timed(self, name: str):
        a, b = self._event(), self._event()
        a.record()
        try:
            yield
        finally:
            b.record()
            self.events.setdefault(name, []).append((a, b))

    def summary(self):
        """{stage: (mean ms, calls)}; synchronises."""
        torch.cuda.synchronize()
        out = {k: [a.elapsed_time(b) for a, b in v] for k, v in self.events.items()}
        if self.raw:
            lib = _lib.load()
            ms = C.c_float()
            for k, pairs in self.raw.items():
                for a, b, _dev in pairs:
                    check(lib.scg_event_elapsed_ms(a, b, C.byref(ms)), "scg_event_elapsed_ms")
                    out.setdefault(k, []).append(ms.value)
        return {k: (sum(v) / len(v), len(v)) for k, v in out.items()}

    def reset(self):
        for pairs in self.raw.values():                          # completed events go back to their device's pool
            for a, b, dev in pairs:
                self._raw_pool.setdefault(dev, []).extend((a, b))
        self.events, self.raw, self._structs = {}, {}, []

    def close(self):
        """Destroy the raw hipEvents of this timer (pool and recorded pairs)."""
        self.reset()
        pools, self._raw_pool = self._raw_pool, {}
        try:
            lib = _lib.load()
            for pool in pools.values():
                for h in pool:
                    lib.scg_event_destroy(h)
        except Exception:                                        # interpreter shutdown: the driver reclaims them
            pass

    def __del__(self):
        self.close()

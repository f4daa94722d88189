"""The Adam step of csrc/adam_math.h restated in numpy float32, one operation per statement, and what the edge tests need around it.

The contract the kernel is held to is not torch's bits (torch's CPU lerp is fused, its exp_avg_sq is not always; see
tests/test_optim_refs_cpu.py) but what adam_math.h states and -ffp-contract=off is there for: fp32 throughout, one rounding per
operation, in torch's order.  `adam_step_ref` is that, `adam_step_f64` the same step in double (the anchor of the restatement
itself), `MUTANTS` the subtly wrong kernels the bit-level bar has to notice, `live_after` the watermark the header promises.

Frames are built from seeds alone.  `Runner` calls scg_adam_step directly (no ArenaAdam): every tensor is carved out of a larger
buffer whose remainder holds a sentinel bit pattern, the carve offset sets the alignment, and the workspace is the runner's own.

The numbers the GPU tests use for (b1, b2, lr, step) all come from LRS / BETAS / STEPS_IN / STEP_LATE below: the coefficient
premise (the host's and the device's double pow may differ by an ulp or two without moving the two fp32 coefficients) is
asserted over all of them on the CPU."""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import List, Optional, Sequence

import numpy as np

F = np.float32
CHUNK = 4096                                   # kAdamChunk of csrc/optim.hip: elements per workgroup
WS_WORDS = 64                                  # scg_adam_workspace_bytes / 4
WS_LIVE_NEXT, WS_LIVE = 16, 32
FORCE_FULL = 1

# the reference's six learning rates, the position schedule of test_gpu_optim.Model.step at the iterations (g) runs, two more
LRS_REFERENCE = (1.6e-4, 2.5e-3, 2.5e-3 / 20, 5e-2, 5e-3, 1e-3)
LRS_SCHEDULE = tuple(1.6e-4 * (0.99 ** it) for it in range(1, 9))
LRS = LRS_REFERENCE + LRS_SCHEDULE + (3e-4, 7e-2)
BETAS = ((0.9, 0.999), (0.8, 0.99), (0.5, 0.9999))
STEPS_IN = (0, 1, 9, 199)                      # incoming step counters
STEP_LATE = 29999                              # the reference's last iteration: both bias corrections are 1 in fp32
STEPS_AHEAD = 12                               # no test launches more often than this from one incoming step

MUTANTS = ("eps_omitted", "eps_under_root", "eps_before_div", "bc2_not_rooted", "step_not_incremented", "lerp_fused", "v_fused",
           "g_squared_first", "denormals_flushed")
LIVE_MUTANTS = ("live_plus_1", "live_minus_1")
TINY = np.float32(np.finfo(np.float32).tiny)   # smallest normal


def bits(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def cbits(a) -> np.ndarray:
    """The bits with every NaN as one pattern: IEEE 754 leaves a NaN's sign and payload to the implementation (an x86 host makes
    0xFFC00000 of 0/0, the GPU 0x7FC00000), so that NaN is where NaN is expected is all a comparison can ask."""
    a = np.ascontiguousarray(a, dtype=np.float32).ravel()
    return np.where(np.isnan(a), np.uint32(0x7FC00000), a.view(np.uint32))


def same_bits(a, b) -> bool:
    return np.array_equal(cbits(a), cbits(b))


def differing(a, b) -> int:
    return int((cbits(a) != cbits(b)).sum())


# ------------------------------------------------------------------------------------------------------------ the restatement

def pow_nudged(b: float, t: float, ulps: int = 0) -> float:
    r = b ** t
    for _ in range(abs(ulps)):
        r = math.nextafter(r, math.inf if ulps > 0 else -math.inf)
    return r


def bias_coefs(step, lr: float, b1: float, b2: float, mutant: Optional[str] = None, nudge=(0, 0)):
    """(bc2s, nss) of the launch that finds `step` in the counter: adam_bias_coefs of adam_math.h.  nudge = ulps added to the two
    double pow results (the coefficient premise)."""
    step1 = F(step) + F(1)
    t = float(F(step)) if mutant == "step_not_incremented" else float(step1)
    with np.errstate(all="ignore"):
        bc1 = np.float64(1.0) - np.float64(pow_nudged(b1, t, nudge[0]))
        bc2 = np.float64(1.0) - np.float64(pow_nudged(b2, t, nudge[1]))
        bc2s = F(bc2) if mutant == "bc2_not_rooted" else F(np.sqrt(bc2))
        nss = F(-(np.float64(lr) / bc1))
    return bc2s, nss


def _ftz(a):
    a = np.array(a, dtype=np.float32)
    a[np.abs(a) < TINY] *= F(0)                # keeps the sign, as a flushing unit does
    return a


def adam_step_ref(p, m, v, g, step, lr, b1, b2, eps, coefs=None, mutant: Optional[str] = None):
    """One step on every element (no skipping): returns new (p, m, v) as float32 arrays.  coefs = (bc2s, nss) overrides the two
    step-dependent coefficients.  mutant: one of MUTANTS, a subtly wrong kernel."""
    assert mutant is None or mutant in MUTANTS, mutant
    p, m, v, g = (np.array(x, dtype=np.float32) for x in (p, m, v, g))
    if mutant == "denormals_flushed":
        p, m, v, g = _ftz(p), _ftz(m), _ftz(v), _ftz(g)
    bc2s, nss = coefs if coefs is not None else bias_coefs(step, lr, b1, b2, mutant)
    bc2s, nss = F(bc2s), F(nss)
    w1 = F(1.0 - b1)
    b2f = F(b2)
    w2 = F(1.0 - b2)
    epsf = F(eps)
    with np.errstate(all="ignore"):
        if mutant == "lerp_fused":
            m = (m.astype(np.float64) + np.float64(w1) * (g.astype(np.float64) - m.astype(np.float64))).astype(np.float32)
        else:
            d = g - m
            d = w1 * d
            m = m + d
        if mutant == "v_fused":
            g64 = g.astype(np.float64)
            v = (v.astype(np.float64) * np.float64(b2f) + np.float64(w2) * g64 * g64).astype(np.float32)
        else:
            a = v * b2f
            if mutant == "g_squared_first":
                c = g * g
                c = w2 * c
            else:
                c = w2 * g
                c = c * g
            v = a + c
        if mutant == "eps_omitted":
            den = np.sqrt(v)
            den = den / bc2s
        elif mutant == "eps_under_root":
            den = v + epsf
            den = np.sqrt(den)
            den = den / bc2s
        elif mutant == "eps_before_div":
            den = np.sqrt(v)
            den = den + epsf
            den = den / bc2s
        else:
            den = np.sqrt(v)
            den = den / bc2s
            den = den + epsf
        q = m / den
        q = nss * q
        p = p + q
    if mutant == "denormals_flushed":
        p, m, v = _ftz(p), _ftz(m), _ftz(v)
    assert p.dtype == m.dtype == v.dtype == np.float32
    return p, m, v


def adam_step_f64(p, m, v, g, step, lr, b1, b2, eps):
    """The same step from the same fp32 state, every operation in double (Python's scalars as they are): new (p, m, v), float64."""
    p, m, v, g = (np.asarray(x, dtype=np.float32).astype(np.float64) for x in (p, m, v, g))
    t = float(step) + 1.0
    bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
    with np.errstate(all="ignore"):
        m = m + (1.0 - b1) * (g - m)
        v = v * b2 + (1.0 - b2) * g * g
        den = np.sqrt(v) / math.sqrt(bc2) + eps
        p = p + (-(lr / bc1)) * (m / den)
    return p, m, v


def live_after(m, v, row_len: int, mutant: Optional[str] = None) -> int:
    """The largest column with m != 0 or v != 0, plus 1, over all rows; 0 when there is none.  NaN counts as non-zero."""
    m, v = np.asarray(m, dtype=np.float32).reshape(-1, row_len), np.asarray(v, dtype=np.float32).reshape(-1, row_len)
    cols = np.nonzero(((m != 0) | (v != 0)).any(axis=0))[0]
    w = int(cols.max()) + 1 if cols.size else 0
    if mutant == "live_plus_1":
        return w + 1
    if mutant == "live_minus_1":
        return w - 1
    assert mutant is None, mutant
    return w


# ---------------------------------------------------------------------------------------------------------------- the frames

@dataclass
class Seg:
    """One segment of a launch and the gradients of its successive launches."""
    p: np.ndarray
    m: np.ndarray
    v: np.ndarray
    g: List[np.ndarray]                        # one per launch
    step: float = 0.0
    lr: float = 1e-3
    b1: float = 0.9
    b2: float = 0.999
    eps: float = 1e-15
    row_len: int = 0
    off: Sequence[int] = (0, 0, 0, 0)          # carve offsets in bytes of p, g, m, v
    name: str = ""
    w: int = -1                                # row frames: the watermark the frame was built for

    def __post_init__(self):
        # only what the coefficient premise covers (tests/test_optim_refs_cpu.py)
        assert self.lr in LRS and (self.b1, self.b2) in BETAS and self.step in STEPS_IN + (STEP_LATE,), self.name

    @property
    def numel(self) -> int:
        return int(self.p.size)


def empty_seg(step: float, launches: int, **kw) -> Seg:
    z = np.zeros(0, np.float32)
    return Seg(z, z.copy(), z.copy(), [z.copy() for _ in range(launches)], step=step, name="empty", **kw)


def plain_seg(numel: int, seed: int, launches: int = 3, off=(0, 0, 0, 0), **kw) -> Seg:
    """Random state and gradients of the size the suite's other Adam tests use (|g| about 1e-2)."""
    r = np.random.default_rng(seed)
    f = lambda s: (r.standard_normal(numel) * s).astype(np.float32)          # noqa: E731
    return Seg(f(1.0), f(1e-3), np.abs(f(1e-3)) ** 2, [f(1e-2) for _ in range(launches)], off=off,
               name=f"plain n={numel} off={tuple(off)}", **kw)


G_VALUES = np.array([0.0, -0.0, 1e-38, -1e-38, 1e-25, -1e-25, 1e-20, 1e-12, -1e-12, 1e-8, 1e-3, -1e-3, 1.0, -1.0, 1e19, -1e19, 3e19, -3e19, 1e21, -1e21,
                     np.nan, np.inf, -np.inf], dtype=np.float32)
DENORM_MIN = np.float32(1.401298464324817e-45)
M_VALUES = np.array([0.0, DENORM_MIN, -DENORM_MIN, 1e-30, 3e-3, -0.25], dtype=np.float32)
V_VALUES = np.array([0.0, DENORM_MIN, 1e-30, 7e-5], dtype=np.float32)
ARITH_NUMEL = CHUNK + 5


def arith_seg(eps: float, step: float, seed: int = 0, launches: int = 2, lr: float = 1e-3) -> Seg:
    """Every combination of G_VALUES x M_VALUES x V_VALUES, repeated over 4096 + 5 elements in a seeded order; p from a normal
    draw with +0 and -0 strewn in.  The second launch's gradient is the first's, rotated by 7 elements."""
    r = np.random.default_rng(seed)
    n = ARITH_NUMEL
    combo = r.permutation(n) % (G_VALUES.size * M_VALUES.size * V_VALUES.size)
    g = G_VALUES[combo % G_VALUES.size]
    m = M_VALUES[(combo // G_VALUES.size) % M_VALUES.size]
    v = V_VALUES[combo // (G_VALUES.size * M_VALUES.size)]
    p = r.standard_normal(n).astype(np.float32)
    p[::5] = 0.0
    p[::10] = -0.0
    return Seg(p, m.copy(), v.copy(), [np.roll(g, 7 * k).copy() for k in range(launches)], step=step, eps=eps, lr=lr,
               name=f"arith eps={eps:g} step={step:g}")


def row_seg(rows: int, row_len: int, w: int, seed: int, launches: int = 4, off=(0, 0, 0, 0), **kw) -> Seg:
    """Moments zero at columns >= w and non-zero below (every seventh element a denormal); gradients zero at columns >= w.
    Column w - 1 holds denormal moments in every row and zero gradients in launches 0 and 1: they stay denormal, so the watermark
    rests on denormals alone and a unit that flushed them would report w - 1.  Launch 2 feeds that column (its moments become
    normal), launch 3 does not again: the last live column then decays with a zero gradient, which a skip that took it for dead
    would leave untouched."""
    assert 0 <= w <= row_len
    r = np.random.default_rng(seed)
    n = rows * row_len
    col = np.arange(n) % row_len
    below = col < w
    m = np.where(r.random(n) < 0.5, -1.0, 1.0) * (1e-3 + 1e-3 * r.random(n))
    v = 1e-6 + 1e-6 * r.random(n)
    m, v = m.astype(np.float32), v.astype(np.float32)
    m[::7] = DENORM_MIN * F(3)
    v[::7] = DENORM_MIN
    m[~below] = 0
    v[~below] = 0
    m[col == w - 1] = DENORM_MIN * F(3)
    v[col == w - 1] = DENORM_MIN
    gs = []
    for k in range(launches):
        g = (r.standard_normal(n) * 1e-2).astype(np.float32)
        g[~below] = 0
        if k != 2:
            g[col == w - 1] = 0
        gs.append(g)
    return Seg(r.standard_normal(n).astype(np.float32), m, v, gs, row_len=row_len, off=off, w=w,
               name=f"rows={rows} L={row_len} w={w} off={tuple(off)}", **kw)


def row_premises(numel: int, row_len: int, live: int) -> dict:
    """What the float4 groups and workgroup chunks of a row segment look like: is there a group with columns on both sides of
    `live`, a group that wraps a row end, a row that has elements on both sides of element 4096."""
    q = np.arange(numel // 4)
    cols = (q[:, None] * 4 + np.arange(4)[None, :]) % row_len
    lo = (cols < live).any(axis=1) & (cols >= live).any(axis=1)
    wrap = (cols[:, 1:] <= cols[:, :-1]).any(axis=1)
    crosses = numel > CHUNK and CHUNK % row_len != 0
    return dict(straddles_live=bool(lo.any()), wraps_row=bool(wrap.any()), row_crosses_chunk=bool(crosses))


ROW_WS = (0, 1, 3, 4, 5, 9, 24, 44, 45)
ROW_COUNTS = (1, 91, 92, 273)
OTHER_ROW_LENS = {1: ((4099, 0), (4099, 1)), 3: ((1367, 0), (1367, 2), (1367, 3)), 4: ((1025, 1), (1025, 3), (1025, 4)),
                  48: ((86, 0), (86, 5), (86, 47), (86, 48)), 4097: ((3, 0), (3, 1), (3, 4095), (3, 4097))}    # L: ((rows, w), ...)


PLAIN_SIZES = (1, 3, 4, 5, 4095, 4096, 4097, 8193)
PLAIN_OFFSETS = ((0, 0, 0, 0), (4, 4, 4, 4), (8, 8, 8, 8), (12, 12, 12, 12), (0, 4, 0, 0))     # the last: the gradient alone
ARITH_EPS = (1e-15, 1e-8)


def plain_frames(off=(0, 0, 0, 0)) -> List[Seg]:
    return [plain_seg(n, seed=100 + n, off=off) for n in PLAIN_SIZES]


def arith_frames() -> List[Seg]:
    return [arith_seg(eps, step, seed=int(step) + i) for i, eps in enumerate(ARITH_EPS) for step in STEPS_IN + (STEP_LATE,)]


def row_frames(rows: int, off=(0, 0, 0, 0)) -> List[Seg]:
    return [row_seg(rows, 45, w, seed=1000 * rows + w, off=off) for w in ROW_WS]


def other_row_frames() -> List[Seg]:
    return [row_seg(rows, L, w, seed=7 * L + w) for L, cases in OTHER_ROW_LENS.items() for rows, w in cases]


MOVE_ROWS, MOVE_W = 92, 9


def moving_frames() -> dict:
    """The w = 9 state of 92 rows; launch 0 establishes the watermark, launch 1 carries the gradient that should (or should not)
    move it, launch 2 is ordinary again.  {name: (Seg, watermark expected after launch 1)}."""
    L, out = 45, {}
    at = lambda row, col: row * L + col                                     # noqa: E731
    assert at(91, 9) > CHUNK                                               # a row of the second workgroup

    def frame(name, edit, want):
        s = row_seg(MOVE_ROWS, L, MOVE_W, seed=4242, launches=3)
        edit(s.g[1])
        s.name = f"moving {name}"
        out[name] = (s, want)

    def at_live(g):
        g[at(91, 9)] = 3e-3

    def at_last(g):
        g[at(91, 44)] = -2e-3

    def poison(g):
        g[at(50, 20)] = np.nan
        g[at(91, 30)] = -np.inf

    def minus_zero(g):
        g[(np.arange(g.size) % L) >= MOVE_W] = -0.0

    frame("column_live", at_live, 10)
    frame("last_column_last_row", at_last, 45)
    frame("nan_and_inf_beyond", poison, 31)
    frame("minus_zero_beyond", minus_zero, 9)
    return out


def sixteen_frame() -> List[Seg]:
    """One launch of 16 segments: empty ones first, in the middle and last, two row segments (45 and 48 columns, watermarks 9 and
    5), plain ones of the sizes of PLAIN_SIZES at every alignment; lr, betas, eps and the incoming step differ per segment."""
    steps = STEPS_IN + (STEP_LATE,)
    hyper = lambda i: dict(lr=LRS[(5 * i + 1) % len(LRS)], b1=BETAS[i % 3][0], b2=BETAS[i % 3][1], eps=ARITH_EPS[i % 2],   # noqa: E731
                           step=steps[i % len(steps)])
    kinds = [("empty",), ("plain", 4097, (0, 0, 0, 0)), ("row", 92, 45, 9), ("plain", 5, (4, 4, 4, 4)), ("empty",),
             ("plain", 4096, (8, 8, 8, 8)), ("row", 86, 48, 5), ("plain", 1, (0, 0, 0, 0)), ("plain", 3, (12, 12, 12, 12)),
             ("plain", 8193, (0, 0, 0, 0)), ("empty",), ("plain", 4095, (0, 4, 0, 0)), ("plain", 4, (0, 0, 0, 0)),
             ("plain", 4095, (4, 4, 4, 4)), ("plain", 4097, (4, 4, 4, 4)), ("empty",)]
    segs = []
    for i, k in enumerate(kinds):
        if k[0] == "empty":
            segs.append(empty_seg(launches=3, **hyper(i)))
        elif k[0] == "plain":
            segs.append(plain_seg(k[1], seed=16 + i, off=k[2], **hyper(i)))
        else:
            segs.append(row_seg(k[1], k[2], k[3], seed=16 + i, launches=3, **hyper(i)))
    assert len(segs) == 16
    return segs


# ------------------------------------------------------------------------------------------ K launches of the restatement

@dataclass
class State:
    p: np.ndarray
    m: np.ndarray
    v: np.ndarray
    step: np.float32
    live: int = 0


def ref_launches(segs: Sequence[Seg], launches: int, lrs: Optional[Sequence[float]] = None, mutant: Optional[str] = None):
    """[[State per segment] per launch]: K successive restatement steps of every segment (empty ones advance their counter)."""
    cur = [State(s.p.copy(), s.m.copy(), s.v.copy(), F(s.step)) for s in segs]
    out = []
    for k in range(launches):
        nxt = []
        for i, (s, c) in enumerate(zip(segs, cur)):
            lr = s.lr if lrs is None else lrs[i]
            p, m, v = c.p, c.m, c.v
            if s.numel:
                p, m, v = adam_step_ref(p, m, v, s.g[k], c.step, lr, s.b1, s.b2, s.eps,
                                        mutant=mutant if mutant in MUTANTS else None)
            live = live_after(m, v, s.row_len, mutant if mutant in LIVE_MUTANTS else None) if s.row_len and s.numel else 0
            nxt.append(State(p, m, v, F(c.step) + F(1), live))
        out.append(nxt)
        cur = nxt
    return out


# ---------------------------------------------------------------------------------------------------------------- the runner

GUARD = 64                                      # sentinel floats in front of and behind every carved tensor
SENTINELS = dict(p=0x4B3C614E, g=0xC2F6E979, m=0x3DFCD6EA, v=0x40490FDB, step=0x447A4000, ws=0x5A5A5A5A)


def _i32(word: int) -> int:
    return word - (1 << 32) if word >= (1 << 31) else word


class Carved:
    """`numel` fp32 (or int32) words at `off` bytes past a 16-byte boundary inside a device buffer full of a sentinel."""

    def __init__(self, numel: int, off: int, sentinel: int, device):
        import torch
        assert off % 4 == 0 and 0 <= off < 16
        self.sentinel, self.numel = _i32(sentinel), numel
        self.buf = torch.full((2 * GUARD + numel + 4,), self.sentinel, dtype=torch.int32, device=device)
        assert self.buf.data_ptr() % 16 == 0
        self.start = GUARD + off // 4
        self.view = self.buf[self.start:self.start + numel]
        assert numel == 0 or self.view.data_ptr() % 16 == off

    def ptr(self) -> Optional[int]:
        return self.view.data_ptr() if self.numel else None

    def write(self, a: np.ndarray) -> None:
        import torch
        assert a.size == self.numel
        if self.numel:
            self.view.copy_(torch.from_numpy(np.ascontiguousarray(a).view(np.int32).copy()))

    def read(self, dtype=np.float32) -> np.ndarray:
        return self.view.cpu().numpy().view(dtype).copy()

    def intact(self) -> bool:
        b = self.buf.cpu().numpy()
        return bool((b[:self.start] == self.sentinel).all() and (b[self.start + self.numel:] == self.sentinel).all())


class Runner:
    """scg_adam_step on the segments of a frame: launch(k) is the k-th launch (gradient k of every segment), without a
    synchronisation of its own."""

    def __init__(self, segs: Sequence[Seg], device="cuda", lr_table: Optional[Sequence[float]] = None):
        import torch
        from scgaussian_amd import _lib
        self._lib, self._torch, self.device = _lib, torch, device
        self.segs = list(segs)
        assert 1 <= len(self.segs) <= _lib.ADAM_MAX_SEGMENTS
        assert all(len(s.g) <= STEPS_AHEAD for s in self.segs)             # the coefficient premise covers that many
        self.t = []
        for s in self.segs:
            d = dict(p=Carved(s.numel, s.off[0], SENTINELS["p"], device), m=Carved(s.numel, s.off[2], SENTINELS["m"], device),
                     v=Carved(s.numel, s.off[3], SENTINELS["v"], device), step=Carved(1, 0, SENTINELS["step"], device),
                     g=[Carved(s.numel, s.off[1], SENTINELS["g"], device) for _ in s.g])
            d["p"].write(s.p), d["m"].write(s.m), d["v"].write(s.v)
            d["step"].write(np.array([s.step], np.float32))
            for c, g in zip(d["g"], s.g):
                c.write(g)
            self.t.append(d)
        self.ws = Carved(WS_WORDS, 0, SENTINELS["ws"], device)
        self.ws.write(np.zeros(WS_WORDS, np.float32))
        assert _lib.load().scg_adam_workspace_bytes(len(self.segs)) == WS_WORDS * 4
        self.table = None
        if lr_table is not None:
            self.table = torch.tensor(list(lr_table) + [0.0] * (_lib.ADAM_MAX_SEGMENTS - len(lr_table)), dtype=torch.float64,
                                      device=device)
        torch.cuda.synchronize()

    def launch(self, k: int, force=False, use_table: bool = False) -> None:
        lib = self._lib
        arr = (lib.ScgAdamSegment * len(self.segs))()
        forces = force if isinstance(force, (list, tuple)) else [force] * len(self.segs)
        for a, s, d, f in zip(arr, self.segs, self.t, forces):
            a.param, a.grad, a.exp_avg, a.exp_avg_sq = d["p"].ptr(), d["g"][k].ptr(), d["m"].ptr(), d["v"].ptr()
            a.step = d["step"].ptr()
            a.numel, a.row_len, a.flags = s.numel, s.row_len, FORCE_FULL if (f and s.row_len) else 0
            a.lr, a.beta1, a.beta2, a.eps = s.lr, s.b1, s.b2, s.eps
        table = self.table.data_ptr() if use_table else None
        stream = self._torch.cuda.current_stream(self.device).cuda_stream
        lib.check(lib.load().scg_adam_step(arr, len(self.segs), table, self.ws.ptr(), WS_WORDS * 4, stream), "scg_adam_step")

    def vec(self, i: int, k: int = 0) -> bool:
        """What the host entry decides for segment i: all four tensors 16-byte aligned."""
        d = self.t[i]
        return all(c.ptr() % 16 == 0 for c in (d["p"], d["g"][k], d["m"], d["v"]))

    def write(self, i: int, name: str, a: np.ndarray) -> None:
        self.t[i][name].write(np.asarray(a, dtype=np.float32))

    def read(self):
        """([State per segment], workspace words as uint32) after a synchronisation."""
        self._torch.cuda.synchronize()
        ws = self.ws.read(np.uint32)
        st = [State(d["p"].read(), d["m"].read(), d["v"].read(), d["step"].read()[0], int(ws[WS_LIVE + i]))
              for i, d in enumerate(self.t)]
        return st, ws

    def sentinels_intact(self) -> bool:
        self._torch.cuda.synchronize()
        return self.ws.intact() and all(d[n].intact() for d in self.t for n in ("p", "m", "v", "step")) and \
            all(c.intact() for d in self.t for c in d["g"])


def assert_state_bits(got: Sequence[State], want: Sequence[State], what: str) -> None:
    for i, (a, b) in enumerate(zip(got, want)):
        for n in ("m", "v", "p"):
            x, y = getattr(a, n), getattr(b, n)
            nd = differing(x, y)
            if nd:
                j = int(np.nonzero(cbits(x) != cbits(y))[0][0])
                raise AssertionError(f"{what}: segment {i} {n}: {nd} of {x.size} elements differ in bits, first at {j}: "
                                     f"got {x[j]!r} ({bits(x)[j]:#010x}) want {y[j]!r} ({bits(y)[j]:#010x})")
        assert bits(np.array([a.step]))[0] == bits(np.array([b.step]))[0], (what, i, "step", a.step, b.step)


def coefficient_pairs_explaining(prev: State, seg: Seg, g, lr: float, got_p) -> list:
    """If p alone differs from the restatement: the (ulps of bc2s, ulps of nss) moves, each in -1..1, under which the restatement
    gives got_p in every element.  One pair: the device's double pow rounds differently from the host's.  None: the divide or the
    root is not IEEE."""
    bc2s, nss = bias_coefs(prev.step, lr, seg.b1, seg.b2)
    move = lambda x, d: x if d == 0 else np.nextafter(x, F(np.inf) if d > 0 else F(-np.inf))          # noqa: E731
    out = []
    for da in (-1, 0, 1):
        for db in (-1, 0, 1):
            p, _m, _v = adam_step_ref(prev.p, prev.m, prev.v, g, prev.step, lr, seg.b1, seg.b2, seg.eps,
                                      coefs=(move(bc2s, da), move(nss, db)))
            if same_bits(p, got_p):
                out.append((da, db))
    return out


def assert_workspace(ws: np.ndarray, lives: dict, what: str) -> None:
    """Ticket zero, live_next zero, live[slot] as given for the row slots, every other word zero."""
    want = np.zeros(WS_WORDS, np.uint32)
    for slot, w in lives.items():
        want[WS_LIVE + slot] = w
    assert np.array_equal(ws, want), (what, "workspace", {int(i): (int(ws[i]), int(want[i])) for i in np.nonzero(ws != want)[0]})

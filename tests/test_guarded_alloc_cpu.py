"""The teeth of tests/guarded_alloc.py, on CPU tensors: a stand-in "kernel" written in torch writes or reads through a raw, larger
view of the same storage, and the helper has to say where; and stand-in "entries" that read a scratch word nobody wrote, leave an
output's tail unwritten or index through an unwritten word give different results under the two fills, because the body of an
empty / empty_like request starts from the fill.  tests/test_gpu_guard_bands.py relies on every property held here."""
import ctypes as C
import math

import pytest
import torch

import guarded_alloc as G
from guarded_alloc import FILL_A, FILL_B, guarded, traced

CPU = ("cpu",)
DTYPES = [torch.float32, torch.float16, torch.float64, torch.uint8, torch.int8, torch.int16, torch.int32, torch.int64]
OTHER = {FILL_A: FILL_B, FILL_B: FILL_A}

# name -> a call that makes a 1-D tensor of n elements of the dtype
MAKERS = {
    "empty": lambda n, dt: torch.empty(n, dtype=dt),
    "zeros": lambda n, dt: torch.zeros((n,), dtype=dt),
    "full": lambda n, dt: torch.full((n,), 3, dtype=dt),
    "ones": lambda n, dt: torch.ones(n, dtype=dt),
    "empty_like": lambda n, dt: torch.empty_like(G._REAL["empty"](n, dtype=dt)),
    "zeros_like": lambda n, dt: torch.zeros_like(G._REAL["empty"](n, dtype=dt)),
    "full_like": lambda n, dt: torch.full_like(G._REAL["empty"](n, dtype=dt), 3),
    "ones_like": lambda n, dt: torch.ones_like(G._REAL["empty"](n, dtype=dt)),
    "tensor": lambda n, dt: torch.tensor([5] * n, dtype=dt),
    "arange": lambda n, dt: torch.arange(n, dtype=dt),
}


def raw_view(t, first, count):
    """`count` elements of t's storage from element `first` of t (negative: before its start): what a kernel's pointer reaches."""
    return torch.as_strided(t, (count,), (1,), t.storage_offset() + first)


def value_unlike(dtype, fill):
    """A value whose bytes differ from the band's under `fill` in the element's first byte."""
    return 77 if dtype not in (torch.float16, torch.float32, torch.float64) else 77.5


def test_every_patched_name_is_covered_here():
    assert set(MAKERS) == set(G.PATCHED) and len(G.PATCHED) == 10


@pytest.mark.parametrize("fill", [FILL_A, FILL_B])
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("name", sorted(MAKERS))
def test_one_element_past_the_end(name, dtype, fill):
    with guarded(fill, CPU) as reg:
        t = MAKERS[name](5, dtype)
        assert t.dtype == dtype and t.shape == (5,) and reg.covers(t.data_ptr())
        assert reg.check() == []
        raw_view(t, 5, 1)[0] = value_unlike(dtype, fill)
    (hit,) = reg.check()
    assert (hit.side, hit.dtype, hit.shape) == ("back", dtype, (5,))
    assert 0 <= hit.offset < dtype.itemsize                      # inside the first element past the end
    assert hit.found == value_unlike(dtype, fill)
    assert hit.module == __name__ and hit.line > 0


@pytest.mark.parametrize("fill", [FILL_A, FILL_B])
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("name", sorted(MAKERS))
def test_one_element_before_the_start(name, dtype, fill):
    with guarded(fill, CPU) as reg:
        t = MAKERS[name](5, dtype)
        raw_view(t, -1, 1)[0] = value_unlike(dtype, fill)
    (hit,) = reg.check()
    assert hit.side == "front" and -dtype.itemsize <= hit.offset < 0 and hit.found == value_unlike(dtype, fill)


@pytest.mark.parametrize("fill", [FILL_A, FILL_B])
@pytest.mark.parametrize("dtype", [torch.float32, torch.uint8, torch.int32], ids=str)
@pytest.mark.parametrize("name", sorted(MAKERS))
def test_zero_sized_body(name, dtype, fill):
    with guarded(fill, CPU) as reg:
        t = MAKERS[name](0, dtype)
        assert t.numel() == 0 and reg.check() == []              # (torch reports the address of an empty tensor as 0)
        raw_view(t, 0, 1)[0] = value_unlike(dtype, fill)
    (hit,) = reg.check()
    assert hit.side == "back" and 0 <= hit.offset < dtype.itemsize and hit.shape == (0,)


def test_a_far_write_is_found_at_its_offset():
    with guarded(FILL_A, CPU) as reg:
        t = torch.empty(3, dtype=torch.uint8)
        raw_view(t, 3 + 4095, 1)[0] = 0                          # the last byte of the back band
        u = torch.empty(7, dtype=torch.float32)
        raw_view(u, -1024, 1)[0] = 1.0                           # the first element of the front band
    hits = {h.shape: h for h in reg.check()}
    assert hits[(3,)].offset == 4095 and hits[(3,)].side == "back"
    assert hits[(7,)].offset in range(-4096, -4092) and hits[(7,)].side == "front"


@pytest.mark.parametrize("dtype", [torch.float32, torch.uint8, torch.int32, torch.int64], ids=str)
@pytest.mark.parametrize("fill", [FILL_A, FILL_B])
def test_a_write_of_one_fill_is_caught_under_the_other(dtype, fill):
    """A stray store of exactly the band's value is invisible under that fill; the second fill is why it cannot hide."""
    results = {}
    for run in (fill, OTHER[fill]):
        with guarded(run, CPU) as reg:
            t = torch.empty(4, dtype=dtype)
            stray = G.band_bytes(dtype, fill)[:dtype.itemsize].view(dtype)      # one element of the bytes of `fill`
            raw_view(t, 4, 1).copy_(stray)
        results[run] = reg.check()
    assert results[fill] == []
    (hit,) = results[OTHER[fill]]
    assert hit.side == "back" and 0 <= hit.offset < dtype.itemsize


@pytest.mark.parametrize("dtype", [torch.float32, torch.uint8, torch.int32], ids=str)
def test_a_read_past_an_input_differs_between_the_fills(dtype):
    def kernel(x):                                               # sums one element more than it was given
        return raw_view(x, 0, x.numel() + 1).to(torch.float64).sum()

    def honest(x):
        return raw_view(x, 0, x.numel()).to(torch.float64).sum()

    got, clean = {}, {}
    for fill in (FILL_A, FILL_B):
        with guarded(fill, CPU) as reg:
            x = torch.tensor([1, 2, 3], dtype=dtype)
            got[fill], clean[fill] = kernel(x), honest(x)
        assert reg.check() == []                                 # a read touches no band: only the A/B comparison sees it
    assert clean[FILL_A].equal(clean[FILL_B])
    assert not got[FILL_A].equal(got[FILL_B])


def test_a_wide_integer_band_holds_small_valid_indices():
    for fill, value in ((FILL_A, 1), (FILL_B, 2)):
        with guarded(fill, CPU):
            for dtype in (torch.int16, torch.int32, torch.int64):
                t = torch.empty(3, dtype=dtype)
                assert raw_view(t, 3, 4).tolist() == [value] * 4 and raw_view(t, -4, 4).tolist() == [value] * 4
    with guarded(FILL_A, CPU):
        assert raw_view(torch.empty(2, dtype=torch.float32), 2, 1).isnan().all()
        assert raw_view(torch.empty(2, dtype=torch.uint8), 2, 1).item() == 0xFF
    with guarded(FILL_B, CPU):
        assert abs(raw_view(torch.empty(2, dtype=torch.float32), 2, 1).item() - 0.0115) < 1e-4
        assert raw_view(torch.empty(2, dtype=torch.int8), -1, 1).item() == 0x3C


def test_a_clean_run_reports_nothing():
    with guarded(FILL_A, CPU) as reg:
        ts = [MAKERS[n](9, dt) for n in MAKERS for dt in DTYPES]
        for t in ts:
            t.fill_(1)                                           # every element of the body, none outside
        ts[0][:] = float("nan")
    assert reg.check() == [] and len(reg.allocations) == len(ts)


def test_names_are_restored_also_after_an_exception():
    before = {n: getattr(torch, n) for n in G.PATCHED}
    with pytest.raises(ZeroDivisionError):
        with guarded(FILL_A, CPU):
            assert all(getattr(torch, n) is not before[n] for n in G.PATCHED)
            1 / 0
    assert all(getattr(torch, n) is before[n] for n in G.PATCHED)
    with guarded(FILL_B, CPU):
        pass
    assert all(getattr(torch, n) is before[n] for n in G.PATCHED)
    with pytest.raises(ValueError):
        with guarded("C"):
            pass


def test_other_devices_and_pinned_requests_pass_through():
    with guarded(FILL_A) as reg:                                 # the default guards GPU tensors only
        t = torch.empty(4)
        u = torch.zeros_like(t)
        v = torch.tensor([1.0])
    assert reg.allocations == [] and not reg.covers(t.data_ptr()) and u.tolist() == [0] * 4 and v.item() == 1
    with guarded(FILL_A, CPU) as reg:
        out = G._REAL["empty"](3)
        assert torch.zeros(3, out=out) is out and reg.allocations == []


def test_bodies_hold_what_was_asked():
    with guarded(FILL_A, CPU) as reg:
        assert torch.zeros(3, 4).tolist() == [[0.0] * 4] * 3
        assert torch.zeros((2, 0, 3), dtype=torch.int32).shape == (2, 0, 3)
        assert torch.full((5,), 2.5).tolist() == [2.5] * 5
        assert torch.full((2, 2), 7).dtype == torch.int64 and torch.full((2, 2), 7).tolist() == [[7, 7], [7, 7]]
        assert torch.full([3], fill_value=-1, dtype=torch.int32).tolist() == [-1] * 3
        assert torch.ones(2, 3, dtype=torch.uint8).tolist() == [[1] * 3] * 2
        src = G._REAL["empty"](4, 6, dtype=torch.float16).t()
        for t in (torch.empty_like(src), torch.zeros_like(src), torch.ones_like(src), torch.full_like(src, 3)):
            assert (t.shape, t.stride(), t.dtype) == (src.shape, src.stride(), src.dtype)      # preserve_format, as unpatched
        assert torch.zeros_like(src).eq(0).all() and torch.full_like(src, 3).eq(3).all() and torch.ones_like(src).eq(1).all()
        assert torch.zeros_like(src, dtype=torch.int32).dtype == torch.int32
        assert torch.tensor([[1, 2], [3, 4]], dtype=torch.int32).tolist() == [[1, 2], [3, 4]]
        assert torch.tensor(3.5).shape == () and torch.tensor(3.5).item() == 3.5
        assert torch.arange(2, 11, 3).tolist() == [2, 5, 8] and torch.arange(4, dtype=torch.float32).dtype == torch.float32
        assert torch.empty(3, requires_grad=True).requires_grad and torch.empty((3, 2)).shape == (3, 2)
        assert torch.empty(torch.Size([2, 5]), dtype=torch.float64).shape == (2, 5)
    assert reg.check() == []


@pytest.mark.parametrize("nbytes", [0, 1, 3, 17, 255, 4097])
def test_views_keep_the_alignment_of_an_unpatched_allocation(nbytes):
    """The caching allocator hands out device memory at multiples of 512 bytes; a body starts at one too, whatever the sizes of the
    bodies before it, so every alignment the libraries ask for (16, 64, 256) holds as it does without the guard."""
    with guarded(FILL_A, CPU) as reg:
        for make in (lambda: torch.empty(nbytes, dtype=torch.uint8), lambda: torch.zeros(nbytes, dtype=torch.uint8),
                     lambda: torch.tensor([0] * nbytes, dtype=torch.uint8), lambda: torch.empty((nbytes, 3), dtype=torch.float32)):
            t = make()
            if t.numel():                                        # (torch reports the address of an empty tensor as 0)
                assert all(t.data_ptr() % a == 0 for a in (16, 64, 256, G.ALIGN))
        assert all(a.ptr % G.ALIGN == 0 for a in reg.allocations) and G.BAND % 256 == 0 and G.ALIGN % 256 == 0
    assert reg.check() == []


def test_rehome_moves_tensors_made_by_other_means():
    with guarded(FILL_A, CPU) as reg:
        x = torch.randn(3, 4).t().requires_grad_()
        tree = reg.rehome({"x": x, "l": [torch.randint(5, (3,)), 7], "t": (None, "s")})
        assert reg.covers(tree["x"].data_ptr()) and tree["x"].requires_grad and tree["x"].stride() == x.stride()
        assert tree["x"].equal(x) and reg.covers(tree["l"][0].data_ptr()) and tree["l"][1] == 7 and tree["t"] == (None, "s")
        assert reg.rehome(tree["x"]) is tree["x"]                # already inside a body
        sparse_rows = torch.randn(6, 4)[::2]                     # not dense: a dense copy
        assert reg.rehome(sparse_rows).equal(sparse_rows) and reg.rehome(sparse_rows).is_contiguous()
        # a model and its optimizer share their parameters, and the optimizer's state is keyed by them: still so afterwards
        p = torch.nn.Parameter(torch.randn(4))
        opt = torch.optim.Adam([p], lr=0.1)
        p.grad = torch.ones(4)
        opt.step()
        holder = type("Holder", (), {})()
        holder.p, holder.opt, holder.twice = p, opt, [p, p.grad]
        reg.rehome(holder)
        q = holder.p
        assert q is not p and isinstance(q, torch.nn.Parameter) and q.requires_grad and q.equal(p) and reg.covers(q.data_ptr())
        assert holder.opt.param_groups[0]["params"][0] is q and holder.twice[0] is q and list(holder.opt.state) == [q]
        assert all(reg.covers(holder.opt.state[q][k].data_ptr()) for k in ("exp_avg", "exp_avg_sq"))
    assert reg.check() == []


# ---- poison: the body of an empty / empty_like request starts from the fill

ALL_DTYPES = DTYPES + [torch.bool, torch.bfloat16]


def poison_of(dtype, fill, n):
    """The n elements a poisoned body of `dtype` holds under `fill`, built here from the rule's own words."""
    if dtype == torch.bool:
        return torch.tensor([fill == FILL_A] * n, dtype=torch.bool)
    if dtype in (torch.int16, torch.int32, torch.int64):
        return torch.tensor([{FILL_A: 1, FILL_B: 2}[fill]] * n, dtype=dtype)
    byte = {FILL_A: 0xFF, FILL_B: 0x3C}[fill]
    return torch.tensor([byte] * (n * dtype.itemsize), dtype=torch.uint8).view(dtype)


@pytest.mark.parametrize("fill", [FILL_A, FILL_B])
@pytest.mark.parametrize("dtype", ALL_DTYPES, ids=str)
def test_an_empty_body_reads_back_as_the_fill(dtype, fill):
    with guarded(fill, CPU) as reg:
        src = G._REAL["zeros"](4, 6, dtype=dtype).t()              # (empty_like keeps the transposed strides)
        made = [torch.empty(7, dtype=dtype), torch.empty((3, 5), dtype=dtype), torch.empty_like(src),
                torch.empty_like(G._REAL["zeros"](9), dtype=dtype), torch.empty(0, dtype=dtype)]
        for t in made:
            assert reg.covers(t.data_ptr()) or t.numel() == 0
            assert G.same_bits(t.contiguous().reshape(-1), poison_of(dtype, fill, t.numel())), (dtype, fill, t.shape)
        assert made[2].stride() == src.stride()
        # what was asked for is what the body holds, and a rehomed tensor is its source: none of them is poisoned
        three = 1 if dtype == torch.bool else 3
        assert torch.zeros(7, dtype=dtype).eq(0).all() and torch.zeros_like(src).eq(0).all()
        assert torch.ones(7, dtype=dtype).eq(1).all() and torch.full((7,), three, dtype=dtype).eq(three).all()
        assert torch.ones_like(src).eq(1).all() and torch.full_like(src, three).eq(three).all()
        assert torch.tensor([0, 1, 0], dtype=dtype).tolist() == [0, 1, 0] and torch.arange(3).tolist() == [0, 1, 2]
        moved = reg.rehome(G._REAL["zeros"](5, dtype=dtype))
        assert reg.covers(moved.data_ptr()) and moved.eq(0).all() and reg.like(src).shape == src.shape
    assert reg.check() == []                                     # the poison stops where the body ends
    if dtype.is_floating_point and fill == FILL_A:
        assert made[0].isnan().all()                             # every floating format reads all-ones bytes as a NaN
    if dtype == torch.float32 and fill == FILL_B:
        assert ((made[0] - 0.0115).abs() < 1e-4).all()


def test_poison_off_leaves_bodies_alone(monkeypatch):
    marker = G._REAL["full"]((1 << 16,), 0x5A, dtype=torch.uint8)

    real = G._REAL["empty"]

    def recycled(*args, **kwargs):                               # the allocator's leftovers, made visible: every raw buffer is 0x5A
        if str(kwargs.get("device")) == "meta":                     # (the patched names ask a meta tensor for the shape and strides)
            return real(*args, **kwargs)
        assert kwargs["dtype"] == torch.uint8
        return marker[:args[0]].clone()
    monkeypatch.setitem(G._REAL, "empty", recycled)
    for fill in (FILL_A, FILL_B):
        with guarded(fill, CPU, poison=False) as reg:
            assert not reg.poison
            for dtype in (torch.float32, torch.uint8, torch.int32):
                for t in (torch.empty(6, dtype=dtype), torch.empty_like(G._REAL["zeros"](6, dtype=dtype))):
                    assert t.view(torch.uint8).eq(0x5A).all() and reg.covers(t.data_ptr())
            assert torch.zeros(3).eq(0).all()
        assert reg.check() == []                                 # (the bands are filled as ever)
        with guarded(fill, CPU) as reg:
            assert reg.poison and not torch.empty(6, dtype=torch.uint8).eq(0x5A).any()


@pytest.mark.parametrize("fill", [FILL_A, FILL_B])
def test_a_pinned_empty_is_poisoned_and_lies_in_no_body(fill, monkeypatch):
    """Pinned memory needs a GPU runtime, so the unpatched names are stood in for here by ones that accept pin_memory and hand out
    ordinary host memory holding a marker: the patched name has to pass the request through (no body, no bands) and fill it."""
    asked = []

    def stand_in(real):
        def fn(*args, **kwargs):
            asked.append(bool(kwargs.pop("pin_memory", False)))
            return real(*args, **kwargs).view(torch.uint8).fill_(0x5A).view(kwargs.get("dtype") or torch.float32) if asked[-1] \
                else real(*args, **kwargs)
        return fn
    monkeypatch.setitem(G._REAL, "empty", stand_in(G._REAL["empty"]))
    monkeypatch.setitem(G._REAL, "empty_like", stand_in(G._REAL["empty_like"]))
    monkeypatch.setitem(G._REAL, "zeros", stand_in(G._REAL["zeros"]))
    for devices in (CPU, ("cuda",)):                             # a host buffer: poisoned whichever device type is guarded
        del asked[:]
        with guarded(fill, devices) as reg:
            before = len(reg.allocations)
            made = [torch.empty(9, dtype=torch.uint8, pin_memory=True), torch.empty((3, 2), dtype=torch.int32, pin_memory=True),
                    torch.empty(4, dtype=torch.float32, pin_memory=True),
                    torch.empty_like(G._REAL["zeros"](5, dtype=torch.float32), pin_memory=True)]
            kept = torch.zeros(4, dtype=torch.uint8, pin_memory=True)
            assert len(reg.allocations) == before and not any(reg.covers(t.data_ptr()) for t in made)
        assert sum(asked) == 5                                   # every pinned request reached the unpatched name as a pinned one
        for t in made:
            assert G.same_bits(t.reshape(-1), poison_of(t.dtype, fill, t.numel())), (t.dtype, fill)
        assert kept.eq(0x5A).all()                               # not an `empty`: passed through as it came
        with guarded(fill, devices, poison=False):
            assert torch.empty(9, dtype=torch.uint8, pin_memory=True).eq(0x5A).all()


# Three toy "entries" in plain torch, each with one of the faults the poison is for; `scratch` and `out` come from torch.empty, as in
# the bindings.  tests/test_gpu_guard_bands.py compares its runs with G.same_bits, the comparison used here.

def _sums_a_scratch_it_never_wrote(x):
    scratch = torch.empty(4, dtype=torch.float32)
    scratch[:2] = x[:2]                                          # two of the four partial sums are written ...
    return dict(total=scratch.sum())                             # ... and four are read


def _leaves_an_output_tail_unwritten(x):
    out = torch.empty_like(x)
    out[:-1] = x[:-1] * 2                                        # the "nothing to do" path forgets the last element
    return dict(out=out)


def _gathers_through_an_unwritten_index(x):
    index = torch.empty(3, dtype=torch.int32)
    index[:2] = torch.tensor([0, 3], dtype=torch.int32)          # the third word is whatever was there: 1 or 2, inside the table
    return dict(picked=x[index.long()])


def _honest(x):
    scratch, out = torch.empty(4, dtype=torch.float32), torch.empty_like(x)
    scratch[:] = x[:4]
    out[:] = x * 2
    return dict(total=scratch.sum(), out=out)


@pytest.mark.parametrize("entry", [_sums_a_scratch_it_never_wrote, _leaves_an_output_tail_unwritten,
                                   _gathers_through_an_unwritten_index], ids=lambda f: f.__name__.strip("_"))
def test_a_dependence_on_unwritten_memory_differs_between_the_fills(entry):
    x = torch.tensor([1.0, 2.0, 3.0, 4.0, 5.0])
    runs = {}
    for fill in (FILL_A, FILL_B):
        with guarded(fill, CPU) as reg:
            runs[fill] = entry(reg.rehome(x.clone()))
        assert reg.check() == []                                 # nothing outside a body was touched: only the A/B comparison sees it
    assert not G.same_bits(runs[FILL_A], runs[FILL_B])
    if entry is _gathers_through_an_unwritten_index:             # the fills are valid indices: the read stayed inside its table
        assert runs[FILL_A]["picked"].tolist() == [1.0, 4.0, 2.0] and runs[FILL_B]["picked"].tolist() == [1.0, 4.0, 3.0]
    if entry is _sums_a_scratch_it_never_wrote:
        assert math.isnan(float(runs[FILL_A]["total"])) and abs(float(runs[FILL_B]["total"]) - (3 + 2 * 0.0115)) < 1e-3
    off = {}
    for fill in (FILL_A, FILL_B):                                # without the poison both runs start from the same bytes: nothing shows
        with guarded(fill, CPU, poison=False) as reg:
            reg.allocate = _from_zeros(reg.allocate)
            off[fill] = entry(reg.rehome(x.clone()))
    assert G.same_bits(off[FILL_A], off[FILL_B])


def _from_zeros(allocate):
    """Registry.allocate with the body cleared: a recycled block that happens to hold zeros, the case that hides these faults."""
    def fn(*args, **kwargs):
        return allocate(*args, **kwargs).zero_()
    return fn


def test_an_entry_that_writes_what_it_reads_is_the_same_under_both_fills():
    x = torch.tensor([1.0, 2.0, 3.0, 4.0, 5.0])
    runs = {}
    for fill in (FILL_A, FILL_B):
        with guarded(fill, CPU) as reg:
            runs[fill] = _honest(reg.rehome(x.clone()))
    assert G.same_bits(runs[FILL_A], runs[FILL_B]) and float(runs[FILL_A]["total"]) == 10.0


def test_same_bits_tells_what_equality_does_not():
    nan, t = float("nan"), torch.tensor
    assert G.same_bits(nan, nan) and G.same_bits(t([nan, 1.0]), t([nan, 1.0])) and G.same_bits({"a": [t([1]), b"x"]}, {"a": [t([1]), b"x"]})
    assert not G.same_bits(t([0.0]), t([-0.0])) and not G.same_bits(t([1]), t([1], dtype=torch.int32))
    assert not G.same_bits(t([1.0, 2.0]), t([[1.0, 2.0]])) and not G.same_bits({"a": 1}, {"b": 1}) and not G.same_bits([1], [1, 2])
    assert not G.same_bits(b"ab", b"ac") and not G.same_bits(t([nan]), t([1.0]))


# ---- traced()

class Inner(C.Structure):
    _fields_ = [("n", C.c_int32), ("p", C.c_void_p), ("q", C.c_void_p)]


class Outer(C.Structure):
    _fields_ = [("count", C.c_int32), ("a", Inner), ("b", Inner), ("r", C.c_void_p), ("events", C.c_void_p * 2), ("pair", Inner * 2),
                ("link", C.POINTER(Inner)), ("x", C.c_double)]


class FakeFunction:
    def __init__(self, argtypes, result=0):
        self.argtypes, self.result, self.seen = argtypes, result, []

    def __call__(self, *args):
        self.seen.append(args)
        return self.result


class FakeLibrary:
    def __init__(self):
        P = C.c_void_p
        self.plain = FakeFunction([P, C.c_int32, P, C.c_size_t, P], 7)
        self.structs = FakeFunction([C.POINTER(Outer), P])
        self.table = FakeFunction([C.POINTER(Inner), C.c_int32, P])
        self.words = FakeFunction([C.POINTER(C.c_int32), P])
        self.untyped = lambda: "free"


def test_traced_finds_plain_pointers():
    lib = traced(FakeLibrary())
    assert lib.plain(0x1000, 5, None, 64, C.c_void_p(0x2000)) == 7
    assert lib.untyped() == "free"
    (call,) = lib.calls
    assert call.name == "plain" and call.pointers == [((0,), 0x1000), ((2,), None), ((4,), 0x2000)]
    assert lib._lib.plain.seen == [(0x1000, 5, None, 64, lib._lib.plain.seen[0][4])]       # forwarded unchanged


def test_traced_finds_pointers_in_byref_nested_and_linked_structures():
    lib = traced(FakeLibrary())
    linked = Inner(1, 0x70, None)
    o = Outer(count=2, a=Inner(3, 0x10, 0x20), b=Inner(0, None, 0x30), r=0x40, x=1.5, link=C.pointer(linked))
    o.events[1] = 0x50
    o.pair[1].p = 0x60
    for arg in (C.byref(o), C.pointer(o), o):
        lib.calls.clear()
        lib.structs(arg, 0x99)
        found = dict(lib.calls[0].pointers)
        assert found == {(0, "a", "p"): 0x10, (0, "a", "q"): 0x20, (0, "b", "p"): None, (0, "b", "q"): 0x30, (0, "r"): 0x40,
                         (0, "events", 0): None, (0, "events", 1): 0x50, (0, "pair", 0, "p"): None, (0, "pair", 0, "q"): None,
                         (0, "pair", 1, "p"): 0x60, (0, "pair", 1, "q"): None, (0, "link", "p"): 0x70, (0, "link", "q"): None,
                         (1,): 0x99}
    lib.calls.clear()
    lib.structs(None, None)                                      # a NULL struct has no fields to record
    assert lib.calls[0].pointers == [((1,), None)]


def test_traced_finds_pointers_in_arrays_of_structures():
    lib = traced(FakeLibrary())
    table = (Inner * 3)()
    table[0].p, table[2].q = 0x11, 0x22
    lib.table(table, 3, 0x33)
    found = dict(lib.calls[0].pointers)
    assert found[(0, 0, "p")] == 0x11 and found[(0, 2, "q")] == 0x22 and found[(0, 1, "p")] is None and found[(2,)] == 0x33
    assert len(found) == 7
    words = (C.c_int32 * 2)(1, 2)
    lib.words(words, 0x44)                                       # a pointer to host integers is no pointer-typed argument
    assert lib.calls[1].pointers == [((1,), 0x44)]


def test_traced_handles_share_one_list():
    calls = []
    a, b = traced(FakeLibrary(), calls), traced(FakeLibrary(), calls)
    a.plain(1, 0, 2, 0, 3)
    b.words(None, 4)
    assert [c.name for c in calls] == ["plain", "words"] and a.calls is b.calls

"""Guard bands around the tensors the binding allocates, and a recorder of the pointers it hands to the libraries.

The caching allocator rounds every allocation up and carves it from large blocks, so a kernel that writes or reads a few bytes past
a buffer never faults and never changes a value a parity test looks at.  This helper makes such an access visible without a
sanitizer:

    with guarded(FILL_A) as reg:          # torch.empty / zeros / full / ones, their *_like forms, torch.tensor and torch.arange
        x = reg.rehome(inputs)            # hand out views of [4096-byte band | body | 4096-byte band]; rehome() moves tensors
        out = entry(x)                    # that were made by other means (torch.randn, .to(device), ...) into such buffers
    assert reg.check() == []              # every band still holds its fill, bit for bit
    assert reg.covers(out.data_ptr())

    lib = traced(real_lib)                # a stand-in for a ctypes library handle: lib.calls lists, per call, the function's
                                          # name and every pointer-typed argument and struct field that was passed

What traced() does not see: a struct field that POINTS to a struct is followed to its first record only (the walker knows no count),
and an address kept in an integer field or in a table behind a plain pointer (the per-image `src` words of the PNG image table, the
records of a segment table) is not a pointer-typed argument and is not recorded.

Two fills (FILL_A, FILL_B) exist so that a stray write of a value that happens to equal one fill is caught under the other, and so
that a result which depends on bytes outside its inputs differs between the two runs.  The fills of wider integers are the small
valid indices 1 and 2: a kernel that reads an index one element too far is not steered to a wild address.

Poison.  The caching allocator recycles blocks, so the first bytes of a torch.empty / torch.empty_like request are whatever was there
last — usually zeros or the previous call's values, which is exactly what a kernel that reads a scratch word before anyone wrote it,
leaves part of an output unwritten or assumes that a counter starts at 0 needs in order to pass.  Under guarded(fill) — poison=True
is the default — the BODY of such a request starts from the same fill as its bands: every byte 0xFF (A) or 0x3C (B) for floating
and 8-bit types, the indices 1 (A) and 2 (B) for int16/32/64, and True (A) / False (B) for bool, whose bytes torch defines only as
0 and 1.  A result that depends on an unwritten word then differs between the A run and the B run.  zeros, ones, full, tensor and
arange hold what was asked for, and Registry.like / rehome are followed by a copy_: none of them is poisoned.  A pinned host
empty(..., pin_memory=True) stays unguarded (no bands, in no body) but gets the same fill: the wrappers fill such buffers with
device-to-host copies and then write them to files or upload them, and a byte the copy does not cover must not look written.
guarded(fill, poison=False) leaves every body as the allocator gave it.

Nothing here reads or changes the environment, the allocator's settings or how Python starts; the patched names are restored when the
context ends, also after an exception.
"""
import contextlib
import ctypes as C
import functools
import math
import sys
import types
from collections import namedtuple

import numpy as np
import torch

BAND = 4096                    # bytes of each band: a multiple of every alignment the libraries ask for (16, 64, 256)
ALIGN = 512                    # the body's alignment: what the caching allocator gives a device allocation
FILL_A, FILL_B = "A", "B"
_BYTE = {FILL_A: 0xFF, FILL_B: 0x3C}          # floating (0xFF..: a NaN; 0x3C..: about 0.0115) and 8-bit types
_WIDE = {FILL_A: 1, FILL_B: 2}                # int16 / int32 / int64

PLAIN = ("empty", "zeros", "full", "ones")
LIKE = ("empty_like", "zeros_like", "full_like", "ones_like")
DATA = ("tensor", "arange")
PATCHED = PLAIN + LIKE + DATA

_WIDE_INTS = (torch.int16, torch.int32, torch.int64)
_REAL = {n: getattr(torch, n) for n in PATCHED}          # the unpatched names, for the helper's own allocations

Touched = namedtuple("Touched", "module line dtype shape side offset found")
Touched.__doc__ = """A band that no longer holds its fill.  side: "front" or "back"; offset: bytes from the body to the first touched
byte (back: 0 is the first byte past the end; front: -1 is the byte just before the start); found: the element of the request's
dtype that holds that byte, as the band now reads."""

_FUNCTIONS = (types.FunctionType, types.MethodType, types.BuiltinFunctionType, functools.partial)      # rehome() leaves them alone

Call = namedtuple("Call", "name pointers")     # pointers: [(path, value)], path (argument index, field, field or index, ...)


def fill_class(dtype):
    return "wide" if dtype in _WIDE_INTS else "byte"


def fill_byte(fill):
    """The byte every floating and 8-bit band and poisoned body holds under `fill`."""
    return _BYTE[fill]


def poison_(t, fill):
    """Fill every byte the dense tensor `t` owns with the fill of its dtype, in place; returns t."""
    if t.numel() == 0:
        return t
    if t.dtype == torch.bool:
        return t.fill_(fill == FILL_A)
    if fill_class(t.dtype) == "wide":
        return t.fill_(_WIDE[fill])
    flat = torch.as_strided(t, (_span(t.shape, t.stride()),), (1,), t.storage_offset())      # complex, bfloat16, ...: bytes all the same
    flat.view(torch.uint8).fill_(_BYTE[fill])
    return t


def same_bits(a, b):
    """Whether two results (tensors, arrays, numbers, bytes, or dicts and lists of them) are equal bit for bit; two NaN floats are."""
    if isinstance(a, torch.Tensor):
        return isinstance(b, torch.Tensor) and a.shape == b.shape and a.dtype == b.dtype and \
            torch.equal(a.contiguous().reshape(-1).view(torch.uint8), b.contiguous().reshape(-1).view(torch.uint8))
    if isinstance(a, dict):
        return isinstance(b, dict) and a.keys() == b.keys() and all(same_bits(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return isinstance(b, (list, tuple)) and len(a) == len(b) and all(same_bits(x, y) for x, y in zip(a, b))
    if isinstance(a, float) and isinstance(b, float) and math.isnan(a) and math.isnan(b):
        return True
    if isinstance(a, np.ndarray):
        return isinstance(b, np.ndarray) and a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()
    return a == b


def band_bytes(dtype, fill, device="cpu"):
    """The BAND bytes a band of a request of `dtype` holds under `fill`."""
    if fill_class(dtype) == "wide":
        return _REAL["full"]((BAND // dtype.itemsize,), _WIDE[fill], dtype=dtype, device=device).view(torch.uint8)
    return _REAL["full"]((BAND,), _BYTE[fill], dtype=torch.uint8, device=device)


class _Allocation:
    __slots__ = ("raw", "start", "nbytes", "dtype", "shape", "module", "line", "ptr")

    def __init__(self, raw, start, nbytes, dtype, shape, module, line):
        self.raw, self.start, self.nbytes, self.dtype, self.shape = raw, start, nbytes, dtype, shape
        self.module, self.line = module, line
        self.ptr = raw.data_ptr() + start

    def band(self, side):
        lo = self.start - BAND if side == "front" else self.start + self.nbytes
        return self.raw[lo:lo + BAND]


def _span(shape, strides):
    """Elements of storage a tensor of this shape and these strides reaches."""
    if any(s == 0 for s in shape):
        return 0
    return 1 + sum((s - 1) * st for s, st in zip(shape, strides))


def _requester():
    """Module name and line of the nearest frame outside this file and outside torch."""
    f = sys._getframe(1)
    while f is not None:
        name = f.f_globals.get("__name__", "?")
        if f.f_code.co_filename != __file__ and name != "torch" and not name.startswith("torch."):
            return name, f.f_lineno
        f = f.f_back
    return "?", 0


class Registry:
    """Every raw buffer of one guarded() context, kept alive until the registry itself goes."""

    def __init__(self, fill, devices, poison=True):
        self.fill, self.devices, self.poison = fill, tuple(devices), bool(poison)
        self.allocations = []

    # ---- allocation
    def wants(self, device, kwargs=()):
        if kwargs and (kwargs.get("pin_memory") or kwargs.get("out") is not None or kwargs.get("names") is not None
                       or kwargs.get("layout") not in (None, torch.strided)):
            return False
        if device is None:
            device = torch.get_default_device() if hasattr(torch, "get_default_device") else "cpu"
        return torch.device(device).type in self.devices

    def allocate(self, shape, dtype, device, strides=None, undefined=False):
        """A tensor of this shape, dtype and (dense or overlapping-free) strides between two bands.  undefined: the request leaves
        the content to chance (empty, empty_like), so under poison the whole body starts from the fill; otherwise the caller writes
        every element next and the body is left as the allocator gave it."""
        shape = tuple(int(s) for s in shape)
        if strides is None:
            strides, acc = [], 1
            for s in reversed(shape):
                strides.append(acc)
                acc *= max(s, 1)
            strides = tuple(reversed(strides))
        nbytes = _span(shape, strides) * dtype.itemsize
        raw = _REAL["empty"](nbytes + 2 * BAND + ALIGN, dtype=torch.uint8, device=device)
        start = (-raw.data_ptr()) % ALIGN + BAND
        module, line = _requester()
        a = _Allocation(raw, start, nbytes, dtype, shape, module, line)
        fill = band_bytes(dtype, self.fill, raw.device)
        a.band("front").copy_(fill)
        a.band("back").copy_(fill)
        self.allocations.append(a)
        if undefined and self.poison:
            poison_(raw[start:start + nbytes].view(dtype), self.fill)
        body = raw[start:start + nbytes].view(dtype)
        return body.as_strided(shape, strides, body.storage_offset())

    def like(self, t):
        """An uninitialised guarded tensor with the shape, dtype, strides and device of `t`."""
        if _span(t.shape, t.stride()) > t.numel():                 # not dense: a dense one of the same shape
            return self.allocate(t.shape, t.dtype, t.device)
        return self.allocate(t.shape, t.dtype, t.device, t.stride())

    def rehome(self, obj, _memo=None):
        """`obj` with every tensor on a guarded device replaced by a guarded copy (same values, strides, requires_grad; a Parameter
        stays one).  Dicts (their tensor keys too), lists and the attributes of plain objects are rewritten IN PLACE, tuples (named
        ones too) rebuilt; a tensor met twice is moved once, so an optimizer and its model still share their parameters.  Tensors
        already in a body are kept."""
        memo = {} if _memo is None else _memo
        if id(obj) in memo:
            return memo[id(obj)][1]
        if isinstance(obj, torch.Tensor):
            new = obj
            if self.wants(obj.device) and obj.layout == torch.strided and not self.covers(obj.data_ptr()):
                new = self.like(obj)
                new.copy_(obj.detach())
                if isinstance(obj, torch.nn.Parameter):
                    new = torch.nn.Parameter(new, requires_grad=obj.requires_grad)
                else:
                    new.requires_grad_(obj.requires_grad)
            memo[id(obj)] = (obj, new)
            return new
        if obj is None or isinstance(obj, (str, bytes, int, float, bool, type, torch.nn.Module, torch.device, torch.dtype)):
            return obj
        if isinstance(obj, dict):
            memo[id(obj)] = (obj, obj)
            items = [(self.rehome(k, memo) if isinstance(k, torch.Tensor) else k, self.rehome(v, memo)) for k, v in obj.items()]
            if any(k is not k0 or v is not v0 for (k, v), (k0, v0) in zip(items, obj.items())):
                obj.clear()
                obj.update(items)
            return obj
        if isinstance(obj, list):
            memo[id(obj)] = (obj, obj)
            obj[:] = [self.rehome(v, memo) for v in obj]
            return obj
        if isinstance(obj, tuple):
            items = [self.rehome(v, memo) for v in obj]
            new = type(obj)(*items) if hasattr(obj, "_fields") else type(obj)(items)
            memo[id(obj)] = (obj, new)
            return new
        if hasattr(obj, "__dict__") and not isinstance(obj, _FUNCTIONS) and type(obj).__module__ not in ("builtins", "numpy", "ctypes"):
            memo[id(obj)] = (obj, obj)
            for k, v in list(vars(obj).items()):
                new = self.rehome(v, memo)
                if new is not v:
                    setattr(obj, k, new)
        return obj

    # ---- queries
    def covers(self, ptr):
        """Whether the address lies inside a guarded body (a zero-sized body covers its own address)."""
        if ptr is None:
            return False
        return any(a.ptr <= ptr < a.ptr + max(a.nbytes, 1) for a in self.allocations)

    def check(self):
        """The Touched records of every band that is not bit-for-bit intact (an empty list: nothing was written outside a body)."""
        groups = {}
        for a in self.allocations:
            for side in ("front", "back"):
                groups.setdefault((a.raw.device, a.dtype if fill_class(a.dtype) == "wide" else None), []).append((a, side))
        touched = []
        for (device, wide), members in groups.items():
            want = band_bytes(wide or torch.uint8, self.fill, device)
            for lo in range(0, len(members), 1024):
                part = members[lo:lo + 1024]
                bad = (torch.stack([a.band(side) for a, side in part]) != want[None]).any(1).cpu()
                for (a, side), is_bad in zip(part, bad.tolist()):
                    if is_bad:
                        touched.append(self._describe(a, side, want))
        return touched

    @staticmethod
    def _describe(a, side, want):
        band = a.band(side)
        first = int((band != want).nonzero()[0])
        elem = first - first % a.dtype.itemsize
        found = band[elem:elem + a.dtype.itemsize].clone().view(a.dtype).cpu()[0].item()
        return Touched(a.module, a.line, a.dtype, a.shape, side, first if side == "back" else first - BAND, found)


def _meta(kwargs):
    kw = {k: v for k, v in kwargs.items() if k != "requires_grad"}
    kw["device"] = "meta"
    return kw


def _make_patches(reg, orig):
    def finish(t, kwargs):
        return t.requires_grad_() if kwargs.get("requires_grad") else t

    def pinned(name, t, kwargs):
        """A pinned host empty / empty_like passes through unguarded whatever `devices` says, and is poisoned all the same."""
        if reg.poison and name in ("empty", "empty_like") and kwargs.get("pin_memory") and kwargs.get("out") is None \
                and isinstance(t, torch.Tensor) and t.layout == torch.strided and t.device.type == "cpu":
            poison_(t, reg.fill)
        return t

    def plain(name):
        def fn(*args, **kwargs):
            if not reg.wants(kwargs.get("device"), kwargs):
                return pinned(name, orig[name](*args, **kwargs), kwargs)
            m = orig[name](*args, **_meta(kwargs))
            t = reg.allocate(m.shape, m.dtype, kwargs.get("device") or _default_device(), m.stride(), undefined=name == "empty")
            if name == "zeros":
                t.zero_()
            elif name == "ones":
                t.fill_(1)
            elif name == "full":
                t.fill_(kwargs["fill_value"] if "fill_value" in kwargs else args[1])
            return finish(t, kwargs)
        return fn

    def like(name):
        def fn(*args, **kwargs):
            src = args[0] if args else kwargs["input"]
            device = kwargs.get("device")
            if not reg.wants(src.device if device is None else device, kwargs) or src.layout != torch.strided:
                return pinned(name, orig[name](*args, **kwargs), kwargs)
            m = orig[name](*args, **_meta(kwargs))
            t = reg.allocate(m.shape, m.dtype, src.device if device is None else device, m.stride(), undefined=name == "empty_like")
            if name == "zeros_like":
                t.zero_()
            elif name == "ones_like":
                t.fill_(1)
            elif name == "full_like":
                t.fill_(kwargs["fill_value"] if "fill_value" in kwargs else args[1])
            return finish(t, kwargs)
        return fn

    def data(name):
        def fn(*args, **kwargs):
            t = orig[name](*args, **kwargs)
            if not reg.wants(t.device, kwargs) or t.layout != torch.strided:
                return t
            new = reg.like(t)
            new.copy_(t.detach())
            return new.requires_grad_(t.requires_grad)
        return fn

    patches = {n: plain(n) for n in PLAIN}
    patches.update({n: like(n) for n in LIKE})
    patches.update({n: data(n) for n in DATA})
    return patches


def _default_device():
    return torch.get_default_device() if hasattr(torch, "get_default_device") else torch.device("cpu")


@contextlib.contextmanager
def guarded(fill, devices=("cuda",), poison=True):
    """Replace torch.<name> for every name in PATCHED while the context is active; yields the Registry.  Allocations on a device
    type outside `devices` (the default: GPU only), pinned ones and those with `out=` get no bands and lie in no body.  poison: the
    body of an empty / empty_like request, and a pinned host one, starts from the fill (the module's docstring)."""
    if fill not in (FILL_A, FILL_B):
        raise ValueError(f"fill is FILL_A or FILL_B, not {fill!r}")
    orig = {n: getattr(torch, n) for n in PATCHED}
    reg = Registry(fill, devices, poison)
    patches = _make_patches(reg, _REAL)
    try:
        for n in PATCHED:
            setattr(torch, n, patches[n])
        yield reg
    finally:
        for n in PATCHED:
            setattr(torch, n, orig[n])


# ---- traced(lib)

def _is_struct_ptr(t):
    return isinstance(t, type) and issubclass(t, C._Pointer) and isinstance(t._type_, type) and issubclass(t._type_, C.Structure)


def _walk_struct(obj, path, out):
    for field in obj._fields_:
        name, ftype = field[0], field[1]
        _walk_value(getattr(obj, name), ftype, path + (name,), out)


def _walk_value(value, ftype, path, out):
    """Record `value`, read from a struct field or array element of ctypes type `ftype`."""
    if ftype is C.c_void_p:
        out.append((path, value.value if isinstance(value, C.c_void_p) else value))
    elif isinstance(ftype, type) and issubclass(ftype, C.Structure):
        _walk_struct(value, path, out)
    elif isinstance(ftype, type) and issubclass(ftype, C.Array):
        inner = ftype._type_
        if inner is C.c_void_p or (isinstance(inner, type) and issubclass(inner, (C.Structure, C.Array))):
            for i in range(ftype._length_):
                _walk_value(value[i], inner, path + (i,), out)
    elif _is_struct_ptr(ftype) and value:                         # (the first record only: nothing here says how many follow)
        _walk_struct(value.contents, path, out)


def _walk_argument(arg, argtype, path, out):
    if argtype is C.c_void_p:
        if isinstance(arg, C.c_void_p):
            arg = arg.value
        elif isinstance(arg, C._Pointer):
            arg = C.cast(arg, C.c_void_p).value
        elif isinstance(arg, (C.Array, C.Structure)):
            arg = C.addressof(arg)
        elif hasattr(arg, "_obj"):                                  # byref(x)
            arg = C.addressof(arg._obj)
        out.append((path, arg))
    elif _is_struct_ptr(argtype) and arg is not None:
        target = arg._obj if hasattr(arg, "_obj") else arg           # byref(x) -> x
        if isinstance(target, C._Pointer):
            if not target:
                return
            target = target.contents
        if isinstance(target, C.Array):
            for i in range(len(target)):
                _walk_struct(target[i], path + (i,), out)
        elif isinstance(target, C.Structure):
            _walk_struct(target, path, out)


class Traced:
    """A stand-in for a ctypes library handle.  Every call through it is forwarded unchanged and appended to `calls`."""

    def __init__(self, lib, calls=None):
        self.__dict__["_lib"] = lib
        self.__dict__["calls"] = [] if calls is None else calls

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        argtypes = getattr(fn, "argtypes", None)
        if argtypes is None:
            return fn

        def call(*args):
            pointers = []
            for i, (arg, argtype) in enumerate(zip(args, argtypes)):
                _walk_argument(arg, argtype, (i,), pointers)
            self.calls.append(Call(name, pointers))
            return fn(*args)
        call.__name__ = name
        return call

    def __setattr__(self, name, value):
        setattr(self._lib, name, value)


def traced(lib, calls=None):
    """Wrap a loaded library handle (or anything whose attributes are functions with `argtypes`); `calls` may be a list shared by
    several handles."""
    return Traced(lib, calls)

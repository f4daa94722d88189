"""What png.py and jpeg.py share on the host: a batch of images of unequal sizes becomes a batch of files in three launches and two
host reads.  A format supplies its library, its record dtypes, its layout call and how it fills its Scg*Encode; everything that
depends only on "a table of records, a workspace, an output buffer and a table that says where each file lies" is here, once.
"""
from __future__ import annotations

import ctypes as C
from typing import List, Optional, Sequence

import numpy as np
import torch

from . import _lib


def hwc(shape, err) -> tuple:
    shape = tuple(int(s) for s in shape)
    if len(shape) == 2:
        shape = shape + (1,)
    if len(shape) != 3 or shape[2] not in (1, 3):
        raise err(f"an image is (H, W), (H, W, 1) or (H, W, 3), not {shape}")
    return shape


def takes(t) -> bool:
    """Is `t` an image the kernels take as it is?  (What they do not take goes to Pillow in save_png / save_jpeg.)"""
    return (isinstance(t, torch.Tensor) and t.device.type == "cuda" and t.dtype == torch.uint8 and t.is_contiguous() and
            (t.dim() == 2 or (t.dim() == 3 and t.shape[2] in (1, 3))) and t.numel() > 0)


class FilePlan:
    """Everything of a batch that depends on its shapes and options alone: the layout, the record tables on the device, the workspace
    and the output buffer.  encode() on it allocates nothing and reads nothing back, so it can be captured in a graph: `inputs` are
    the plan's own image tensors (views of one arena), to be rewritten in place between replays.

    A format sets LIB (its _lib_* module), WHAT (the prefix of its messages), ENTRY (its scg_*_encode), ENCODE (that call's struct),
    COLUMNS (the width of its table), PACKED (its PackedFiles) and defines _configure, _lay_out and _fill."""

    LIB = WHAT = ENTRY = ENCODE = COLUMNS = PACKED = None

    @classmethod
    def _err(cls, msg: str) -> _lib.ScgError:
        return _lib.ScgError(f"{cls.WHAT}: {msg}")

    def __init__(self, shapes: Sequence, device, own_inputs: bool, **options):
        self.device = torch.device(device)
        _lib.stream_of(self.device, type(self).__name__)
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self._configure(**options)
        self.shapes = [hwc(s, self._err) for s in shapes]
        # the format's layout call: its Scg*Layout, the image records, {attribute: the host table it names on the device}
        self.layout, self.images_host, tables = self._lay_out()
        self.inputs: List[torch.Tensor] = []
        self._src = None
        n = len(self.shapes)
        if n == 0:
            return
        with torch.cuda.device(self.device):
            for name, table in tables.items():                    # (an allocation and a copy: the plan of a retry owns its tables too)
                setattr(self, name, torch.empty(table.nbytes, dtype=torch.uint8, device=self.device))
                getattr(self, name).copy_(torch.from_numpy(table.view(np.uint8).reshape(-1)))
            self.images_dev = torch.empty(n * self.images_host.dtype.itemsize, dtype=torch.uint8, device=self.device)
            self.workspace = torch.empty(int(self.layout.workspace_bytes), dtype=torch.uint8, device=self.device)
            self.out = torch.empty(int(self.layout.capacity), dtype=torch.uint8, device=self.device)
            if own_inputs:
                sizes = [h * w * c for h, w, c in self.shapes]
                starts = np.concatenate([[0], np.cumsum([(s + 15) // 16 * 16 for s in sizes])])
                self.arena = torch.zeros(int(starts[-1]), dtype=torch.uint8, device=self.device)
                self.inputs = [self.arena[int(o):int(o) + s].view(shape) for o, s, shape in zip(starts, sizes, self.shapes)]
                self._bind(self.inputs)
        t = self.layout.table_offset
        self.table = self.workspace[t:t + self.layout.table_bytes].view(torch.int32)

    def _bind(self, images) -> None:
        """Put the images' addresses into the image table; upload it when they changed (a host-to-device copy, never a read)."""
        src = [int(t.data_ptr()) for t in images]
        if src == self._src:
            return
        if torch.cuda.is_current_stream_capturing():
            raise self._err(f"a captured call must use the tensors of the call before it ({type(self).__name__}.inputs): the image "
                            "table cannot be uploaded inside a capture")
        self.images_host["src"] = src
        self.images_dev.copy_(torch.from_numpy(self.images_host.view(np.uint8).reshape(-1).copy()))
        self._src = src

    def args(self):
        """The Scg*Encode of this plan."""
        a = self.ENCODE()
        a.struct_bytes = C.sizeof(self.ENCODE)
        a.images, a.images_host, a.images_dev = len(self.shapes), self.images_host.ctypes.data, self.images_dev.data_ptr()
        self._fill(a)
        return a

    @torch.no_grad()
    def encode(self, images: Optional[Sequence[torch.Tensor]] = None):
        """Three launches on the current stream.  images: None for the plan's own inputs, or tensors of the plan's shapes."""
        if not self.shapes:
            return self.PACKED(self)
        if images is None:
            images = self.inputs
            if not images:
                raise self._err("the plan has no inputs of its own (own_inputs=False): pass the images")
        images = list(images)
        if len(images) != len(self.shapes):
            raise self._err(f"{len(images)} images for a plan of {len(self.shapes)}")
        for i, (t, shape) in enumerate(zip(images, self.shapes)):
            if not isinstance(t, torch.Tensor) or t.device != self.device or t.dtype != torch.uint8 or not t.is_contiguous() or \
                    hwc(t.shape, self._err) != shape:
                raise self._err(f"image {i} must be a contiguous uint8 tensor of shape {shape} on {self.device}")
        stream = _lib.stream_of(self.out, self.WHAT)
        with torch.cuda.device(self.device):
            self._bind(images)
            a = self.args()
            self.LIB.check(getattr(self.LIB.load(), self.ENTRY)(C.byref(a), self.out.data_ptr(), self.out.numel(),
                                                                self.workspace.data_ptr(), self.workspace.numel(), stream), self.ENTRY)
        return self.PACKED(self, keep=images)


class PackedFiles:
    """The files of a batch in the plan's output buffer, each at a multiple of 16 bytes, and the table that says where: a row of
    plan.COLUMNS uint32 per image (offset, bytes, ...), then a row (total bytes, images, ...)."""

    def __init__(self, plan: FilePlan, keep=None):
        self.plan, self._keep = plan, keep
        self.table_host: Optional[np.ndarray] = None
        self.host: Optional[torch.Tensor] = None

    def __len__(self):
        return len(self.plan.shapes)

    def _read_table(self) -> bool:
        """The first host read, the table into pinned memory.  False: nothing is left to read (an empty batch, or both reads made)."""
        n, plan = len(self), self.plan
        if self.host is not None or n == 0:
            if n == 0 and self.table_host is None:
                self.table_host = np.zeros((1, plan.COLUMNS), dtype=np.uint32)
            return False
        table = torch.empty((n + 1, plan.COLUMNS), dtype=torch.int32, pin_memory=True)
        table.copy_(plan.table.view(n + 1, plan.COLUMNS), non_blocking=True)
        torch.cuda.current_stream(plan.device).synchronize()
        self.table_host = table.numpy().view(np.uint32)
        total = int(self.table_host[n, 0])
        if int(self.table_host[n, 1]) != n or total > plan.out.numel():
            raise plan._err(f"the table names {int(self.table_host[n, 1])} images and {total} bytes: not this batch's")
        return True

    def _read_files(self) -> None:
        """The second host read: exactly `total` bytes of the buffer into pinned memory."""
        total = int(self.table_host[len(self), 0])
        self.host = torch.empty(total, dtype=torch.uint8, pin_memory=True)
        self.host.copy_(self.plan.out[:total], non_blocking=True)
        torch.cuda.current_stream(self.plan.device).synchronize()

    def to_host(self):
        """The batch's TWO host reads: the table, then exactly `total` bytes of the buffer into pinned memory."""
        if self._read_table():
            self._read_files()
        return self

    def _paths(self, paths) -> list:
        paths = list(paths)
        if len(paths) != len(self):
            raise self.plan._err(f"{len(paths)} paths for {len(self)} images")
        return paths


def encode(images, plan_class, **options):
    """The batch's files on the device: three launches whatever the number of images and their sizes, no host read."""
    images = list(images)
    for i, t in enumerate(images):
        if not isinstance(t, torch.Tensor):
            raise plan_class._err(f"image {i} is not a tensor")
        _lib.stream_of(t, plan_class.WHAT)
        if not takes(t):
            raise plan_class._err(f"image {i} must be a contiguous, non-empty uint8 tensor shaped (H, W), (H, W, 1) or (H, W, 3); it is "
                                  f"{t.dtype} {tuple(t.shape)}")
    device = images[0].device if images else torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else None
    if device is None:
        raise plan_class._err("needs the ROCm GPU ('cuda'); there is no CPU path")
    return plan_class([t.shape for t in images], device, own_inputs=False, **options).encode(images)

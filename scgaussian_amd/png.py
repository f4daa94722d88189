"""PNG files from uint8 device tensors, host side (libscg_png.so, include/png/scg_png.h states the stream).

    packed = png.encode([img0, img1, ...])        three launches for the whole batch, no host read
    packed.to_host()                              TWO host reads: the table, then exactly `total` bytes into pinned memory
    packed.files() / packed.write(paths)          the complete files: the host adds the 41 leading bytes, the IDAT's CRC-32 and IEND
    plan = png.PngPlan(shapes, device)            the uploaded tables and the buffers, for repeated and captured calls
    png.save_png(path, tensor)                    one image; what the kernels do not take goes to Pillow, as before

An image is a contiguous uint8 tensor on the GPU shaped (H, W), (H, W, 1) or (H, W, 3).  One channel is written as three equal
ones by default (gray_as_rgb), which is what evaluate._save_png and torchvision's save_image write; the repetition happens inside
the kernels.  A missing library raises: there is no CPU stand-in for a kernel.
"""
from __future__ import annotations

import ctypes as C
import struct
import zlib
from typing import List, Optional, Sequence

import numpy as np
import torch

from . import _lib, _lib_png
from ._lib_png import check

NONE, SUB, UP, PAETH = _lib_png.PNG_FILTER_NONE, _lib_png.PNG_FILTER_SUB, _lib_png.PNG_FILTER_UP, _lib_png.PNG_FILTER_PAETH
FILTERS = (NONE, SUB, UP, PAETH)
CHUNK = _lib_png.PNG_CHUNK
_WHAT = "png.encode"
_SIGNATURE = b"\x89PNG\r\n\x1a\n"
_IEND = struct.pack(">I", 0) + b"IEND" + struct.pack(">I", zlib.crc32(b"IEND"))
_IMAGE_DTYPE = np.dtype([("src", "<u8"), ("H", "<i4"), ("W", "<i4"), ("channels", "<i4"), ("first_chunk", "<i4"), ("chunks", "<i4"),
                         ("stream_bytes", "<i4")])
_CHUNK_DTYPE = np.dtype([("image", "<i4"), ("index", "<i4")])
assert _IMAGE_DTYPE.itemsize == C.sizeof(_lib_png.ScgPngImage) and _CHUNK_DTYPE.itemsize == C.sizeof(_lib_png.ScgPngChunk)


def _err(msg: str) -> _lib.ScgError:
    return _lib.ScgError(f"{_WHAT}: {msg}")


def _hwc(shape) -> tuple:
    shape = tuple(int(s) for s in shape)
    if len(shape) == 2:
        shape = shape + (1,)
    if len(shape) != 3 or shape[2] not in (1, 3):
        raise _err(f"an image is (H, W), (H, W, 1) or (H, W, 3), not {shape}")
    return shape


def takes(t) -> bool:
    """Is `t` an image the kernels take as it is?  (What they do not take goes to Pillow in save_png.)"""
    return (isinstance(t, torch.Tensor) and t.device.type == "cuda" and t.dtype == torch.uint8 and t.is_contiguous() and
            (t.dim() == 2 or (t.dim() == 3 and t.shape[2] in (1, 3))) and t.numel() > 0)


def file_header(H: int, W: int, color_type: int, idat_bytes: int) -> bytes:
    """The 41 bytes in front of the zlib stream: signature, IHDR, the IDAT's length and name."""
    ihdr = b"IHDR" + struct.pack(">IIBBBBB", W, H, 8, color_type, 0, 0, 0)
    return _SIGNATURE + struct.pack(">I", 13) + ihdr + struct.pack(">I", zlib.crc32(ihdr)) + struct.pack(">I", idat_bytes) + b"IDAT"


class PngPlan:
    """Everything of a batch that depends on its shapes alone: the layout, the image and chunk tables on the device, the workspace
    and the output buffer.  encode() on it allocates nothing and reads nothing back, so it can be captured in a graph: `inputs` are
    the plan's own image tensors (views of one arena), to be rewritten in place between replays."""

    def __init__(self, shapes: Sequence, device="cuda", filter: int = UP, gray_as_rgb: bool = True, own_inputs: bool = True):
        self.device = torch.device(device)
        _lib.stream_of(self.device, "PngPlan")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        if filter not in FILTERS:
            raise _err(f"filter {filter!r} is not one of NONE (0), SUB (1), UP (2), PAETH (4)")
        self.filter, self.gray_as_rgb = int(filter), bool(gray_as_rgb)
        self.shapes = [_hwc(s) for s in shapes]
        n = len(self.shapes)
        self.layout = _lib_png.ScgPngLayout()
        self.images_host = np.zeros(n, dtype=_IMAGE_DTYPE)
        self.inputs: List[torch.Tensor] = []
        self._src = None
        if n == 0:
            return
        lib = _lib_png.load()
        hwc = np.ascontiguousarray(np.asarray(self.shapes, dtype=np.int32).reshape(n, 3))
        hp = hwc.ctypes.data_as(C.POINTER(C.c_int32))
        check(lib.scg_png_layout(n, hp, int(self.gray_as_rgb), C.byref(self.layout), None, None), "scg_png_layout")
        chunks = np.zeros(int(self.layout.chunks), dtype=_CHUNK_DTYPE)
        check(lib.scg_png_layout(n, hp, int(self.gray_as_rgb), C.byref(self.layout),
                                 self.images_host.ctypes.data_as(C.POINTER(_lib_png.ScgPngImage)),
                                 chunks.ctypes.data_as(C.POINTER(_lib_png.ScgPngChunk))), "scg_png_layout")
        with torch.cuda.device(self.device):
            self.chunks_dev = torch.from_numpy(chunks.view(np.uint8).reshape(-1).copy()).to(self.device)
            self.images_dev = torch.empty(n * _IMAGE_DTYPE.itemsize, dtype=torch.uint8, device=self.device)
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

    @property
    def color_types(self):
        return [2 if (c == 3 or self.gray_as_rgb) else 0 for _h, _w, c in self.shapes]

    def _bind(self, images) -> None:
        """Put the images' addresses into the image table; upload it when they changed (a host-to-device copy, never a read)."""
        src = [int(t.data_ptr()) for t in images]
        if src == self._src:
            return
        if torch.cuda.is_current_stream_capturing():
            raise _err("a captured call must use the tensors of the call before it (PngPlan.inputs): the image table cannot be "
                       "uploaded inside a capture")
        self.images_host["src"] = src
        self.images_dev.copy_(torch.from_numpy(self.images_host.view(np.uint8).reshape(-1).copy()))
        self._src = src

    @torch.no_grad()
    def encode(self, images: Optional[Sequence[torch.Tensor]] = None) -> "PackedPngs":
        """Three launches on the current stream.  images: None for the plan's own inputs, or tensors of the plan's shapes."""
        if not self.shapes:
            return PackedPngs(self)
        if images is None:
            images = self.inputs
            if not images:
                raise _err("the plan has no inputs of its own (own_inputs=False): pass the images")
        images = list(images)
        if len(images) != len(self.shapes):
            raise _err(f"{len(images)} images for a plan of {len(self.shapes)}")
        for i, (t, shape) in enumerate(zip(images, self.shapes)):
            if not isinstance(t, torch.Tensor) or t.device != self.device or t.dtype != torch.uint8 or not t.is_contiguous() or \
                    _hwc(t.shape) != shape:
                raise _err(f"image {i} must be a contiguous uint8 tensor of shape {shape} on {self.device}")
        stream = _lib.stream_of(self.out, _WHAT)
        with torch.cuda.device(self.device):
            self._bind(images)
            a = _lib_png.ScgPngEncode()
            a.struct_bytes = C.sizeof(_lib_png.ScgPngEncode)
            a.images, a.filter, a.gray_as_rgb = len(images), self.filter, int(self.gray_as_rgb)
            a.images_host, a.images_dev, a.chunks_dev = self.images_host.ctypes.data, self.images_dev.data_ptr(), self.chunks_dev.data_ptr()
            check(_lib_png.load().scg_png_encode(C.byref(a), self.out.data_ptr(), self.out.numel(), self.workspace.data_ptr(),
                                                 self.workspace.numel(), stream), "scg_png_encode")
        return PackedPngs(self, keep=images)

    def chunk_info(self) -> np.ndarray:
        """What the count kernel left per chunk (bytes, kind, sum_a, sum_b), copied to the host: for tests and tools."""
        o, n = int(self.layout.info_offset), int(self.layout.chunks)
        return self.workspace[o:o + 16 * n].cpu().numpy().view(np.uint32).reshape(n, 4)


    def chunk_lengths(self) -> np.ndarray:
        """The 288 code lengths per chunk as the count kernel left them, copied to the host: for tests and tools."""
        o, n = int(self.layout.lengths_offset), int(self.layout.chunks)
        return self.workspace[o:o + _lib_png.PNG_LENGTHS * n].cpu().numpy().reshape(n, _lib_png.PNG_LENGTHS)


class PackedPngs:
    """The zlib streams of a batch in the plan's output buffer, each at a multiple of 16 bytes, and the table that says where."""

    def __init__(self, plan: PngPlan, keep=None):
        self.plan, self._keep = plan, keep
        self.table_host: Optional[np.ndarray] = None
        self.host: Optional[torch.Tensor] = None

    def __len__(self):
        return len(self.plan.shapes)

    def to_host(self) -> "PackedPngs":
        """The batch's TWO host reads: the table, then exactly `total` bytes of the buffer into pinned memory."""
        n = len(self)
        if self.host is not None or n == 0:
            if n == 0 and self.table_host is None:
                self.table_host = np.zeros((1, 2), dtype=np.uint32)
            return self
        stream = torch.cuda.current_stream(self.plan.device)
        table = torch.empty((n + 1, 2), dtype=torch.int32, pin_memory=True)
        table.copy_(self.plan.table.view(n + 1, 2), non_blocking=True)
        stream.synchronize()
        self.table_host = table.numpy().view(np.uint32)
        total = int(self.table_host[n, 0])
        if int(self.table_host[n, 1]) != n or total > self.plan.out.numel():
            raise _err(f"the table names {int(self.table_host[n, 1])} images and {total} bytes: not this batch's")
        self.host = torch.empty(total, dtype=torch.uint8, pin_memory=True)
        self.host.copy_(self.plan.out[:total], non_blocking=True)
        stream.synchronize()
        return self

    def streams(self) -> List[memoryview]:
        """The images' zlib streams as views of the host copy (the gaps between them belong to none)."""
        self.to_host()
        if len(self) == 0:
            return []
        data = memoryview(self.host.numpy())
        return [data[int(o):int(o) + int(b)] for o, b in self.table_host[:len(self)]]

    def files(self) -> List[bytes]:
        """The complete PNG files."""
        out = []
        for (H, W, _c), ctype, s in zip(self.plan.shapes, self.plan.color_types, self.streams()):
            crc = zlib.crc32(s, zlib.crc32(b"IDAT"))
            out.append(b"".join((file_header(H, W, ctype, len(s)), s, struct.pack(">I", crc), _IEND)))
        return out

    def write(self, paths: Sequence[str]) -> None:
        paths = list(paths)
        if len(paths) != len(self):
            raise _err(f"{len(paths)} paths for {len(self)} images")
        for path, (H, W, _c), ctype, s in zip(paths, self.plan.shapes, self.plan.color_types, self.streams()):
            with open(path, "wb") as fh:
                fh.write(file_header(H, W, ctype, len(s)))
                fh.write(s)
                fh.write(struct.pack(">I", zlib.crc32(s, zlib.crc32(b"IDAT"))) + _IEND)


def encode(images: Sequence[torch.Tensor], filter: int = UP, gray_as_rgb: bool = True) -> PackedPngs:
    """The batch's zlib streams on the device: three launches whatever the number of images and their sizes, no host read."""
    images = list(images)
    for i, t in enumerate(images):
        if not isinstance(t, torch.Tensor):
            raise _err(f"image {i} is not a tensor")
        _lib.stream_of(t, _WHAT)
        if not takes(t):
            raise _err(f"image {i} must be a contiguous, non-empty uint8 tensor shaped (H, W), (H, W, 1) or (H, W, 3); it is "
                       f"{t.dtype} {tuple(t.shape)}")
    device = images[0].device if images else torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else None
    if device is None:
        raise _err("needs the ROCm GPU ('cuda'); there is no CPU path")
    return PngPlan([t.shape for t in images], device, filter, gray_as_rgb, own_inputs=False).encode(images)


def check_route(png: str) -> bool:
    """The `png` keyword of render_set, render_video and MatchpointSnapshot.write: True for "device", False for "pillow"."""
    if png not in ("pillow", "device"):
        raise ValueError(f'png must be "pillow" or "device", not {png!r}')
    return png == "device"


def write_batch(paths: Sequence[str], images: Sequence[torch.Tensor], filter: int = UP, gray_as_rgb: bool = True) -> None:
    """All files of a call in one batch: encode, the two reads, the writes."""
    encode(images, filter, gray_as_rgb).write(paths)


def save_png(path: str, tensor, filter: int = UP, gray_as_rgb: bool = True) -> None:
    """One image.  A uint8 device tensor of one or three channels goes through the kernels; CPU tensors, arrays, other dtypes and
    other channel counts go to Pillow as before (evaluate._save_png for what it takes, Image.fromarray for the rest)."""
    if takes(tensor):
        write_batch([path], [tensor], filter, gray_as_rgb)
        return
    from PIL import Image
    arr = tensor.detach().cpu().numpy() if isinstance(tensor, torch.Tensor) else np.asarray(tensor)
    if arr.dtype == np.uint8 and (arr.ndim == 2 or (arr.ndim == 3 and arr.shape[2] == 3)):
        from .evaluate import _save_png
        _save_png(path, arr)
        return
    Image.fromarray(arr[:, :, 0] if arr.ndim == 3 and arr.shape[2] == 1 else arr).save(path, format="PNG")

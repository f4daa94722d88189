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
from typing import List, Sequence

import numpy as np
import torch

from . import _filebatch, _lib_png
from ._filebatch import takes        # noqa: F401  (png.takes)
from ._lib_png import check

NONE, SUB, UP, PAETH = _lib_png.PNG_FILTER_NONE, _lib_png.PNG_FILTER_SUB, _lib_png.PNG_FILTER_UP, _lib_png.PNG_FILTER_PAETH
FILTERS = (NONE, SUB, UP, PAETH)
CHUNK = _lib_png.PNG_CHUNK
_SIGNATURE = b"\x89PNG\r\n\x1a\n"
_IEND = struct.pack(">I", 0) + b"IEND" + struct.pack(">I", zlib.crc32(b"IEND"))
_IMAGE_DTYPE = np.dtype([("src", "<u8"), ("H", "<i4"), ("W", "<i4"), ("channels", "<i4"), ("first_chunk", "<i4"), ("chunks", "<i4"),
                         ("stream_bytes", "<i4")])
_CHUNK_DTYPE = np.dtype([("image", "<i4"), ("index", "<i4")])
assert _IMAGE_DTYPE.itemsize == C.sizeof(_lib_png.ScgPngImage) and _CHUNK_DTYPE.itemsize == C.sizeof(_lib_png.ScgPngChunk)


def file_header(H: int, W: int, color_type: int, idat_bytes: int) -> bytes:
    """The 41 bytes in front of the zlib stream: signature, IHDR, the IDAT's length and name."""
    ihdr = b"IHDR" + struct.pack(">IIBBBBB", W, H, 8, color_type, 0, 0, 0)
    return _SIGNATURE + struct.pack(">I", 13) + ihdr + struct.pack(">I", zlib.crc32(ihdr)) + struct.pack(">I", idat_bytes) + b"IDAT"


class PngPlan(_filebatch.FilePlan):
    """The plan of a batch of PNG files (FilePlan): the image and chunk tables on the device, the workspace, the output buffer."""

    LIB, WHAT, ENTRY, ENCODE, COLUMNS = _lib_png, "png.encode", "scg_png_encode", _lib_png.ScgPngEncode, 2

    def __init__(self, shapes: Sequence, device="cuda", filter: int = UP, gray_as_rgb: bool = True, own_inputs: bool = True):
        super().__init__(shapes, device, own_inputs, filter=filter, gray_as_rgb=gray_as_rgb)

    def _configure(self, filter, gray_as_rgb) -> None:
        if filter not in FILTERS:
            raise self._err(f"filter {filter!r} is not one of NONE (0), SUB (1), UP (2), PAETH (4)")
        self.filter, self.gray_as_rgb = int(filter), bool(gray_as_rgb)

    def _lay_out(self):
        n = len(self.shapes)
        lay, images = _lib_png.ScgPngLayout(), np.zeros(n, dtype=_IMAGE_DTYPE)
        if n == 0:
            return lay, images, {}
        lib = _lib_png.load()
        hwc = np.ascontiguousarray(np.asarray(self.shapes, dtype=np.int32).reshape(n, 3))
        hp = hwc.ctypes.data_as(C.POINTER(C.c_int32))
        check(lib.scg_png_layout(n, hp, int(self.gray_as_rgb), C.byref(lay), None, None), "scg_png_layout")
        chunks = np.zeros(int(lay.chunks), dtype=_CHUNK_DTYPE)
        check(lib.scg_png_layout(n, hp, int(self.gray_as_rgb), C.byref(lay), images.ctypes.data_as(C.POINTER(_lib_png.ScgPngImage)),
                                 chunks.ctypes.data_as(C.POINTER(_lib_png.ScgPngChunk))), "scg_png_layout")
        return lay, images, {"chunks_dev": chunks}

    def _fill(self, a) -> None:
        a.filter, a.gray_as_rgb, a.chunks_dev = self.filter, int(self.gray_as_rgb), self.chunks_dev.data_ptr()

    @property
    def color_types(self):
        return [2 if (c == 3 or self.gray_as_rgb) else 0 for _h, _w, c in self.shapes]

    def chunk_info(self) -> np.ndarray:
        """What the count kernel left per chunk (bytes, kind, sum_a, sum_b), copied to the host: for tests and tools."""
        o, n = int(self.layout.info_offset), int(self.layout.chunks)
        return self.workspace[o:o + 16 * n].cpu().numpy().view(np.uint32).reshape(n, 4)

    def chunk_lengths(self) -> np.ndarray:
        """The 288 code lengths per chunk as the count kernel left them, copied to the host: for tests and tools."""
        o, n = int(self.layout.lengths_offset), int(self.layout.chunks)
        return self.workspace[o:o + _lib_png.PNG_LENGTHS * n].cpu().numpy().reshape(n, _lib_png.PNG_LENGTHS)


class PackedPngs(_filebatch.PackedFiles):
    """The zlib streams of a batch in the plan's output buffer (PackedFiles; the table's row: offset, bytes)."""

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
        for path, (H, W, _c), ctype, s in zip(self._paths(paths), self.plan.shapes, self.plan.color_types, self.streams()):
            with open(path, "wb") as fh:
                fh.write(file_header(H, W, ctype, len(s)))
                fh.write(s)
                fh.write(struct.pack(">I", zlib.crc32(s, zlib.crc32(b"IDAT"))) + _IEND)


PngPlan.PACKED = PackedPngs


def encode(images: Sequence[torch.Tensor], filter: int = UP, gray_as_rgb: bool = True) -> PackedPngs:
    """The batch's zlib streams on the device: three launches whatever the number of images and their sizes, no host read."""
    return _filebatch.encode(images, PngPlan, filter=filter, gray_as_rgb=gray_as_rgb)


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

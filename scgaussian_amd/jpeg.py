"""JPEG files and Motion-JPEG video from uint8 device tensors, host side (libscg_jpg.so, include/jpg/scg_jpeg.h states the stream).

    packed = jpeg.encode([img0, img1, ...], quality=90, subsampling="4:2:0", bgr=False)     three launches, no host read
    packed.to_host()                              TWO host reads: the table, then exactly `total` bytes into pinned memory
    packed.files() / packed.write(paths)          complete JPEG files, the bytes libjpeg writes for the same options
    plan = jpeg.JpegPlan(shapes, device, ...)     the uploaded tables and the buffers, for repeated and captured calls
    jpeg.save_jpeg(path, tensor)                  one image; what the kernels do not take goes to Pillow
    jpeg.write_avi(path, files, fps, W, H)        the files as the frames of a Motion-JPEG AVI: host only, `struct` alone
    jpeg.read_avi(path)                           the frames' files of such a video, for jpeg_decode.decode: host only, `struct` alone

An image is a contiguous uint8 tensor on the GPU shaped (H, W), (H, W, 1) or (H, W, 3); a list of them or one (N, H, W, 3) tensor
is a batch.  The output capacity of an image defaults to header + 3 H W bytes, which every real frame stays far below; a file that
needs more is flagged by the kernels, no byte of it is written, and to_host() encodes the batch once more with what the table says
each file needs.  A missing library raises: there is no CPU stand-in for a kernel.
"""
from __future__ import annotations

import ctypes as C
import struct
from fractions import Fraction
from typing import List, Sequence

import numpy as np
import torch

from . import _filebatch, _lib, _lib_jpg
from ._filebatch import takes        # noqa: F401  (jpeg.takes)
from ._lib_jpg import check

SUBSAMPLINGS = {"4:4:4": _lib_jpg.JPEG_444, "4:2:0": _lib_jpg.JPEG_420}
_WHAT = "jpeg.encode"
_IMAGE_DTYPE = np.dtype([("src", "<u8"), ("H", "<i4"), ("W", "<i4"), ("channels", "<i4"), ("first_segment", "<i4"), ("segments", "<i4"),
                         ("mcus", "<i4"), ("header_offset", "<i4"), ("header_bytes", "<i4"), ("capacity", "<u4"), ("reserved", "<i4")])
_SEGMENT_DTYPE = np.dtype([("image", "<i4"), ("row", "<i4")])
assert _IMAGE_DTYPE.itemsize == C.sizeof(_lib_jpg.ScgJpegImage) and _SEGMENT_DTYPE.itemsize == C.sizeof(_lib_jpg.ScgJpegSegment)
AVI_MAX_BYTES = 2 ** 32 - 1


def _err(msg: str) -> _lib.ScgError:
    return _lib.ScgError(f"{_WHAT}: {msg}")


def _options(quality, subsampling, bgr):
    if isinstance(quality, bool) or not isinstance(quality, (int, np.integer)) or not 1 <= int(quality) <= 100:
        raise _err(f"quality {quality!r} is not an integer in 1..100")
    if subsampling not in SUBSAMPLINGS:
        raise _err(f'subsampling {subsampling!r} is not "4:4:4" or "4:2:0"')
    return int(quality), str(subsampling), bool(bgr)


def layout(shapes: Sequence, quality: int = 90, subsampling: str = "4:2:0", capacities=None):
    """scg_jpeg_layout on the host alone (no GPU is touched): (ScgJpegLayout, image records, segment records, header templates)."""
    quality, subsampling, _ = _options(quality, subsampling, False)
    shapes = [_filebatch.hwc(s, _err) for s in shapes]
    n = len(shapes)
    lay = _lib_jpg.ScgJpegLayout()
    images = np.zeros(n, dtype=_IMAGE_DTYPE)
    if n == 0:
        return lay, images, np.zeros(0, dtype=_SEGMENT_DTYPE), np.zeros(0, dtype=np.uint8)
    lib = _lib_jpg.load()
    hwc = np.ascontiguousarray(np.asarray(shapes, dtype=np.int32).reshape(n, 3))
    hp = hwc.ctypes.data_as(C.POINTER(C.c_int32))
    cp = None
    if capacities is not None:
        caps = np.ascontiguousarray(np.asarray(capacities, dtype=np.int64).reshape(-1))
        if caps.shape[0] != n or caps.min() < 0 or caps.max() > 2 ** 32 - 1:
            raise _err(f"capacities must be {n} values in 0..2^32 - 1")
        caps = caps.astype(np.uint32)
        cp = caps.ctypes.data_as(C.POINTER(C.c_uint32))
    sub = SUBSAMPLINGS[subsampling]
    check(lib.scg_jpeg_layout(n, hp, quality, sub, cp, C.byref(lay), None, None, None), "scg_jpeg_layout")
    segments = np.zeros(int(lay.segments), dtype=_SEGMENT_DTYPE)
    headers = np.zeros(int(lay.headers_bytes), dtype=np.uint8)
    check(lib.scg_jpeg_layout(n, hp, quality, sub, cp, C.byref(lay), images.ctypes.data_as(C.POINTER(_lib_jpg.ScgJpegImage)),
                              segments.ctypes.data_as(C.POINTER(_lib_jpg.ScgJpegSegment)),
                              headers.ctypes.data_as(C.POINTER(C.c_uint8))), "scg_jpeg_layout")
    return lay, images, segments, headers


class JpegPlan(_filebatch.FilePlan):
    """The plan of a batch of JPEG files (FilePlan): the image, segment and header tables on the device, the workspace, the output
    buffer with every file's capacity."""

    LIB, WHAT, ENTRY, ENCODE, COLUMNS = _lib_jpg, _WHAT, "scg_jpeg_encode", _lib_jpg.ScgJpegEncode, 4

    def __init__(self, shapes: Sequence, device="cuda", quality: int = 90, subsampling: str = "4:2:0", bgr: bool = False,
                 capacities=None, own_inputs: bool = True):
        super().__init__(shapes, device, own_inputs, quality=quality, subsampling=subsampling, bgr=bgr, capacities=capacities)

    def _configure(self, quality, subsampling, bgr, capacities) -> None:
        self.quality, self.subsampling, self.bgr = _options(quality, subsampling, bgr)
        self._capacities = capacities

    def _lay_out(self):
        lay, images, segments, headers = layout(self.shapes, self.quality, self.subsampling, self._capacities)
        return lay, images, {"segments_dev": segments, "headers_dev": headers}

    def _fill(self, a) -> None:
        a.quality, a.subsampling, a.bgr = self.quality, SUBSAMPLINGS[self.subsampling], int(self.bgr)
        a.headers_bytes = int(self.layout.headers_bytes)
        a.segments_dev, a.headers_dev = self.segments_dev.data_ptr(), self.headers_dev.data_ptr()


class PackedJpegs(_filebatch.PackedFiles):
    """The files of a batch in the plan's output buffer (PackedFiles; the table's row: offset, bytes, need, overflow)."""

    def __init__(self, plan: JpegPlan, keep=None):
        super().__init__(plan, keep)
        self.retried = False

    def to_host(self, retry: bool = True) -> "PackedJpegs":
        """The batch's TWO host reads: the table, then exactly `total` bytes of the buffer into pinned memory.  When the table flags
        a file that did not fit its capacity and `retry` holds, the batch is encoded once more with what every file needs (and read
        again); without `retry` the flagged files stay empty."""
        if not self._read_table():
            return self
        n, plan = len(self), self.plan
        if retry and int(self.table_host[n, 2]) and not self.retried:
            need = np.maximum(self.table_host[:n, 2].astype(np.int64), plan.images_host["capacity"].astype(np.int64))
            again = JpegPlan(plan.shapes, plan.device, plan.quality, plan.subsampling, plan.bgr, capacities=need, own_inputs=False)
            self.plan = again.encode(self._keep).plan
            self.retried = True
            return self.to_host(retry=False)
        self._read_files()
        return self

    @property
    def overflowed(self) -> List[int]:
        """The images whose file did not fit (after to_host)."""
        self.to_host()
        return [i for i in range(len(self)) if self.table_host[i, 3]]

    def files(self) -> List[bytes]:
        """The complete JPEG files (b"" for a file that did not fit and was not encoded again)."""
        self.to_host()
        if len(self) == 0:
            return []
        data = memoryview(self.host.numpy())
        return [bytes(data[int(o):int(o) + int(b)]) for o, b, _need, _flag in self.table_host[:len(self)]]

    def write(self, paths: Sequence[str]) -> None:
        for path, f in zip(self._paths(paths), self.files()):
            with open(path, "wb") as fh:
                fh.write(f)


JpegPlan.PACKED = PackedJpegs


def _batch(images) -> list:
    if isinstance(images, torch.Tensor):
        if images.dim() != 4:
            raise _err(f"a batch tensor is (N, H, W, 3) or (N, H, W, 1), not {tuple(images.shape)}")
        return [images[i] for i in range(images.shape[0])]
    return list(images)


def encode(images, quality: int = 90, subsampling: str = "4:2:0", bgr: bool = False, capacities=None) -> PackedJpegs:
    """The batch's files on the device: three launches whatever the number of images and their sizes, no host read."""
    quality, subsampling, bgr = _options(quality, subsampling, bgr)
    return _filebatch.encode(_batch(images), JpegPlan, quality=quality, subsampling=subsampling, bgr=bgr, capacities=capacities)


def save_jpeg(path: str, tensor, quality: int = 90, subsampling: str = "4:2:0", bgr: bool = False) -> None:
    """One image.  A uint8 device tensor of one or three channels goes through the kernels; CPU tensors, arrays, other dtypes and
    other modes go to Pillow, with the same options where it takes them."""
    quality, subsampling, bgr = _options(quality, subsampling, bgr)
    if takes(tensor):
        encode([tensor], quality, subsampling, bgr).write([path])
        return
    from PIL import Image
    arr = tensor.detach().cpu().numpy() if isinstance(tensor, torch.Tensor) else np.asarray(tensor)
    if arr.ndim == 3 and arr.shape[2] == 1:
        arr = arr[:, :, 0]
    if arr.ndim == 3 and arr.shape[2] == 3 and bgr:
        arr = np.ascontiguousarray(arr[:, :, ::-1])
    kw = {"subsampling": {"4:4:4": 0, "4:2:0": 2}[subsampling]} if arr.ndim == 3 else {}
    Image.fromarray(arr).save(path, format="JPEG", quality=quality, optimize=False, restart_marker_rows=1, **kw)


def _chunk(name: bytes, body: bytes) -> bytes:
    return name + struct.pack("<I", len(body)) + body + (b"\0" if len(body) & 1 else b"")


def write_avi(path: str, files: Sequence[bytes], fps, width: int, height: int) -> None:
    """The JPEG files as the frames of a Motion-JPEG AVI (AVI 1.0, one video stream, an idx1 index): RIFF 'AVI ', LIST hdrl (avih,
    LIST strl (strh 'vids' / 'MJPG', strf: a BITMAPINFOHEADER, 'MJPG', 24 bit)), LIST movi of '00dc' chunks padded to even length,
    idx1 with offsets counted from the 'movi' name.  A file of more than 2^32 - 1 bytes raises: no OpenDML extension is written."""
    files = [bytes(f) for f in files]
    width, height = int(width), int(height)
    if not files:
        raise ValueError("write_avi needs at least one frame")
    if not (1 <= width <= 65535 and 1 <= height <= 65535):
        raise ValueError(f"a frame of {width} x {height} pixels (1..65535)")
    for i, f in enumerate(files):
        if f[:2] != b"\xff\xd8" or f[-2:] != b"\xff\xd9":
            raise ValueError(f"frame {i} is not a JPEG file")
    rate = Fraction(fps).limit_denominator(100000)
    if rate <= 0:
        raise ValueError(f"fps = {fps!r} must be positive")
    n, biggest = len(files), max(len(f) for f in files)
    movi_bytes = 4 + sum(8 + len(f) + (len(f) & 1) for f in files)
    total = 12 + (8 + 4 + (8 + 56) + (8 + 4 + (8 + 56) + (8 + 40))) + (8 + movi_bytes) + (8 + 16 * n)
    if total > AVI_MAX_BYTES:
        raise ValueError(f"the video needs {total} bytes: more than 2^32 - 1 (AVI 1.0, no OpenDML)")
    us = int(round(1e6 * rate.denominator / rate.numerator))
    avih = struct.pack("<14I", us, int(biggest * float(rate)) & 0xFFFFFFFF, 0, 0x10, n, 0, 1, biggest, width, height, 0, 0, 0, 0)
    strh = b"vidsMJPG" + struct.pack("<IHHIIIIIIII4H", 0, 0, 0, 0, rate.denominator, rate.numerator, 0, n, biggest, 0xFFFFFFFF, 0,
                                     0, 0, width, height)
    strf = struct.pack("<IiiHH4sIiiII", 40, width, height, 1, 24, b"MJPG", width * height * 3, 0, 0, 0, 0)
    strl = b"LIST" + struct.pack("<I", 4 + 8 + len(strh) + 8 + len(strf)) + b"strl" + _chunk(b"strh", strh) + _chunk(b"strf", strf)
    hdrl = b"LIST" + struct.pack("<I", 4 + 8 + len(avih) + len(strl)) + b"hdrl" + _chunk(b"avih", avih) + strl
    index, at = [], 4
    for f in files:
        index.append(b"00dc" + struct.pack("<III", 0x10, at, len(f)))
        at += 8 + len(f) + (len(f) & 1)
    with open(path, "wb") as fh:
        fh.write(b"RIFF" + struct.pack("<I", total - 8) + b"AVI " + hdrl + b"LIST" + struct.pack("<I", movi_bytes) + b"movi")
        for f in files:
            fh.write(_chunk(b"00dc", f))
        fh.write(_chunk(b"idx1", b"".join(index)))


def read_avi(path: str) -> List[bytes]:
    """The frames' JPEG files of a Motion-JPEG AVI that write_avi wrote (RIFF 'AVI ', the '00dc' chunks of LIST movi, in order).
    Host only.  With jpeg_decode.decode the project reads back its own videos: their frames carry one restart interval per MCU row."""
    with open(path, "rb") as fh:
        data = fh.read()
    if len(data) < 12 or data[:4] != b"RIFF" or data[8:12] != b"AVI ":
        raise ValueError(f"{path} is not a RIFF AVI file")
    end = min(len(data), 8 + struct.unpack_from("<I", data, 4)[0])
    at, frames = 12, None
    while at + 8 <= end:
        name, size = data[at:at + 4], struct.unpack_from("<I", data, at + 4)[0]
        if name == b"LIST" and data[at + 8:at + 12] == b"movi":
            frames, p, stop = [], at + 12, min(end, at + 8 + size)
            while p + 8 <= stop:
                cname, csize = data[p:p + 4], struct.unpack_from("<I", data, p + 4)[0]
                if p + 8 + csize > stop:
                    raise ValueError(f"{path}: the chunk at byte {p} runs past its list")
                if cname == b"00dc":
                    frames.append(data[p + 8:p + 8 + csize])
                p += 8 + csize + (csize & 1)
            break
        at += 8 + size + (size & 1)
    if frames is None:
        raise ValueError(f"{path} has no LIST movi")
    return frames


def check_options(quality, subsampling, fps) -> None:
    """What render_video(video="mjpeg") validates before its first launch."""
    _options(quality, subsampling, True)
    if not Fraction(fps).limit_denominator(100000) > 0:
        raise ValueError(f"fps = {fps!r} must be positive")


def check_route(video) -> bool:
    """The `video` keyword of render_video: False for None, True for "mjpeg"."""
    if video not in (None, "mjpeg"):
        raise ValueError(f'video must be None or "mjpeg", not {video!r}')
    return video == "mjpeg"

"""The camera images' downsizing on the GPU (csrc/resample.hip, libscg_img.so): Pillow's bicubic resize byte for byte, one upload.

The reference resizes every image on one host core: loadCam (utils/camera_utils.py:20-72) calls PILtoTorch(cam_info.image,
resolution) (utils/general_utils.py:22-28: `pil_image.resize(resolution)`, `/ 255.0`, `permute`), for a 4032 x 3024 photograph at
-r 8 a 33-tap antialiased bicubic over 12 M pixels.  For 8-bit images Pillow's resampler is integer arithmetic, so here the bytes
are computed where they are needed:

    from scgaussian_amd import images
    import utils.camera_utils as camera_utils
    images.install(camera_utils)                      # loadCam's PILtoTorch now runs here; Scene(...) runs unchanged

    images.install(camera_utils, decode="device")     # ... and a JPEG file is decoded on the GPU too (jpeg_decode.py)
    image = images.load_image(path, (w, h))           # the direct form: file -> float32 (C, h, w), PILtoTorch(Image.open(path), ..)
    imgs = images.load_images(paths, (w, h))          # the same tensors for a list: ONE jpeg_decode.decode_batch, one resize per group
    images.install_batched(camera_utils)              # cameraList_from_camInfos loads a scene's JPEG files with one load_images

    u8 = images.resize_u8(np.asarray(pil_image), (w, h))          # device uint8 (h, w, 3) == np.asarray(pil_image.resize((w, h)))
    u8, f32 = images.resize_batch(arrays, (w, h), want_float=True)  # one upload and at most two launches per chunk
    cam.image = u8.cpu().numpy()                                  # what mono.MonoSetup.build takes as a view's bytes

The rule (include/img/scg_resample.h): each axis on its own, horizontal first and rounded to bytes; per output index a window and
coefficients with 22 fractional bits, from IEEE double arithmetic in a fixed order (axis_table below: numpy's element-wise
operations round once each and never fuse); acc = 2^21 + sum(byte * k) in int32, out = clamp(acc >> 22, 0, 255).  Modes `L` and `RGB`
take the kernels.  `RGBA` / `LA` (which Pillow resizes premultiplied, with its own rounding), `P`, `1`, `I;16`, ... and any scale
beyond a 32x reduction (ksize > 129) go through Pillow on the host and one upload and give the same tensor.  With
decode="device" a baseline JPEG file that Image.open has not loaded yet is read from disk, decoded by jpeg_decode.decode (Pillow's
pixels byte for byte) and resized in place: its pixels never exist on the host.  Decoding PNG (and every JPEG the decoder refuses)
stays in Pillow; cv2.resize of the masks (camera_utils.py:52,55) and filters other than bicubic are not covered.
"""
from __future__ import annotations

import functools
import math
import os
from typing import Dict, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import _lib, _lib_img

MAX_KSIZE = _lib_img.RESAMPLE_MAX_KSIZE
STRIP, STRIP_ROWS, VTILE = _lib_img.RESAMPLE_STRIP, _lib_img.RESAMPLE_STRIP_ROWS, _lib_img.RESAMPLE_VTILE
PITCH_ALIGN = _lib_img.RESAMPLE_PITCH_ALIGN
PRECISION_BITS = 22
_ALIGN = 16

Source = Union[np.ndarray, torch.Tensor]


def _err(msg: str):
    return _lib.ScgError("images: " + msg)


# --------------------------------------------------------------------------------------------------------------------------------
# loadCam's size arithmetic
# --------------------------------------------------------------------------------------------------------------------------------
def target_resolution(orig_w: int, orig_h: int, resolution, resolution_scale: float = 1.0) -> Tuple[int, int]:
    """(width, height) loadCam resizes an orig_w x orig_h image to (utils/camera_utils.py:25-42) for args.resolution and the
    scene's resolution_scale: the `round` branch for 1 / 2 / 4 / 8, otherwise the truncating one, where -1 scales images wider
    than 1600 px down to 1600 and any other value is the target width."""
    if resolution in [1, 2, 4, 8]:
        return round(orig_w / (resolution_scale * resolution)), round(orig_h / (resolution_scale * resolution))
    if resolution == -1:
        global_down = orig_w / 1600 if orig_w > 1600 else 1
    else:
        global_down = orig_w / resolution
    scale = float(global_down) * float(resolution_scale)
    return int(orig_w / scale), int(orig_h / scale)


# --------------------------------------------------------------------------------------------------------------------------------
# the host tables
# --------------------------------------------------------------------------------------------------------------------------------
def ksize_of(in_size: int, out_size: int) -> int:
    return int(math.ceil(2.0 * max(in_size / out_size, 1.0))) * 2 + 1


@functools.lru_cache(maxsize=64)
def axis_table(in_size: int, out_size: int) -> Tuple[np.ndarray, np.ndarray]:
    """(bounds int32 (out_size, 2): first source index and count; coeffs int32 (out_size, ksize)) of one axis, read-only.
    Every line is one rounding per operation in the order of the rule; the sum of a window's weights runs in index order."""
    if in_size < 1 or out_size < 1:
        raise _err(f"cannot resample {in_size} samples to {out_size}")
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = 2.0 * fs
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / fs
    center = (np.arange(out_size, dtype=np.float64) + 0.5) * scale
    xmin = np.maximum(np.trunc(center - support + 0.5), 0.0).astype(np.int64)
    xmax = np.minimum(np.trunc(center + support + 0.5), float(in_size)).astype(np.int64) - xmin
    x = np.arange(ksize, dtype=np.int64)[None, :]
    t = np.abs(((x + xmin[:, None]) - center[:, None] + 0.5) * ss)
    a = -0.5
    near = ((a + 2.0) * t - (a + 3.0)) * t * t + 1
    far = (((t - 5) * t + 8) * t - 4) * a
    w = np.where(t < 1.0, near, np.where(t < 2.0, far, 0.0))
    w = np.where(x < xmax[:, None], w, 0.0)
    ww = np.zeros(out_size, dtype=np.float64)
    for j in range(ksize):                                # in index order (adding the zeros behind a window changes nothing)
        ww = ww + w[:, j]
    safe = np.where(ww != 0.0, ww, 1.0)
    w = np.where((ww != 0.0)[:, None], w / safe[:, None], w)
    one = float(1 << PRECISION_BITS)
    k = np.where(w < 0.0, np.trunc(w * one - 0.5), np.trunc(w * one + 0.5)).astype(np.int32)
    bounds = np.stack((xmin, xmax), axis=1).astype(np.int32)
    bounds.setflags(write=False)
    k.setflags(write=False)
    return bounds, k


def _round_up(v: int, to: int) -> int:
    return (v + to - 1) // to * to


class ResizePlan:
    """The host tables of both axes, the byte sizes and the layout of the staged buffer of one (in_size, out_size, channels).
    Sizes are (width, height), as Pillow takes them.  Staged buffer of n images: [n * image_bytes | tables], the tables at
    tables_offset(n): hbounds, hcoeffs, vbounds, vcoeffs, each 16-byte aligned (an axis that does not change has none)."""

    def __init__(self, in_size: Tuple[int, int], out_size: Tuple[int, int], channels: int):
        self.win, self.hin = int(in_size[0]), int(in_size[1])
        self.wout, self.hout = int(out_size[0]), int(out_size[1])
        self.channels = int(channels)
        if self.channels not in (1, 3):
            raise _err(f"{channels} channels: the kernels take 1 or 3")
        if min(self.win, self.hin, self.wout, self.hout) < 1:
            raise _err(f"cannot resize {self.win} x {self.hin} to {self.wout} x {self.hout}")
        self.horizontal, self.vertical = self.wout != self.win, self.hout != self.hin
        self.hksize = ksize_of(self.win, self.wout) if self.horizontal else 0
        self.vksize = ksize_of(self.hin, self.hout) if self.vertical else 0
        # what the kernels take; anything else is resized by Pillow on the host
        self.device_route = (max(self.hksize, self.vksize) <= MAX_KSIZE
                             and max(self.win, self.hin, self.wout, self.hout) <= _lib_img.RESAMPLE_MAX_SIZE)
        self.image_bytes = self.hin * self.win * self.channels
        self.out_bytes = self.hout * self.wout * self.channels
        self.pitch = _round_up(self.wout * self.channels, PITCH_ALIGN)
        self.table_offsets: Dict[str, int] = {}
        parts: List[Tuple[int, np.ndarray]] = []
        pos = 0
        if self.device_route:
            for axis, on, sizes in (("h", self.horizontal, (self.win, self.wout)), ("v", self.vertical, (self.hin, self.hout))):
                if not on:
                    continue
                for name, arr in zip((axis + "bounds", axis + "coeffs"), axis_table(*sizes)):
                    self.table_offsets[name] = pos
                    parts.append((pos, arr))
                    pos = _round_up(pos + arr.nbytes, _ALIGN)
        self.tables = np.zeros(pos, dtype=np.uint8)
        for off, arr in parts:
            self.tables[off:off + arr.nbytes] = arr.reshape(-1).view(np.uint8)
        self.tables.setflags(write=False)
        self._device_tables: Dict[torch.device, torch.Tensor] = {}

    def mid_bytes(self, n: int) -> int:
        return n * self.hin * self.pitch if self.horizontal else 0

    def tables_offset(self, n: int) -> int:
        return _round_up(n * self.image_bytes, _ALIGN)

    def staged_bytes(self, n: int) -> int:
        return self.tables_offset(n) + self.tables.size

    def device_tables(self, dev: torch.device) -> torch.Tensor:
        """The tables on `dev` for sources that are there already: uploaded once per plan and device, then reused."""
        t = self._device_tables.get(dev)
        if t is None:
            t = torch.from_numpy(np.array(self.tables)).to(dev)
            self._device_tables[dev] = t
        return t


@functools.lru_cache(maxsize=32)
def plan_of(in_size: Tuple[int, int], out_size: Tuple[int, int], channels: int) -> ResizePlan:
    return ResizePlan(in_size, out_size, channels)


# --------------------------------------------------------------------------------------------------------------------------------
# the calls
# --------------------------------------------------------------------------------------------------------------------------------
def _device(device) -> torch.device:
    dev = torch.device(device)
    if dev.type != "cuda":
        raise _err("the resize runs on the ROCm GPU ('cuda'); there is no CPU path (Pillow resizes on the host)")
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    return dev


def _hwc(shape: Sequence[int], what: str) -> Tuple[int, int, int]:
    if len(shape) == 2:
        return int(shape[0]), int(shape[1]), 1
    if len(shape) == 3 and shape[2] in (1, 3):
        return int(shape[0]), int(shape[1]), int(shape[2])
    raise _err(f"{what} has shape {tuple(shape)}, not (H, W), (H, W, 1) or (H, W, 3)")


def _check_u8(src: Source, what: str) -> None:
    dtype = src.dtype
    if dtype not in (np.uint8, torch.uint8):
        raise _err(f"{what} is {dtype}, not uint8")


def _launch(plan: ResizePlan, n: int, src_ptr: int, tables: torch.Tensor, tables_off: int, out: torch.Tensor,
            out_float: Optional[torch.Tensor], dev: torch.device) -> None:
    """At most two launches on the current stream of `dev`; `tables` is the device buffer that holds plan.tables at tables_off."""
    mid = torch.empty(plan.mid_bytes(n), dtype=torch.uint8, device=dev)
    base = tables.data_ptr() + tables_off
    ptr = {name: base + off for name, off in plan.table_offsets.items()}
    with torch.cuda.device(dev):
        _lib_img.check(_lib_img.load().scg_resample_u8(
            src_ptr, n, plan.hin, plan.win, plan.channels, plan.hout, plan.wout,
            ptr.get("hbounds"), ptr.get("hcoeffs"), plan.hksize, ptr.get("vbounds"), ptr.get("vcoeffs"), plan.vksize,
            mid.data_ptr() if mid.numel() else None, mid.numel(), out.data_ptr(), out.numel(),
            out_float.data_ptr() if out_float is not None else None, out_float.numel() * 4 if out_float is not None else 0,
            _lib.stream_of(dev, "images.resize")), "scg_resample_u8")


def _pillow_resize(arr: np.ndarray, size: Tuple[int, int]) -> np.ndarray:
    from PIL import Image
    return np.asarray(Image.fromarray(arr).resize(size))


def _check_out(t: Optional[torch.Tensor], shape: Tuple[int, ...], dtype: torch.dtype, dev: torch.device, what: str) -> None:
    if t is not None and (tuple(t.shape) != shape or t.dtype != dtype or t.device != dev or not t.is_contiguous()):
        raise _err(f"{what} must be a contiguous {dtype} tensor of shape {shape} on {dev}, not {t.dtype} {tuple(t.shape)} on {t.device}")


@torch.no_grad()
def resize_batch(sources, size: Tuple[int, int], max_staged_bytes: int = 256 << 20, want_float: bool = False, device="cuda",
                 out: Optional[torch.Tensor] = None, out_float: Optional[torch.Tensor] = None):
    """`sources`: equally sized uint8 images — a sequence of (H, W), (H, W, 1) or (H, W, 3) host arrays or tensors, or ONE
    (n, H, W, C) array or tensor on the host or the device.  size = (width, height).  Returns the device uint8 tensor
    (n, Hout, Wout, C) and, with want_float (or out_float), also float32 (n, C, Hout, Wout) = bytes / 255.

    Host sources are staged, together with the tables, in one pinned buffer per chunk of at most max_staged_bytes and uploaded
    with one copy; a chunk is resized with at most two launches.  A device source is read in place: no copy, no host read."""
    stacked = isinstance(sources, (np.ndarray, torch.Tensor))
    if stacked:
        if sources.ndim != 4:
            raise _err(f"a stacked source has shape {tuple(sources.shape)}, not (n, H, W, C)")
        n, first_shape = int(sources.shape[0]), tuple(sources.shape[1:])
        _check_u8(sources, "the source")
    else:
        sources = list(sources)
        n = len(sources)
        if n == 0:
            raise _err("no image")
        first_shape = tuple(sources[0].shape)
        for i, s in enumerate(sources):
            _check_u8(s, f"image {i}")
            if tuple(s.shape) != first_shape:
                raise _err(f"image {i} has shape {tuple(s.shape)}, image 0 {first_shape}: a batch holds images of one size")
            if torch.is_tensor(s) and s.is_cuda:
                raise _err("a batch of device images is passed as ONE (n, H, W, C) tensor, which is read in place")
    if n < 1:
        raise _err("no image")
    H, W, Cn = _hwc(first_shape, "an image")
    on_device = stacked and torch.is_tensor(sources) and sources.is_cuda
    dev = sources.device if on_device else _device(device)
    plan = plan_of((W, H), (int(size[0]), int(size[1])), Cn)
    want_float = want_float or out_float is not None
    _check_out(out, (n, plan.hout, plan.wout, Cn), torch.uint8, dev, "out")
    _check_out(out_float, (n, Cn, plan.hout, plan.wout), torch.float32, dev, "out_float")

    if not plan.device_route:
        # beyond what the kernels take (a reduction of more than 32x): Pillow on the host, one upload
        if on_device:
            raise _err(f"{W} x {H} -> {plan.wout} x {plan.hout} is beyond the kernels (ksize > {MAX_KSIZE}) and the source is on "
                       "the device: resize it on the host")
        host = np.stack([_pillow_resize(np.asarray(s).reshape((H, W) if Cn == 1 else (H, W, Cn)), (plan.wout, plan.hout))
                         .reshape(plan.hout, plan.wout, Cn) for s in sources])
        u8 = torch.from_numpy(host).to(dev) if out is None else out.copy_(torch.from_numpy(host))
        if not want_float:
            return u8
        fl = (torch.from_numpy(host) / 255.0).permute(0, 3, 1, 2).contiguous()
        return u8, (fl.to(dev) if out_float is None else out_float.copy_(fl))

    if n > _lib_img.RESAMPLE_MAX_SIZE:
        raise _err(f"{n} images are more than one call takes")
    out = torch.empty((n, plan.hout, plan.wout, Cn), dtype=torch.uint8, device=dev) if out is None else out
    if want_float and out_float is None:
        out_float = torch.empty((n, Cn, plan.hout, plan.wout), dtype=torch.float32, device=dev)

    if on_device:
        src = sources if sources.is_contiguous() else sources.contiguous()
        _launch(plan, n, src.data_ptr(), plan.device_tables(dev), 0, out, out_float, dev)
    else:
        per = max(1, min(n, (int(max_staged_bytes) - plan.tables.size) // max(plan.image_bytes, 1)))
        for first in range(0, n, per):
            m = min(per, n - first)
            staged = torch.empty(plan.staged_bytes(m), dtype=torch.uint8, pin_memory=True)
            view = staged.numpy()
            for i in range(m):                                                      # the staging copy
                s = sources[first + i]
                s = s.numpy() if torch.is_tensor(s) else np.asarray(s)
                view[i * plan.image_bytes:(i + 1) * plan.image_bytes] = s.reshape(-1)
            toff = plan.tables_offset(m)
            view[toff:] = plan.tables
            upload = staged.to(dev, non_blocking=True)                              # the chunk's ONE upload
            _launch(plan, m, upload.data_ptr(), upload, toff, out[first:first + m],
                    out_float[first:first + m] if out_float is not None else None, dev)
    return (out, out_float) if want_float else out


@torch.no_grad()
def resize_u8(src: Source, size: Tuple[int, int], out: Optional[torch.Tensor] = None, out_float: Optional[torch.Tensor] = None,
              stream: Optional[torch.cuda.Stream] = None, device="cuda") -> torch.Tensor:
    """Pillow's `Image.fromarray(src).resize(size)` on the GPU.  src: uint8 (H, W), (H, W, 1) or (H, W, 3), array or tensor, on
    the host (staged with the tables in one pinned buffer, one upload) or on the device (read in place; the tables are uploaded
    on the first call of a size and kept).  size = (width, height).  Returns the device uint8 tensor of the resized shape (`out`
    when given); out_float, float32 (C, Hout, Wout), receives bytes / 255 in the same launch.  The launches go to `stream`
    (default: the current one)."""
    _check_u8(src, "the source")
    H, W, Cn = _hwc(src.shape, "the source")
    shape = (int(size[1]), int(size[0])) + tuple(src.shape[2:])
    on_device = torch.is_tensor(src) and src.is_cuda
    dev = src.device if on_device else _device(device)
    _check_out(out, shape, torch.uint8, dev, "out")
    _check_out(out_float, (Cn, shape[0], shape[1]), torch.float32, dev, "out_float")
    if on_device:
        batch = src.reshape(1, H, W, Cn)
    else:
        batch = (src.numpy() if torch.is_tensor(src) else np.asarray(src)).reshape(1, H, W, Cn)
    kw = dict(device=dev, out=None if out is None else out.view(1, shape[0], shape[1], Cn),
              out_float=None if out_float is None else out_float.view(1, Cn, shape[0], shape[1]))
    if stream is None:
        res = resize_batch(batch, size, **kw)
    else:
        with torch.cuda.stream(stream):
            res = resize_batch(batch, size, **kw)
    u8 = res[0] if isinstance(res, tuple) else res
    return u8.view(shape)


def _check_decode(decode) -> bool:
    if decode not in (None, "device"):
        raise _err(f'decode must be None or "device", not {decode!r}')
    return decode == "device"


def lazily_opened_jpeg(pil_image) -> bool:
    """Is this what Image.open gives for a JPEG file before anything loaded its pixels: format JPEG, a file name, mode RGB or L,
    no pixel storage yet?"""
    name = getattr(pil_image, "filename", None)
    storage = vars(pil_image).get("_im", vars(pil_image).get("im"))          # (`im` is a property that asserts in newer Pillows)
    return (getattr(pil_image, "format", None) == "JPEG" and isinstance(name, (str, os.PathLike)) and bool(name)
            and pil_image.mode in ("L", "RGB") and storage is None and os.path.isfile(name))


@torch.no_grad()
def pil_to_torch(pil_image, resolution, device="cuda", decode=None) -> torch.Tensor:
    """The drop-in for PILtoTorch (utils/general_utils.py:22-28): float32 (C, H, W) on `device`, the tensor
    `PILtoTorch(pil_image, resolution).to(device)` gives.  Modes `L` and `RGB` take the kernels; every other mode (and a reduction
    beyond 32x) is resized by Pillow on the host and uploaded once.  decode="device": a lazily opened JPEG file is read from disk
    and decoded on the GPU (jpeg_decode.decode; a file the decoder refuses comes back from Pillow, the same bytes), then resized
    where it lies.  decode=None is the route above, unchanged."""
    dev = _device(device)
    w, h = int(resolution[0]), int(resolution[1])
    if _check_decode(decode) and lazily_opened_jpeg(pil_image):
        Cn = 1 if pil_image.mode == "L" else 3
        if plan_of((pil_image.size[0], pil_image.size[1]), (w, h), Cn).device_route:
            from . import jpeg_decode
            u8 = jpeg_decode.decode(pil_image.filename, dev)
            if u8.dtype == torch.uint8 and tuple(u8.shape[:2]) == (pil_image.size[1], pil_image.size[0]) and u8.dim() == (2 if Cn == 1 else 3):
                fl = torch.empty((Cn, h, w), dtype=torch.float32, device=dev)
                resize_u8(u8, (w, h), out_float=fl, device=dev)
                return fl
    if pil_image.mode in ("L", "RGB"):
        arr = np.asarray(pil_image)
        Cn = 1 if arr.ndim == 2 else arr.shape[2]
        if arr.dtype == np.uint8 and plan_of((arr.shape[1], arr.shape[0]), (w, h), Cn).device_route:
            fl = torch.empty((Cn, h, w), dtype=torch.float32, device=dev)
            resize_u8(arr, (w, h), out_float=fl, device=dev)
            return fl
    resized = torch.from_numpy(np.array(pil_image.resize((w, h)))) / 255.0
    if len(resized.shape) == 3:
        return resized.permute(2, 0, 1).to(dev)
    return resized.unsqueeze(dim=-1).permute(2, 0, 1).to(dev)


@torch.no_grad()
def load_image(path, resolution, device="cuda") -> torch.Tensor:
    """The direct form: the file at `path` as float32 (C, h, w) on `device`, resolution = (w, h) — the tensor
    `PILtoTorch(Image.open(path), resolution).to(device)` gives.  A baseline JPEG is decoded and resized on the GPU; anything else
    takes pil_to_torch's other routes."""
    from PIL import Image
    with Image.open(path) as im:
        return pil_to_torch(im, resolution, device=device, decode="device")


def install(module, decode=None):
    """Rebind `PILtoTorch` in `module` — utils.camera_utils, which imports the name and calls it from loadCam — to pil_to_torch
    (with decode="device": to pil_to_torch with that argument).  Returns the function that was bound before."""
    old = getattr(module, "PILtoTorch", None)
    if _check_decode(decode):
        module.PILtoTorch = functools.partial(pil_to_torch, decode="device")
    else:
        module.PILtoTorch = pil_to_torch
    return old


@torch.no_grad()
def load_images(paths, resolutions, device="cuda") -> List[torch.Tensor]:
    """[load_image(p, r) for p, r in zip(paths, resolutions)], bit for bit, with the JPEG files decoded by ONE
    jpeg_decode.decode_batch (one upload, one host read for the list) and resized by one resize_batch(..., want_float=True) per
    group of equal (source shape, target size), read where the decoder left them.  resolutions: one (w, h) or one per path.  A file
    that is no JPEG, a file the decoder refuses and a reduction beyond the resize kernels take load_image's routes."""
    from PIL import Image
    from . import jpeg_decode
    dev = _device(device)
    paths = list(paths)
    if len(resolutions) == 2 and not isinstance(resolutions[0], (tuple, list)):
        resolutions = [resolutions] * len(paths)
    resolutions = [(int(r[0]), int(r[1])) for r in resolutions]
    if len(resolutions) != len(paths):
        raise _err(f"{len(resolutions)} resolutions for {len(paths)} paths")
    results: List[Optional[torch.Tensor]] = [None] * len(paths)
    batch = []                                                                    # (index, expected u8 shape)
    for i, (path, res) in enumerate(zip(paths, resolutions)):
        with Image.open(path) as im:
            if lazily_opened_jpeg(im):
                Cn = 1 if im.mode == "L" else 3
                if plan_of((im.size[0], im.size[1]), res, Cn).device_route:
                    batch.append((i, (im.size[1], im.size[0]) + ((3,) if Cn == 3 else ())))
    decoded = jpeg_decode.decode_batch([paths[i] for i, _shape in batch], dev) if batch else []
    groups: Dict[tuple, List[Tuple[int, torch.Tensor]]] = {}
    for (i, shape), u8 in zip(batch, decoded):
        if u8.dtype == torch.uint8 and tuple(u8.shape) == shape:
            groups.setdefault((shape, resolutions[i]), []).append((i, u8))
    for (shape, res), members in groups.items():
        H, W, Cn = _hwc(shape, "an image")
        tensors = [u8 for _i, u8 in members]
        nbytes = H * W * Cn
        first = tensors[0]
        same = all(t.untyped_storage().data_ptr() == first.untyped_storage().data_ptr() and t.is_contiguous()
                   and t.storage_offset() == first.storage_offset() + k * nbytes for k, t in enumerate(tensors))
        if same:                                                                  # side by side where the decoder wrote them
            stacked = torch.as_strided(first, (len(tensors), H, W, Cn), (nbytes, W * Cn, Cn, 1), first.storage_offset())
        else:
            stacked = torch.stack([t.reshape(H, W, Cn) for t in tensors])
        _u8, fl = resize_batch(stacked, res, want_float=True)
        for k, (i, _t) in enumerate(members):
            results[i] = fl[k]
    for i, (path, res) in enumerate(zip(paths, resolutions)):
        if results[i] is None:
            results[i] = load_image(path, res, device=dev)
    return results


def install_batched(module):
    """Rebind `cameraList_from_camInfos` in `module` (utils.camera_utils): the lazily opened JPEG files among cam_infos are loaded
    with ONE load_images call at the sizes loadCam will ask for (target_resolution), then the module's own loop runs with PILtoTorch
    bound to a function that serves those tensors by (file name, resolution) and calls pil_to_torch for anything else.  Returns
    the function that was bound before, as install does."""
    old = module.cameraList_from_camInfos

    def cameraList_from_camInfos(cam_infos, resolution_scale, args):
        cam_infos = list(cam_infos)
        wanted: Dict[tuple, None] = {}
        for c in cam_infos:
            im = getattr(c, "image", None)
            if im is not None and lazily_opened_jpeg(im):
                res = target_resolution(im.size[0], im.size[1], args.resolution, resolution_scale)
                wanted[(os.fspath(im.filename), (int(res[0]), int(res[1])))] = None
        keys = list(wanted)
        ready = dict(zip(keys, load_images([k[0] for k in keys], [k[1] for k in keys]))) if keys else {}

        def serve(pil_image, resolution):
            name = getattr(pil_image, "filename", None)
            key = (os.fspath(name), (int(resolution[0]), int(resolution[1]))) if isinstance(name, (str, os.PathLike)) and name else None
            if key in ready:
                return ready[key]
            return pil_to_torch(pil_image, resolution)

        before = getattr(module, "PILtoTorch", None)
        module.PILtoTorch = serve
        try:
            return old(cam_infos, resolution_scale, args)
        finally:
            module.PILtoTorch = before

    module.cameraList_from_camInfos = cameraList_from_camInfos
    return old

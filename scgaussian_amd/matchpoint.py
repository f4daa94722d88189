"""GaussianModel.save_ply_at_matchpoint on the GPU (csrc/matchpoint.hip, libscg_mp.so): the init stage's snapshot in four launches
and ONE device-to-host copy.

The reference (scene/gaussian_model.py:611-642; scene.save_init, train.py:97) loops over the ordered view pairs in Python: per pair an
index_put into the view's sparse depth image; per view a synchronising copy for np.save, a min() / max() and a second copy inside
torchvision's save_image; at the end two concatenations, two more copies and one Python tuple per match inside storePly.  It needs
torchvision and plyfile.  Every match is decided from that match alone and every pixel from its winning match and two scalars of
its view, so here the matched point cloud, every view's sparse depth plane, its normalised 8-bit plane and its (min, max) are
built where the arena lies, views of unequal size included:

    from scgaussian_amd import matchpoint
    matchpoint.install(gaussians, stage)             # gaussians.save_ply_at_matchpoint now runs here: scene.save_init(2000) unchanged

    snap = matchpoint.pack(matchpoint.MatchpointInputs.from_view_gs(gaussians.view_gs, stage))     # four launches, no host read
    snap.to_host()                                   # the ONE device-to-host copy, into pinned memory
    snap.write(path)                                 # <path> (the PLY), <key>.npy and sparsedepth_<key>.png next to it

Where several matches of one view fall on one pixel the match latest in arena order wins: what the reference gives wherever it is
defined (a later pair overwrites an earlier one) and what its index_put gives on the CPU within a pair.  A match whose uv is not
finite is in the point cloud but writes no depth (the seeding step's rule).  The inputs are read only.

There is no CPU path: CPU tensors raise ScgError.
"""
from __future__ import annotations

import ctypes as C
import functools
import os
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _arena, _lib, _lib_mp, ply

RECORD_BYTES = _lib_mp.MP_RECORD_BYTES
_SEG_DTYPE = np.dtype(_lib.ScgSeedSegment)
_VIEW_DTYPE = np.dtype(_lib_mp.ScgMpView)
_WHAT = "matchpoint: the snapshot"                   # ... needs tensors on the GPU (_lib.stream_of)


def _err(msg: str):
    return _lib.ScgError("matchpoint: " + msg)


def _flat(t: torch.Tensor, tail: Tuple[int, ...], dev) -> torch.Tensor:
    _lib.stream_of(t, _WHAT)
    return t.detach().to(device=dev, dtype=torch.float32).reshape((-1,) + tail)


def layout_of(N: int, sizes: Sequence[Tuple[int, int]]):
    """(ScgMpLayout, the view table as a numpy record array) for N matches and the views' (H, W): the library's arithmetic."""
    V = len(sizes)
    if V < 1 or V > _lib_mp.MP_MAX_VIEWS:
        raise _err(f"{V} views are outside what the kernels take (1..{_lib_mp.MP_MAX_VIEWS})")
    hw = np.ascontiguousarray(np.asarray(sizes, dtype=np.int64).reshape(V, 2))
    if (hw < 1).any() or (hw > _lib_mp.MP_MAX_DIM).any():
        raise _err(f"a view's height or width is outside 1..{_lib_mp.MP_MAX_DIM}")
    hw = hw.astype(np.int32)
    lay = _lib_mp.ScgMpLayout()
    views = np.zeros(V, dtype=_VIEW_DTYPE)
    _lib_mp.check(_lib_mp.load().scg_mp_layout(int(N), V, hw.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(lay),
                                               views.ctypes.data_as(C.POINTER(_lib_mp.ScgMpView))), "scg_mp_layout")
    return lay, views


class MatchpointInputs:
    """What save_ply_at_matchpoint reads per match, flat in arena order: rays_o, rays_d, color (N,3), uv (N,2), z, cam_z (N); the
    segment table (host and device) with each segment's source view; the views' names and sizes and the view table (host and
    device).  Every view keeps its own (H, W)."""

    def __init__(self, segments, table_host, table_dev, keys, sizes, color, uv, cam_z, rays_o, rays_d, z, stage):
        self.segments: List[Tuple[object, object, int, int]] = segments
        self.table_host, self.table_dev = table_host, table_dev
        self.keys, self.sizes = list(keys), [(int(h), int(w)) for h, w in sizes]
        self.color, self.uv, self.cam_z, self.rays_o, self.rays_d, self.z = color, uv, cam_z, rays_o, rays_d, z
        self.stage = stage
        if len(self.keys) != len(self.sizes):
            raise _err(f"{len(self.keys)} view names but {len(self.sizes)} sizes")
        if not segments or self.N == 0:
            raise _err("the model holds no match pair")               # the reference's torch.cat([]) raises too
        if len(segments) > _lib_mp.MP_MAX_SEGMENTS:
            raise _err(f"{len(segments)} ordered view pairs are more than the kernels take ({_lib_mp.MP_MAX_SEGMENTS})")
        if self.N >= 2 ** 31:
            raise _err(f"{self.N} matches are more than the kernels take")
        dev = z.device
        _lib.stream_of(dev, _WHAT)
        self.layout, self.views_host = layout_of(self.N, self.sizes)
        self.views_dev = _arena.upload_table(self.views_host, dev)

    @property
    def N(self) -> int:
        return self.z.numel()

    @property
    def V(self) -> int:
        return len(self.keys)

    @classmethod
    def from_view_gs(cls, view_gs: Dict, stage=None) -> "MatchpointInputs":
        """Given `stage` (the InitStage of this view_gs), its rays_o, rays_d and z are shared, not copied: the inputs can be packed
        before the stage runs and see its result.  Without it they are concatenated from view_gs as it is now."""
        keys, pairs = _arena.walk(view_gs)
        if not keys:
            raise _err("view_gs holds no view")
        if not pairs:
            raise _err("the model holds no match pair")
        sizes = [(int(view_gs[k]["height"]), int(view_gs[k]["width"])) for k in keys]
        segments, infos = [p[:4] for p in pairs], [p[4] for p in pairs]
        off = pairs[-1][2] + pairs[-1][3]
        if stage is not None and list(stage.segments) != segments:
            raise _err("the init stage was packed from another view_gs (its segments differ)")
        dev = stage.z.device if stage is not None else infos[0]["rays_o"].device
        _lib.stream_of(dev, _WHAT)
        cat = lambda key, tail: torch.cat([_flat(i[key], tail, dev) for i in infos]).contiguous()      # noqa: E731
        color, uv = cat("color", (3,)), cat("uv", (2,))
        cam_z = torch.cat([_flat(i["cam_rays_d"], (3,), dev)[:, 2] for i in infos]).contiguous()
        for name, t in (("color", color), ("uv", uv), ("cam_rays_d", cam_z)):
            if t.shape[0] != off:
                raise _err(f"{name} holds {t.shape[0]} rows, rays_o {off}")
        if stage is not None:
            rays_o, rays_d, z = stage.rays_o, stage.rays_d, stage.z
        else:
            rays_o, rays_d, z = cat("rays_o", (3,)), cat("rays_d", (3,)), cat("z_val", ())
            if z.shape[0] != off or rays_d.shape[0] != off:
                raise _err(f"z_val / rays_d hold {z.shape[0]} / {rays_d.shape[0]} rows, rays_o {off}")
        rec = np.zeros(len(segments), dtype=_SEG_DTYPE)
        rec["offset"], rec["count"] = [s[2] for s in segments], [s[3] for s in segments]
        rec["view"] = [keys.index(s[0]) for s in segments]
        return cls(segments, rec, _arena.upload_table(rec, dev), keys, sizes, color, uv, cam_z, rays_o, rays_d, z, stage)

    @classmethod
    def from_mono(cls, setup, stage=None) -> "MatchpointInputs":
        """The inputs over the arena of a mono.MonoSetup, read in place: color, uv, cam_z and the segment table are the setup's own
        tensors, rays_o, rays_d and z the stage's (InitStage.from_mono(setup)) or, without one, the setup's.  No tensor is copied."""
        plan = setup.plan
        segments = list(setup.segments)
        if stage is not None and (list(stage.segments) != segments or stage.z.data_ptr() != setup.z.data_ptr()):
            raise _err("the init stage was packed from another setup (its segments or its arena differ)")
        _lib.stream_of(setup.z, _WHAT)
        rays_o, rays_d, z = (stage.rays_o, stage.rays_d, stage.z) if stage is not None else (setup.rays_o, setup.rays_d, setup.z)
        return cls(segments, plan.seed_table_host, setup.seed_table, setup.keys, [(c["H"], c["W"]) for c in plan.consts],
                   setup.color, setup.uv, setup.cam_z, rays_o, rays_d, z, stage)

    @classmethod
    def from_flat(cls, rays_o, rays_d, z, color, uv, cam_z, counts, seg_view, sizes, keys=None) -> "MatchpointInputs":
        """Inputs that already lie flat in arena order: counts[s] matches of source view seg_view[s] per segment; sizes: the
        views' (H, W); keys: their names (default 0 .. V-1).  The tensors are used as they are (pack validates them)."""
        if len(counts) != len(seg_view):
            raise _err(f"{len(counts)} segment sizes but {len(seg_view)} source views")
        segments, off = [], 0
        for s, (M, v) in enumerate(zip(counts, seg_view)):
            segments.append((int(v), s, off, int(M)))
            off += int(M)
        _lib.stream_of(z, _WHAT)
        rec = np.zeros(len(segments), dtype=_SEG_DTYPE)
        rec["offset"], rec["count"], rec["view"] = [s[2] for s in segments], [s[3] for s in segments], [int(v) for v in seg_view]
        return cls(segments, rec, _arena.upload_table(rec, z.device), list(keys) if keys is not None else list(range(len(sizes))),
                   sizes, color, uv, cam_z, rays_o, rays_d, z, None)


class MatchpointSnapshot:
    """The snapshot in ONE device buffer (include/mp/scg_matchpoint.h ScgMpLayout).  body: (N, 27) uint8, the PLY records; planes:
    per view the (H, W) fp32 sparse depth; byte_planes: per view the (H, W) uint8 normalised plane; ranges: (V, 2) fp32 (min, max).
    All are views of `buffer`; host_* are the same views of the host copy."""

    def __init__(self, N: int, keys, sizes, layout, views_host, buffer: torch.Tensor):
        self.N, self.keys, self.sizes, self.layout, self.views_host, self.buffer = N, keys, sizes, layout, views_host, buffer
        self.host: Optional[torch.Tensor] = None
        self.body, self.planes, self.byte_planes, self.ranges = self._carve(buffer)

    def _carve(self, buf: torch.Tensor):
        l = self.layout
        body = buf[l.body_offset:l.body_offset + self.N * RECORD_BYTES].view(self.N, RECORD_BYTES)
        depth = buf[l.depth_offset:l.depth_offset + l.depth_bytes].view(torch.float32)
        bytes_ = buf[l.byte_offset:l.byte_offset + l.byte_bytes]
        planes, byte_planes = [], []
        for (H, W), rec in zip(self.sizes, self.views_host):
            p, b = int(rec["first_pixel"]), int(rec["first_byte"])
            planes.append(depth[p:p + H * W].view(H, W))
            byte_planes.append(bytes_[b:b + H * W].view(H, W))
        ranges = buf[l.range_offset:l.range_offset + l.range_bytes].view(torch.float32).view(len(self.sizes), 2)
        return body, planes, byte_planes, ranges

    def to_host(self) -> torch.Tensor:
        """The step's one device-to-host copy: the whole buffer in one transfer into pinned memory."""
        if self.host is None:
            self.host = self.buffer.to("cpu", non_blocking=True)             # (a non-blocking copy to the host lands in pinned memory)
            torch.cuda.current_stream(self.buffer.device).synchronize()
        return self.host

    def host_views(self):
        """(body, planes, byte_planes, ranges) as numpy views of the host copy."""
        body, planes, byte_planes, ranges = self._carve(self.to_host())
        return body.numpy(), [p.numpy() for p in planes], [b.numpy() for b in byte_planes], ranges.numpy()

    def write(self, path: str, png: str = "pillow") -> None:
        """`path` receives the point cloud (scene.save_init passes .../point_cloud_matchpoint.ply); <key>.npy and
        sparsedepth_<key>.png of every view go next to it, as the reference places them.  The directory is created if missing.
        png="device" encodes the views' byte planes on the GPU in one batch (png.py) where the default, "pillow", encodes them on
        the host; both decode to the same pixels."""
        from . import png as _png
        from .evaluate import _save_png
        on_device = _png.check_route(png)
        body, planes, byte_planes, _ranges = self.host_views()
        folder = os.path.dirname(os.path.abspath(path))
        os.makedirs(folder, exist_ok=True)
        with open(path, "wb") as fh:
            fh.write(ply.header(ply.COLOR_NAMES, self.N, ply.COLOR_TYPES))
            fh.write(memoryview(body))
        for key, plane, q in zip(self.keys, planes, byte_planes):
            np.save(os.path.join(folder, f"{key}.npy"), plane)
            if not on_device:
                _save_png(os.path.join(folder, f"sparsedepth_{key}.png"), q)
        if on_device:
            _png.write_batch([os.path.join(folder, f"sparsedepth_{key}.png") for key in self.keys],
                             [p.contiguous() for p in self.byte_planes])


@torch.no_grad()
def pack(inputs: MatchpointInputs) -> MatchpointSnapshot:
    """Four launches, no host read: capturable in a graph at fixed counts (buffer and workspace come from the graph's pool)."""
    N, V = inputs.N, inputs.V
    stream = _lib.stream_of(inputs.z, _WHAT)
    dev = inputs.z.device
    for name, t, shape in (("rays_o", inputs.rays_o, (N, 3)), ("rays_d", inputs.rays_d, (N, 3)), ("z", inputs.z, (N,)),
                           ("color", inputs.color, (N, 3)), ("uv", inputs.uv, (N, 2)), ("cam_z", inputs.cam_z, (N,))):
        if t.device != dev or t.dtype != torch.float32 or tuple(t.shape) != shape or not t.is_contiguous():
            raise _err(f"{name} must be a contiguous fp32 tensor of shape {shape} on {dev}")
    lib = _lib_mp.load()
    lay = inputs.layout
    hw = np.ascontiguousarray(np.asarray(inputs.sizes, dtype=np.int32).reshape(V, 2))
    ws_bytes = lib.scg_mp_workspace_bytes(V, hw.ctypes.data_as(C.POINTER(C.c_int32)))
    if ws_bytes == 0:
        raise _err("the views hold more pixels than the kernels take")
    with torch.cuda.device(dev):
        buf = torch.empty(int(lay.total), dtype=torch.uint8, device=dev)
        ws = torch.empty(ws_bytes // 4, dtype=torch.int32, device=dev)
        a = _lib_mp.ScgMpPack()
        a.struct_bytes = C.sizeof(_lib_mp.ScgMpPack)
        a.N, a.V, a.nseg = N, V, len(inputs.segments)
        a.segments, a.segments_dev = inputs.table_host.ctypes.data, inputs.table_dev.data_ptr()
        a.views, a.views_dev = inputs.views_host.ctypes.data, inputs.views_dev.data_ptr()
        a.rays_o, a.rays_d, a.z, a.color, a.uv, a.cam_z = (t.data_ptr() for t in (inputs.rays_o, inputs.rays_d, inputs.z, inputs.color,
                                                                                 inputs.uv, inputs.cam_z))
        _lib_mp.check(lib.scg_mp_pack(C.byref(a), buf.data_ptr(), buf.numel(), ws.data_ptr(), ws_bytes, stream), "scg_mp_pack")
    return MatchpointSnapshot(N, inputs.keys, inputs.sizes, lay, inputs.views_host, buf)


def save_ply_at_matchpoint(gaussians, path: str, stage=None, inputs: Optional[MatchpointInputs] = None) -> None:
    """GaussianModel.save_ply_at_matchpoint(path) on `gaussians`, any object with a `view_gs`: pack + one copy + the writes.
    stage: the InitStage of this view_gs (its rays and depths are shared); inputs: a MatchpointInputs packed earlier."""
    if inputs is None:
        if not hasattr(gaussians, "view_gs"):
            raise _err("the model has no view_gs")
        setup = getattr(gaussians, "mono_setup", None)
        if setup is not None and setup.view_gs is gaussians.view_gs and (stage is None or stage.z.data_ptr() == setup.z.data_ptr()):
            inputs = MatchpointInputs.from_mono(setup, stage)
        else:
            inputs = MatchpointInputs.from_view_gs(gaussians.view_gs, stage)
    snap = pack(inputs)
    snap.to_host()
    snap.write(path)


def install(gaussians, stage=None) -> None:
    """Bind save_ply_at_matchpoint as a method of this model instance under the reference's name, so that scene.save_init
    (scene/__init__.py:177-179, train.py:97) runs unchanged, and without torchvision or plyfile; `stage` (an InitStage) is kept and
    its arena tensors are used in place."""
    gaussians.save_ply_at_matchpoint = functools.partial(save_ply_at_matchpoint, gaussians, stage=stage)

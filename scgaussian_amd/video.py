"""Depth colour maps and video frames: the reference's `visualization(depth, path)` and render_video.py's `render_set`, host side
(csrc/depthviz.hip, include/scg_viz.h).

    render.py:97-110,162, render_video.py:98-113,146   np.percentile(depth, 98), depth.min(), matplotlib's Normalize and turbo
                                                       table, the truncating byte cast            -> DepthColorizer
    render_video.py:129-152                            render, clamp, normalised depth, the PNGs, the two video frames
                                                                                                  -> render_video

The reference leaves the GPU twice per frame (the normalised depth and the clamped rendering), partitions the whole image on one
core and maps it through a float64 RGBA image.  Every pixel is decided from that pixel and two scalars of the image, its minimum
and one percentile: here a frame is an exact selection (scg_viz_select) and one per-pixel launch (scg_viz_frame), nothing is read
on the host, and a whole video is ONE copy to the host after the loop.  cv2 and the .mp4 container are not part of this: the
frames go to two caller-supplied sinks (`cv2.VideoWriter.write` fits them), and with video="mjpeg" the two videos are written as
Motion-JPEG AVI files whose frames are encoded on the GPU (jpeg.py).  CPU tensors raise ScgError."""
from __future__ import annotations

import os

import numpy as np
import torch

from . import _lib
from . import render as _render
from ._lib import check

# matplotlib 3.10.8: trunc(colormaps['turbo'](i)[:3] * 255), i = 0..255.  Data, because matplotlib may be absent where this runs;
# tests/test_depthviz_cpu.py holds it against the library where it is installed.
TURBO = np.fromfile(os.path.join(os.path.dirname(os.path.abspath(__file__)), "turbo256.rgb"), dtype=np.uint8).reshape(256, 3)
TURBO.setflags(write=False)


def _as_lut(lut) -> np.ndarray:
    lut = np.ascontiguousarray(lut.detach().cpu().numpy() if isinstance(lut, torch.Tensor) else lut)
    if lut.dtype != np.uint8 or lut.shape != (256, 3):
        raise ValueError("lut must be a 256x3 uint8 table")
    return lut


class DepthColorizer:
    """The colour map of (H,W) planes: owns the select scratch, the four stats, the NaN count and the device copy of the table.
    Every method is stream-ordered, reads nothing on the host and can be captured in a graph.  After `stats` / `colorize`,
    `.vmin` and `.vmax` are device scalars (views of the stats buffer: the next call overwrites them)."""

    def __init__(self, H: int, W: int, lut=TURBO, percentile: float = 98.0, device="cuda"):
        self.device = torch.device(device)
        _lib.stream_of(self.device, "DepthColorizer")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        lib = _lib.load()
        self.H, self.W, self.n, self.percentile = int(H), int(W), int(H) * int(W), float(percentile)
        if self.H < 1 or self.W < 1:
            raise ValueError("H and W must be at least 1")
        need = lib.scg_viz_select_scratch_bytes(self.n)
        if need == 0:
            raise _lib.ScgError(f"DepthColorizer: {H} x {W} is out of range (at most 2^24 pixels)")
        if not 0.0 <= self.percentile <= 100.0:
            raise ValueError("percentile must be in [0, 100]")
        with torch.cuda.device(self.device):
            self._nbytes = max(need, lib.scg_eval_depth_range_scratch_bytes(self.n))
            self._scratch = torch.empty((self._nbytes,), dtype=torch.uint8, device=self.device)
            self._stats = torch.zeros((4,), dtype=torch.float32, device=self.device)
            self._nan = torch.zeros((1,), dtype=torch.int32, device=self.device)
            self._range = torch.empty((2,), dtype=torch.float32, device=self.device)
            self.lut = torch.from_numpy(_as_lut(lut).copy()).to(self.device)
        self.vmin, self.vmax, self.nan_count = self._stats[0], self._stats[1], self._nan[0]

    def _plane(self, depth):
        d = depth.detach()
        _lib.stream_of(d, "DepthColorizer")
        d = d.to(self.device).float().contiguous()
        if d.numel() != self.n:
            raise ValueError(f"depth must be ({self.H},{self.W}) or (1,{self.H},{self.W})")
        return d

    def _range_of(self, range):
        if range is None:
            return None
        if range.dtype != torch.float32 or range.numel() != 2 or not range.is_contiguous() or range.device != self.device:
            raise ValueError("range must be 2 contiguous fp32 on the colorizer's device")
        return range

    def _out(self, t, shape, what):
        if t is None:
            return None
        if t.dtype != torch.uint8 or tuple(t.shape) != shape or not t.is_contiguous() or t.device != self.device:
            raise ValueError(f"{what} must be contiguous uint8 {shape} on the colorizer's device")
        return t

    def depth_range(self, depth):
        """The (min, max) of a raw depth map as two device floats (scg_eval_depth_range), in the colorizer's own buffer."""
        d = self._plane(depth)
        stream = _lib.stream_of(d, "DepthColorizer.depth_range")
        with torch.cuda.device(self.device):
            check(_lib.load().scg_eval_depth_range(d.data_ptr(), self.n, self._range.data_ptr(), self._scratch.data_ptr(), self._nbytes,
                                                   stream), "scg_eval_depth_range")
        return self._range

    def _select(self, d, rng, stream):
        check(_lib.load().scg_viz_select(d.data_ptr(), _lib.ptr(rng), self.n, self.percentile, self._stats.data_ptr(),
                                         self._nan.data_ptr(), self._scratch.data_ptr(), self._nbytes, stream), "scg_viz_select")

    def stats(self, depth, range=None):
        """(vmin, vmax, a, b) of x as four device floats: x = depth, or (depth - range[0]) / (range[1] - range[0]) with `range`."""
        d, rng = self._plane(depth), self._range_of(range)
        with torch.cuda.device(self.device):
            self._select(d, rng, _lib.stream_of(d, "DepthColorizer.stats"))
        return self._stats

    def frame(self, depth, range=None, render=None, depth_color=None, depth_color_bgr=None, depth_u8=None, render_u8=None,
              frame_bgr=None):
        """Select, then every requested 8-bit image of the frame in one launch (scg_viz_frame), into the caller's buffers.
        `depth_color` is allocated when None and returned."""
        d, rng = self._plane(depth), self._range_of(range)
        stream = _lib.stream_of(d, "DepthColorizer.frame")
        H, W = self.H, self.W
        r = None
        if render is not None:
            r = render.detach().to(self.device).float().contiguous()
            if tuple(r.shape) != (3, H, W):
                raise ValueError(f"render must be (3,{H},{W})")
        elif render_u8 is not None or frame_bgr is not None:
            raise ValueError("render_u8 and frame_bgr need a render")
        with torch.cuda.device(self.device):
            if depth_color is None:
                depth_color = torch.empty((H, W, 3), dtype=torch.uint8, device=self.device)
            outs = [self._out(depth_color, (H, W, 3), "depth_color"), self._out(depth_color_bgr, (H, W, 3), "depth_color_bgr"),
                    self._out(depth_u8, (H, W), "depth_u8"), self._out(render_u8, (H, W, 3), "render_u8"),
                    self._out(frame_bgr, (H, W, 3), "frame_bgr")]
            self._select(d, rng, stream)
            check(_lib.load().scg_viz_frame(_lib.ptr(r), d.data_ptr(), _lib.ptr(rng), self._stats.data_ptr(), self._nan.data_ptr(),
                                            self.lut.data_ptr(), H, W, *[_lib.ptr(o) for o in outs], stream), "scg_viz_frame")
        return depth_color

    def colorize(self, depth, range=None, bgr=False, out=None):
        """visualization(x): the (H,W,3) uint8 colour map of x on the device, R, G, B — or B, G, R with `bgr` —, into `out` when
        given."""
        if not bgr:
            return self.frame(depth, range, depth_color=out)
        with torch.cuda.device(self.device):
            out = torch.empty((self.H, self.W, 3), dtype=torch.uint8, device=self.device) if out is None else out
        self.frame(depth, range, depth_color_bgr=out)
        return out

    def colorize_depth(self, depth, bgr=False, out=None):
        """The one-shot form on a RAW depth map: its own min / max first (render.py:143), then the colour map of the normalised
        depth."""
        return self.colorize(depth, self.depth_range(depth), bgr=bgr, out=out)


def colorize_depth(depth, lut=TURBO, percentile: float = 98.0, bgr=False):
    """visualization((depth - depth.min()) / (depth.max() - depth.min())) of one raw (H,W) or (1,H,W) depth map on the GPU."""
    _lib.stream_of(depth, "colorize_depth")
    H, W = depth.shape[-2:]
    return DepthColorizer(H, W, lut=lut, percentile=percentile, device=depth.device).colorize_depth(depth, bgr=bgr)


VIDEO_KEYS = ("renders", "depth", "depth_color", "frames_bgr", "depth_frames_bgr")


def render_video(views, gaussians, pipe, background, out_dir=None, name="video", iteration=0, render=_render.render,
                 frame_sink=None, depth_sink=None, lut=TURBO, percentile: float = 98.0, png="pillow", video=None, fps=30,
                 jpeg_quality: int = 90, jpeg_subsampling: str = "4:2:0"):
    """render_video.py:129-152 over `views` under torch.no_grad().  Per frame: render, the depth's range, the select and the frame
    kernel — at most eight launches behind the rasteriser's and no host read —, written into buffers allocated before the loop;
    after the loop ONE copy to the host.  Returns a dict of uint8 numpy arrays over the F frames:
        renders (F,H,W,3)            q(clamp(render, 0, 1)): renders/{idx:05d}.png
        depth (F,H,W)                q of the normalised depth: depth/{idx:05d}.png
        depth_color (F,H,W,3)        its colour map, R, G, B: depth/color_{idx:05d}.png
        frames_bgr (F,H,W,3)         (clamp(render) * 255.).astype(uint8)[..., ::-1]: the frames of render_video.mp4
        depth_frames_bgr (F,H,W,3)   depth_color[..., ::-1]: the frames of depth_video.mp4
    With `out_dir` the three PNGs per frame are written under <out_dir>/<name>/ours_<iteration>/{renders,depth}/.  `frame_sink` and
    `depth_sink` are called with each frame's B, G, R array in order (cv2.VideoWriter.write fits them); no video library is
    imported and no .mp4 is written here.  All views must have one size, as the reference's single VideoWriter size implies.
    video="mjpeg" (with `out_dir`) encodes frames_bgr and depth_frames_bgr as JPEG files on the GPU in one batch behind the loop
    (jpeg.py, bgr=True, `jpeg_quality`, `jpeg_subsampling`; two more host reads) and writes them as the frames of
    <out_dir>/<name>/ours_<iteration>/render_video.avi and depth_video.avi at `fps`; the default, None, writes no video.
    png="device" encodes the 3 F files on the GPU in one batch behind the loop (png.py; two more host reads) and writes the same
    tree; every file decodes to the pixels that the default, "pillow", writes."""
    from . import png as _png
    from . import jpeg as _jpeg
    from .evaluate import _save_png
    on_device = _png.check_route(png)
    mjpeg = _jpeg.check_route(video) and out_dir is not None
    if video is not None:
        _jpeg.check_options(jpeg_quality, jpeg_subsampling, fps)      # before the first launch
    views = list(views)
    if not views:
        raise ValueError("render_video needs at least one view")
    H, W = int(views[0].image_height), int(views[0].image_width)
    for idx, v in enumerate(views):
        if (int(v.image_height), int(v.image_width)) != (H, W):
            raise ValueError(f"view {idx} is {int(v.image_height)}x{int(v.image_width)}, the video is {H}x{W}: all views must have one size")
    dev, F, n = background.device, len(views), H * W
    with torch.no_grad():
        viz = DepthColorizer(H, W, lut=lut, percentile=percentile, device=dev)
        with torch.cuda.device(dev):
            sizes = [F * n * (1 if k == "depth" else 3) for k in VIDEO_KEYS]
            starts = [0]
            for s in sizes:
                starts.append((starts[-1] + s + 15) // 16 * 16)
            flat = torch.empty((starts[-1],), dtype=torch.uint8, device=dev)
            buf = {k: flat[o:o + s].view((F, H, W) if k == "depth" else (F, H, W, 3)) for k, o, s in zip(VIDEO_KEYS, starts, sizes)}
        for idx, view in enumerate(views):
            pkg = render(view, gaussians, pipe, background)
            depth = pkg["rendered_depth"]
            viz.frame(depth, viz.depth_range(depth), render=pkg["render"], depth_color=buf["depth_color"][idx],
                      depth_color_bgr=buf["depth_frames_bgr"][idx], depth_u8=buf["depth"][idx], render_u8=buf["renders"][idx],
                      frame_bgr=buf["frames_bgr"][idx])
        packed = None
        if out_dir is not None and on_device:
            packed = _png.encode([buf[k][idx] for idx in range(F) for k in ("renders", "depth", "depth_color")])
        movie = None
        if mjpeg:
            movie = _jpeg.encode([buf[k][idx] for k in ("frames_bgr", "depth_frames_bgr") for idx in range(F)], jpeg_quality,
                                 jpeg_subsampling, bgr=True)
        host = flat.cpu().numpy()          # the video's one host read
    out = {k: host[o:o + s].reshape((F, H, W) if k == "depth" else (F, H, W, 3)) for k, o, s in zip(VIDEO_KEYS, starts, sizes)}
    if out_dir is not None:
        base = os.path.join(out_dir, name, f"ours_{iteration}")
        for sub in ("renders", "depth"):
            os.makedirs(os.path.join(base, sub), exist_ok=True)
        if packed is not None:
            packed.write([os.path.join(base, sub, f"{pre}{idx:05d}.png") for idx in range(F)
                          for sub, pre in (("renders", ""), ("depth", ""), ("depth", "color_"))])
        for idx in range(0 if packed is None else F, F):
            _save_png(os.path.join(base, "renders", f"{idx:05d}.png"), out["renders"][idx])
            _save_png(os.path.join(base, "depth", f"{idx:05d}.png"), out["depth"][idx])
            _save_png(os.path.join(base, "depth", f"color_{idx:05d}.png"), out["depth_color"][idx])
        if movie is not None:
            files = movie.files()
            _jpeg.write_avi(os.path.join(base, "render_video.avi"), files[:F], fps, W, H)
            _jpeg.write_avi(os.path.join(base, "depth_video.avi"), files[F:], fps, W, H)
    for idx in range(F):
        if frame_sink is not None:
            frame_sink(out["frames_bgr"][idx])
        if depth_sink is not None:
            depth_sink(out["depth_frames_bgr"][idx])
    return out

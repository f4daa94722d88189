"""Test-set evaluation: the reference's render.py `render_set` and metrics.py `evaluate`, host side (csrc/evalview.hip).

    render.py:133-162    render, depth normalised by its own min / max, get_pixel_loss error map, five save_image calls
                                                                                        -> evaluate_view / render_set
    metrics.py:26-47     the PNGs read back, image * mask + (1 - mask), mask == 1.      -> evaluate_view (the masked images, S, K)
    metrics.py:86-116    11x11 SSIM, PSNR under the mask, set means, the two JSON files -> EvalSet.results / write_results

The reference makes a few dozen small launches and five synchronising copies per view, and a second process uploads the same pixels
again.  PNG is lossless, so what metrics.py computes is a function of the quantised pixels; here a view is at most six launches
(include/scg_eval.h) that read nothing on the host, and a whole set is ONE host read of a (views, 3) record buffer.  LPIPS needs
VGG weights this project does not carry: a caller who has them builds the metric with scgaussian_amd.lpips.Lpips (or brings any
other) and passes it as `lpips_fn`.  CPU tensors raise ScgError."""
from __future__ import annotations

import json
import math
import os

import torch

from . import _lib
from . import render as _render
from ._lib import check

RECORD_WORDS = 3          # one int64 row per view: S, K, and (sum |a - b|, sum of the SSIM map) as two fp32 in the third word
SUBDIRS = ("renders", "gt", "depth", "error_map", "dtumask")          # render.py:120-125


def _plane(t, H, W, what):
    t = t.detach().float().contiguous()
    if t.numel() != H * W:
        raise ValueError(f"{what} must be (H,W) or (1,H,W)")
    return t


def evaluate_view(rendering: torch.Tensor, gt: torch.Tensor, depth: torch.Tensor, dtumask=None, record=None):
    """One view of render_set + evaluate.  rendering (3,H,W) unclamped, gt (3,H,W), depth (H,W) or (1,H,W), dtumask (H,W) / (1,H,W)
    or None, all on the GPU; H, W >= 3.  Returns a dict of device tensors: `renders`, `gt` (H,W,3) uint8, `depth`, `error_map`,
    `dtumask` (H,W) uint8 (None without a mask) — what the reference's PNGs hold —, `error_map_f32` (H,W), `renders_masked` and
    `gt_masked` (3,H,W) fp32 — what metrics.py forms from the PNGs —, and `record`.  `record` is a row of RECORD_WORDS int64 in
    device memory (one is allocated when None) that receives S = sum (q_render - q_gt)^2 and K = their number under mask == 1, and
    in its third word the fp32 sum of the 11x11 SSIM map of the masked images.  The quantiser is torchvision's save_image;
    q(NaN) = 0.  No host read: capturable in a graph."""
    lib = _lib.load()
    stream = _lib.stream_of(rendering, "evaluate_view")
    if rendering.dim() != 3 or rendering.shape[0] != 3:
        raise ValueError("rendering must be (3,H,W)")
    a = rendering.detach().float().contiguous()
    dev = a.device
    b = gt.detach().to(dev).float().contiguous()
    if b.shape != a.shape:
        raise ValueError("rendering and gt shapes differ")
    _, H, W = a.shape
    d = _plane(depth.to(dev), H, W, "depth")
    m = None if dtumask is None else _plane(dtumask.to(dev), H, W, "dtumask")
    with torch.cuda.device(dev):
        if record is None:
            record = torch.zeros((RECORD_WORDS,), dtype=torch.int64, device=dev)
        if record.dtype != torch.int64 or record.numel() != RECORD_WORDS or not record.is_contiguous() or record.device != dev:
            raise ValueError(f"record must be {RECORD_WORDS} contiguous int64 on the images' device")
        u8 = lambda *shape: torch.empty(shape, dtype=torch.uint8, device=dev)          # noqa: E731
        out = {"renders": u8(H, W, 3), "gt": u8(H, W, 3), "depth": u8(H, W), "error_map": u8(H, W),
               "dtumask": None if m is None else u8(H, W),
               "error_map_f32": torch.empty((H, W), dtype=torch.float32, device=dev),
               "renders_masked": torch.empty_like(a), "gt_masked": torch.empty_like(a), "record": record}
        rng = torch.empty((2,), dtype=torch.float32, device=dev)
        nbytes = max(lib.scg_eval_depth_range_scratch_bytes(H * W), lib.scg_image_loss_scratch_bytes(3, H, W))
        scratch = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
        check(lib.scg_eval_depth_range(d.data_ptr(), H * W, rng.data_ptr(), scratch.data_ptr(), nbytes, stream), "scg_eval_depth_range")
        check(lib.scg_eval_view(a.data_ptr(), b.data_ptr(), d.data_ptr(), _lib.ptr(m), rng.data_ptr(), H, W,
                                out["renders"].data_ptr(), out["gt"].data_ptr(), out["depth"].data_ptr(),
                                out["error_map"].data_ptr(), _lib.ptr(out["dtumask"]), out["error_map_f32"].data_ptr(),
                                out["renders_masked"].data_ptr(), out["gt_masked"].data_ptr(), record.data_ptr(), stream),
              "scg_eval_view")
        # metrics.py:87: the 11x11 SSIM is the training loss's kernel on the two masked images; its two sums land in the third word
        check(lib.scg_image_loss_forward(out["renders_masked"].data_ptr(), out["gt_masked"].data_ptr(), 3, H, W,
                                         record.data_ptr() + 16, None, scratch.data_ptr(), nbytes, stream), "scg_image_loss_forward")
    return out


def psnr_from_sums(S: int, K: int) -> float:
    """metrics.py:89 from the integers, in fp64: 10 log10(255^2 K / S).  S == 0 gives inf (the reference's 1 / sqrt(0)), K == 0
    gives NaN (its mean of an empty selection)."""
    if K == 0:
        return float("nan")
    if S == 0:
        return float("inf")
    return 10.0 * math.log10(255.0 ** 2 * K / S)


def _mean32(values) -> float:
    return torch.tensor(values, dtype=torch.float32).mean().item()          # metrics.py:104-107


class EvalSet:
    """The metrics of a set of views with one host read.  Owns the (n_views, 3) record buffer; `add` evaluates a view into the
    next row, `results` reads the buffer and returns (full, per_view) with the keys of the reference's results.json /
    per_view.json: "SSIM" and "PSNR", and "LPIPS" and "AVG" when the set was built with an `lpips_fn` — a function of the two
    masked images as (1,3,H,W) tensors, called once per view, whose values join the same read."""

    def __init__(self, n_views: int, lpips_fn=None, device="cuda"):
        if n_views < 1:
            raise ValueError("n_views must be at least 1")
        self.device = torch.device(device)
        _lib.stream_of(self.device, "EvalSet")
        self.n_views, self.lpips_fn = int(n_views), lpips_fn
        self.records = torch.zeros((self.n_views, RECORD_WORDS), dtype=torch.int64, device=self.device)
        self.names, self.elements, self._lpips = [], [], []

    def add(self, name, rendering, gt, depth, dtumask=None):
        i = len(self.names)
        if i >= self.n_views:
            raise IndexError(f"the set was built for {self.n_views} views")
        out = evaluate_view(rendering, gt, depth, dtumask, record=self.records[i])
        self.names.append(str(name))
        self.elements.append(out["renders_masked"].numel())
        if self.lpips_fn is not None:
            v = self.lpips_fn(out["renders_masked"][None], out["gt_masked"][None])
            self._lpips.append(torch.as_tensor(v, dtype=torch.float32, device=self.device).reshape(-1)[:1])
        return out

    def _read(self):
        """The set's one host read: the records and, with an lpips_fn, its values, in one byte buffer."""
        n = len(self.names)
        parts = [self.records[:n].reshape(-1).view(torch.uint8)]
        if self._lpips:
            parts.append(torch.cat(self._lpips).contiguous().view(torch.uint8))
        host = torch.cat(parts).cpu()
        rec = host[:n * RECORD_WORDS * 8].view(torch.int64).reshape(n, RECORD_WORDS)
        lp = host[n * RECORD_WORDS * 8:].view(torch.float32).tolist() if self._lpips else None
        return rec, lp

    def results(self):
        rec, lp = self._read()
        return results_from_records(rec, self.names, self.elements, lp)


def results_from_records(records: torch.Tensor, names, elements, lpips=None):
    """(full, per_view) from host records (n, 3) int64, the views' names, their 3 * H * W and, optionally, their LPIPS values:
    metrics.py:86-111.  PSNR in fp64 from the integers, SSIM = ssim_sum / (3 H W); the lists then go through fp32 tensors as the
    reference's do.  With LPIPS, "AVG" per view is exp(mean(log([10^(-psnr / 10), sqrt(1 - ssim), lpips]))) and the set's "AVG" is
    the mean of the LPIPS values — metrics.py:107 as it stands."""
    rec = records.cpu().contiguous()
    sums = rec[:, 2:3].contiguous().view(torch.float32).reshape(-1, 2)
    ssims = [float(sums[i, 1]) / float(n) for i, n in enumerate(elements)]
    psnrs = [psnr_from_sums(int(rec[i, 0]), int(rec[i, 1])) for i in range(rec.shape[0])]
    lists = {"SSIM": ssims, "PSNR": psnrs}
    if lpips is not None:
        lists["LPIPS"] = [float(v) for v in lpips]
        avgs = []
        for p, s, l in zip(psnrs, ssims, lists["LPIPS"]):
            p32, s32 = torch.tensor(p, dtype=torch.float32), torch.tensor(s, dtype=torch.float32)
            t = torch.tensor([10 ** (-p32 / 10), math.sqrt(1 - s32), l], dtype=torch.float32)          # metrics.py:91
            avgs.append(torch.exp(torch.log(t).mean()).item())
        lists["AVG"] = avgs
    full = {k: _mean32(v) for k, v in lists.items()}
    if lpips is not None:
        full["AVG"] = _mean32(lists["LPIPS"])
    per_view = {k: dict(zip(names, torch.tensor(v, dtype=torch.float32).tolist())) for k, v in lists.items()}
    return full, per_view


def _save_png(path, arr):
    from PIL import Image
    if arr.ndim == 2:                                  # save_image writes a single channel as three equal ones
        arr = arr[:, :, None].repeat(3, axis=2)
    Image.fromarray(arr).save(path, format="PNG")


def render_set(views, gaussians, pipe, background, out_dir=None, name="test", iteration=0, render=_render.render, lpips_fn=None,
               color_depth=False, png="pillow"):
    """render.py:133-162 and metrics.py's evaluate over `views` under torch.no_grad().  A view needs what render() needs plus
    `original_image` and, optionally, `dtumask`.  Returns (full, per_view, images): the two dicts in the shape of results.json /
    per_view.json — keyed by the method "ours_<iteration>", the views named "<idx:05d>.png" — and per view the dict of uint8 device
    tensors.  With `out_dir` the reference's tree <out_dir>/<name>/ours_<iteration>/{renders,gt,depth,error_map,dtumask}/ is
    written with PIL from those tensors, copied to the host after the loop.  With `color_depth` every view's dict also holds
    `depth_color`, render.py:162's `visualization` of the normalised depth as an (H,W,3) uint8 device tensor (video.DepthColorizer),
    written as depth/color_<idx:05d>.png; the default leaves every result, file and key as without it.  The colour point cloud of
    render.py is not part of this.  png="device" writes the same tree with the files encoded on the GPU (png.py): all images of
    the call in one batch after the loop, two host reads; every file decodes to the pixels that the default, "pillow", writes."""
    from . import png as _png
    on_device = _png.check_route(png)
    views = list(views)
    method = f"ours_{iteration}"
    images = []
    colorizers = {}
    with torch.no_grad():
        es = EvalSet(max(len(views), 1), lpips_fn=lpips_fn, device=background.device)
        for idx, view in enumerate(views):
            pkg = render(view, gaussians, pipe, background)
            out = es.add(f"{idx:05d}.png", pkg["render"], view.original_image[0:3, :, :], pkg["rendered_depth"],
                         getattr(view, "dtumask", None))
            images.append({k: out[k] for k in ("renders", "gt", "depth", "error_map", "dtumask")})
            if color_depth:
                from .video import DepthColorizer
                shape = tuple(out["depth"].shape)
                if shape not in colorizers:
                    colorizers[shape] = DepthColorizer(*shape, device=background.device)
                images[-1]["depth_color"] = colorizers[shape].colorize_depth(pkg["rendered_depth"])
        if out_dir is not None:
            base = os.path.join(out_dir, name, method)
            for sub in SUBDIRS:
                os.makedirs(os.path.join(base, sub), exist_ok=True)
            if on_device:
                paths, batch = [], []
                for idx, im in enumerate(images):
                    for sub, key in zip(SUBDIRS, ("renders", "gt", "depth", "error_map", "dtumask")):
                        if im[key] is not None:
                            paths.append(os.path.join(base, sub, f"{idx:05d}.png"))
                            batch.append(im[key])
                    if color_depth:
                        paths.append(os.path.join(base, "depth", f"color_{idx:05d}.png"))
                        batch.append(im["depth_color"])
                _png.write_batch(paths, [t.contiguous() for t in batch])
            host = [] if on_device else [{k: None if v is None else v.to("cpu", non_blocking=True) for k, v in im.items()}
                                         for im in images]
            torch.cuda.synchronize(background.device)
            for idx, im in enumerate(host):
                for sub, key in zip(SUBDIRS, ("renders", "gt", "depth", "error_map", "dtumask")):
                    if im[key] is not None:
                        _save_png(os.path.join(base, sub, f"{idx:05d}.png"), im[key].numpy())
                if color_depth:
                    _save_png(os.path.join(base, "depth", f"color_{idx:05d}.png"), im["depth_color"].numpy())
        full, per_view = es.results() if views else ({}, {})
    return {method: full}, {method: per_view}, images


def write_results(model_path, full, per_view):
    """metrics.py:113-116: <model_path>/results.json and per_view.json."""
    os.makedirs(model_path, exist_ok=True)
    with open(os.path.join(model_path, "results.json"), "w") as fp:
        json.dump(full, fp, indent=True)
    with open(os.path.join(model_path, "per_view.json"), "w") as fp:
        json.dump(per_view, fp, indent=True)

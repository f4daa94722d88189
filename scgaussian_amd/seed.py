"""GaussianModel.create_from_pcd on the GPU (csrc/seed.hip): the model seeded from the init stage in a fixed number of launches
around one host read.

The reference (scene/gaussian_model.py:362-468, train.py:102) loops over the ordered view pairs in Python: per pair a mask, six
boolean gathers that each read a count back, an index_put into the view's sparse depth image; then five concatenations, RGB2SH,
distCUDA2 and a handful of fills.  Its rule decides every match from that match alone and the arena of the init stage already lies
in the order the loop walks, so here it is classify / scan / scatter, the existing kNN, and a finishing pass:

    from scgaussian_amd import seed
    from scgaussian_amd.init_stage import InitStage
    stage = InitStage.from_view_gs(gaussians.view_gs)
    seed.install(gaussians, stage)                             # gaussians.create_from_pcd now runs here (train.py:102)
    stage.run_schedule(2000, halve_at=(500, 1000, 1500))
    stage.load_best(gaussians.view_gs)
    gaussians.create_from_pcd(stage.min_loss_state())

Where several kept matches of one view fall on one pixel of `sparse_depths`, the match latest in arena order wins: what the
reference gives wherever it is defined (a later pair overwrites an earlier one) and what its index_put gives on the CPU within a
pair, where a GPU's is not deterministic.  A match whose uv is not finite is seeded but writes no depth.

There is no CPU path: CPU tensors raise ScgError.
"""
from __future__ import annotations

import ctypes as C
import functools
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from . import _arena, _lib

THRESHOLD = 0.1                                 # create_from_pcd: min_loss_state[a][b] < 0.1
_BG_NAMES = ("bg_xyz", "bg_features_dc", "bg_features_rest", "bg_scaling", "bg_rotation", "bg_opacity")
_SEG_DTYPE = np.dtype(_lib.ScgSeedSegment)      # the table's record: the ctypes struct's fields, offsets and size
_WHAT = "seed: the seeding step"                # ... needs tensors on the GPU (_lib.stream_of)


def _err(msg: str):
    return _lib.ScgError("seed: " + msg)


def raw_opacity() -> float:
    """inverse_sigmoid(0.1) as the reference forms it on an fp32 tensor: log(x / (1 - x)) with x = float32(0.1)."""
    x = np.float32(0.1)
    return float(np.log(x / (np.float32(1.0) - x), dtype=np.float32))


def _flat(t: torch.Tensor, tail: Tuple[int, ...], dev) -> torch.Tensor:
    _lib.stream_of(t, _WHAT)
    return t.detach().to(device=dev, dtype=torch.float32).reshape((-1,) + tail)


def _table(segments, views, dev):
    """The segment table on the host (a numpy record array the C entry validates) and its copy in device memory."""
    rec = np.zeros(len(segments), dtype=_SEG_DTYPE)
    rec["offset"] = [s[2] for s in segments]
    rec["count"] = [s[3] for s in segments]
    rec["view"] = views
    return rec, _arena.upload_table(rec, dev)


class SeedInputs:
    """What create_from_pcd reads per match, flat in arena order, packed once: color (N,3), the match's own uv (N,2), the z
    component of its camera-space ray (N), rays_o / rays_d (N,3), z (N), min_loss (N) or None, and the segment table (host and
    device) with each segment's source view.  views: the per-view entries of view_gs in dictionary order."""

    def __init__(self, segments, table_host, table_dev, views, H, W, color, uv, cam_z, rays_o, rays_d, z, min_loss, stage):
        self.segments: List[Tuple[object, object, int, int]] = segments
        self.table_host, self.table_dev = table_host, table_dev
        self.views, self.H, self.W = views, H, W
        self.color, self.uv, self.cam_z = color, uv, cam_z
        self.rays_o, self.rays_d, self.z, self.min_loss = rays_o, rays_d, z, min_loss
        self.stage = stage

    @property
    def N(self) -> int:
        return self.z.numel()

    @property
    def V(self) -> int:
        return len(self.views)

    @classmethod
    def from_view_gs(cls, view_gs: Dict, stage=None) -> "SeedInputs":
        """Given `stage` (the InitStage of this view_gs), its rays_o, rays_d, z and min_loss are shared, not copied: the inputs can
        be packed before the stage runs and see its result.  Without it they are concatenated from view_gs as it is now."""
        keys, pairs = _arena.walk(view_gs)
        if not keys:
            raise _err("view_gs holds no view")
        sizes = {(int(view_gs[k]["height"]), int(view_gs[k]["width"])) for k in keys}
        if len(sizes) != 1:
            raise _err(f"the views have unequal sizes {sorted(sizes)}: sparse_depths and img_colors cannot be stacked")
        (H, W), = sizes
        if H <= 0 or W <= 0:
            raise _err(f"views of {W} x {H} pixels")
        if not pairs:
            raise _err("view_gs holds no match pair")
        segments, infos = [p[:4] for p in pairs], [p[4] for p in pairs]
        off = pairs[-1][2] + pairs[-1][3]
        if len(segments) > _lib.SEED_MAX_SEGMENTS:
            raise _err(f"{len(segments)} ordered view pairs are more than the kernels take ({_lib.SEED_MAX_SEGMENTS})")
        if off >= 2 ** 31:
            raise _err(f"{off} matches are more than the kernels take")
        if stage is not None and list(stage.segments) != segments:
            raise _err("the init stage was packed from another view_gs (its segments differ)")
        dev = stage.z.device if stage is not None else infos[0]["rays_o"].device
        _lib.stream_of(dev, _WHAT)
        cat = lambda key, tail: torch.cat([_flat(i[key], tail, dev) for i in infos]).contiguous()      # noqa: E731
        color, uv = cat("color", (3,)), cat("uv", (2,))
        cam_z = torch.cat([_flat(i["cam_rays_d"], (3,), dev)[:, 2] for i in infos]).contiguous()
        for name, t, rows in (("color", color, off), ("uv", uv, off), ("cam_rays_d", cam_z, off)):
            if t.shape[0] != rows:
                raise _err(f"{name} holds {t.shape[0]} rows, rays_o {rows}")
        if stage is not None:
            rays_o, rays_d, z, min_loss = stage.rays_o, stage.rays_d, stage.z, stage.min_loss
        else:
            rays_o, rays_d, min_loss = cat("rays_o", (3,)), cat("rays_d", (3,)), None
            z = cat("z_val", ())
            if z.shape[0] != off or rays_d.shape[0] != off:
                raise _err(f"z_val / rays_d hold {z.shape[0]} / {rays_d.shape[0]} rows, rays_o {off}")
        rec, table_dev = _table(segments, [keys.index(s[0]) for s in segments], dev)
        return cls(segments, rec, table_dev, [view_gs[k] for k in keys], H, W, color, uv, cam_z, rays_o, rays_d, z, min_loss, stage)

    @classmethod
    def from_mono(cls, setup, stage=None) -> "SeedInputs":
        """The inputs over the arena of a mono.MonoSetup, read in place: color, uv and cam_z are the setup's own tensors, rays_o,
        rays_d, z and min_loss the stage's (InitStage.from_mono(setup)) or, without one, the setup's.  No copy, no host read."""
        plan = setup.plan
        sizes = {(c["H"], c["W"]) for c in plan.consts}
        if len(sizes) != 1:
            raise _err(f"the views have unequal sizes {sorted(sizes)}: sparse_depths and img_colors cannot be stacked")
        (H, W), = sizes
        segments = list(setup.segments)
        if len(segments) > _lib.SEED_MAX_SEGMENTS:
            raise _err(f"{len(segments)} ordered view pairs are more than the kernels take ({_lib.SEED_MAX_SEGMENTS})")
        if stage is not None and (list(stage.segments) != segments or stage.z.data_ptr() != setup.z.data_ptr()):
            raise _err("the init stage was packed from another setup (its segments or its arena differ)")
        _lib.stream_of(setup.z, _WHAT)
        rays_o, rays_d, z = (stage.rays_o, stage.rays_d, stage.z) if stage is not None else (setup.rays_o, setup.rays_d, setup.z)
        return cls(segments, plan.seed_table_host, setup.seed_table, [setup.view_gs[k] for k in setup.keys], H, W, setup.color,
                   setup.uv, setup.cam_z, rays_o, rays_d, z, stage.min_loss if stage is not None else None, stage)

    @classmethod
    def from_flat(cls, rays_o, rays_d, z, color, uv, cam_z, counts, seg_view, V: int, H: int, W: int, views=None) -> "SeedInputs":
        """Inputs that already lie flat in arena order: counts[s] matches of source view seg_view[s] per segment.  The tensors
        are used as they are (seed_arrays validates them).  views: V per-view dicts for create_from_pcd's stacks."""
        if len(counts) != len(seg_view):
            raise _err(f"{len(counts)} segment sizes but {len(seg_view)} source views")
        if len(counts) > _lib.SEED_MAX_SEGMENTS:
            raise _err(f"{len(counts)} segments are more than the kernels take ({_lib.SEED_MAX_SEGMENTS})")
        segments, off = [], 0
        for s, (M, v) in enumerate(zip(counts, seg_view)):
            segments.append((int(v), s, off, int(M)))
            off += int(M)
        _lib.stream_of(z, _WHAT)
        rec, table_dev = _table(segments, [int(v) for v in seg_view], z.device)
        return cls(segments, rec, table_dev, list(views) if views is not None else [None] * V, H, W, color, uv, cam_z, rays_o,
                   rays_d, z, None, None)


def _min_loss_flat(inputs: SeedInputs, state: Optional[Dict], stage) -> Optional[torch.Tensor]:
    """The (N) tensor of the nested min_loss_state: the stage's own arena when the dict holds its views in arena order
    (_arena.is_arena), one concatenation otherwise."""
    if state is None:
        return None
    ts = []
    for a, b, _off, M in inputs.segments:
        try:
            t = state[a][b]
        except KeyError:
            raise _err(f"min_loss_state has no entry for pair ({a}, {b})") from None
        _lib.stream_of(t, "seed: min_loss_state")
        if t.numel() != M:
            raise _err(f"min_loss_state of pair ({a}, {b}) has {t.numel()} elements, the pair {M} matches")
        ts.append(t)
    for flat in ([stage.min_loss] if stage is not None else []) + ([inputs.min_loss] if inputs.min_loss is not None else []):
        if flat.numel() == inputs.N and _arena.is_arena(flat, ts, inputs.segments):
            return flat
    return torch.cat([_flat(t, (), inputs.z.device) for t in ts]).contiguous()


def check_rows(n_out: int, counted: int) -> None:
    """The host-side half of the C entries' validation: the rows the outputs were allocated for are the rows that were counted."""
    if n_out != counted:
        raise _err(f"n_out = {n_out} contradicts the counted total {counted}")


def seed_arrays(inputs: SeedInputs, min_loss: Optional[torch.Tensor], threshold: float = THRESHOLD, n_out: Optional[int] = None):
    """The launches of one call on packed inputs: a dict of plain tensors (zval (n,1), rayo, rayd, points (n,3), features_dc
    (n,1,3), features_rest (n,15,3), rotation (n,4), opacity (n,1), scaling (n,3), max_radii2D (n), dist2 (n), sparse_depths
    (V,H,W), masks (V,H,W) bool) and n.  n_out: the rows the caller expects; a contradiction with the counted total raises."""
    N, V, H, W = inputs.N, inputs.V, inputs.H, inputs.W
    stream = _lib.stream_of(inputs.z, _WHAT)
    dev = inputs.z.device
    for name, t, shape in (("rays_o", inputs.rays_o, (N, 3)), ("rays_d", inputs.rays_d, (N, 3)), ("z", inputs.z, (N,)),
                           ("color", inputs.color, (N, 3)), ("uv", inputs.uv, (N, 2)), ("cam_z", inputs.cam_z, (N,)),
                           ("min_loss", min_loss, (N,))):
        if t is None and name == "min_loss":
            continue
        if t.device != dev or t.dtype != torch.float32 or tuple(t.shape) != shape or not t.is_contiguous():
            raise _err(f"{name} must be a contiguous fp32 tensor of shape {shape} on {dev}")
    lib = _lib.load()
    pixels = V * H * W
    ws_bytes = lib.scg_seed_workspace_bytes(N, pixels)
    if ws_bytes == 0:
        raise _err(f"{N} matches / {pixels} pixels are more than the kernels take")
    with torch.cuda.device(dev):
        ws = torch.empty(ws_bytes // 4, dtype=torch.int32, device=dev)
        _lib.check(lib.scg_seed_classify(_lib.ptr(min_loss), N, float(threshold), pixels, ws.data_ptr(), ws_bytes, stream),
                   "scg_seed_classify")
        n = int(ws[0].item())                                                              # the one host read
        if n_out is not None:
            check_rows(int(n_out), n)
        f32 = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)           # noqa: E731
        out = {"zval": f32(n, 1), "rayo": f32(n, 3), "rayd": f32(n, 3), "points": f32(n, 3), "features_dc": f32(n, 1, 3),
               "features_rest": f32(n, 15, 3), "rotation": f32(n, 4), "opacity": f32(n, 1), "scaling": f32(n, 3),
               "max_radii2D": f32(n), "dist2": f32(n), "sparse_depths": f32(V, H, W),
               "masks": torch.empty((V, H, W), dtype=torch.bool, device=dev)}
        a = _lib.ScgSeedScatter()
        a.struct_bytes = C.sizeof(_lib.ScgSeedScatter)
        a.N, a.n_out, a.V, a.H, a.W, a.nseg = N, n, V, H, W, len(inputs.segments)
        a.segments, a.segments_dev = inputs.table_host.ctypes.data, inputs.table_dev.data_ptr()
        a.rays_o, a.rays_d, a.z, a.color, a.uv = (t.data_ptr() or None for t in (inputs.rays_o, inputs.rays_d, inputs.z,
                                                                                inputs.color, inputs.uv))
        a.opacity = raw_opacity()
        a.zval, a.rayo, a.rayd, a.points = (out[k].data_ptr() or None for k in ("zval", "rayo", "rayd", "points"))
        a.features_dc, a.features_rest, a.rotation = (out[k].data_ptr() or None for k in ("features_dc", "features_rest", "rotation"))
        a.opacity_out, a.max_radii2D = out["opacity"].data_ptr() or None, out["max_radii2D"].data_ptr() or None
        _lib.check(lib.scg_seed_scatter(C.byref(a), ws.data_ptr(), ws_bytes, stream), "scg_seed_scatter")
        if n > 0:
            knn_bytes = lib.scg_knn3_scratch_bytes(n)
            scratch = torch.empty((knn_bytes,), dtype=torch.uint8, device=dev)
            _lib.check(lib.scg_knn3_mean_dist2_ws(out["points"].data_ptr(), n, out["dist2"].data_ptr(), scratch.data_ptr(),
                                                  knn_bytes, stream), "scg_knn3_mean_dist2_ws")
        _lib.check(lib.scg_seed_finish(n, out["dist2"].data_ptr() or None, out["scaling"].data_ptr() or None, N,
                                       inputs.z.data_ptr() or None, inputs.cam_z.data_ptr() or None, V, H, W,
                                       out["sparse_depths"].data_ptr() or None, out["masks"].data_ptr() or None, ws.data_ptr(),
                                       ws_bytes, stream), "scg_seed_finish")
    out["n"] = n
    return out


@torch.no_grad()
def create_from_pcd(gaussians, min_loss_state: Optional[Dict] = None, *, stage=None, inputs: Optional[SeedInputs] = None,
                    threshold: float = THRESHOLD) -> None:
    """The reference's GaussianModel.create_from_pcd(min_loss_state) on `gaussians`, any object with the reference model's
    attribute names and a `view_gs`.  min_loss_state: the reference's nested {a: {b: (M)}} or None (every match is kept); when its
    tensors are the stage's own views in arena order they are used in place, otherwise concatenated once.  stage: the InitStage
    of this view_gs (its rays and depths are shared); inputs: a SeedInputs packed earlier.  One host read: the row count."""
    if inputs is None:
        if not hasattr(gaussians, "view_gs"):
            raise _err("the model has no view_gs")
        inputs = SeedInputs.from_view_gs(gaussians.view_gs, stage)
    if stage is None:
        stage = inputs.stage
    min_loss = _min_loss_flat(inputs, min_loss_state, stage)
    dev = inputs.z.device
    out = seed_arrays(inputs, min_loss, threshold)
    n = out["n"]

    views = inputs.views
    on = lambda t: t if t.device == dev else t.to(dev)                                     # noqa: E731
    gaussians.intrs = torch.stack([on(v["intr"]) for v in views])
    gaussians.w2cs = torch.stack([on(v["w2c"]) for v in views])
    gaussians.img_colors = torch.stack([on(v["image_color"]).reshape(inputs.H, inputs.W, 3).permute(2, 0, 1) for v in views])
    gaussians.near_fars = torch.stack([on(v["near_far"]) for v in views])
    gaussians.sparse_depths, gaussians.masks = out["sparse_depths"], out["masks"]
    gaussians.curr_scale, gaussians.curr_patch_size = 1, 5

    print("Number of points at initialisation : ", n)

    param = lambda t: torch.nn.Parameter(t.requires_grad_(True))                           # noqa: E731
    gaussians._zval = param(out["zval"])
    gaussians._rayo, gaussians._rayd = out["rayo"], out["rayd"]
    gaussians._features_dc = param(out["features_dc"])
    gaussians._features_rest = param(out["features_rest"])
    gaussians._scaling = param(out["scaling"])
    gaussians._rotation = param(out["rotation"])
    gaussians._opacity = param(out["opacity"])
    for name in _BG_NAMES:                                           # one-dimensional empties: "no background set yet"
        setattr(gaussians, name, torch.nn.Parameter(torch.empty(0, device=dev)))
    gaussians.max_radii2D = out["max_radii2D"]
    if hasattr(gaussians, "__dict__"):
        gaussians.__dict__.pop("_scg_model_args", None)              # the render path's cache holds the old tensors alive


def install(gaussians, stage=None) -> None:
    """Bind create_from_pcd as a method of this model instance under the reference's name, so that train.py:102 runs unchanged;
    `stage` (an InitStage) is kept and its arena tensors are used in place."""
    gaussians.create_from_pcd = functools.partial(create_from_pcd, gaussians, stage=stage)

"""ctypes binding of libscg_raster.so (the headers under include/).

The library is the product path: if it is missing or fails to load this module raises — there is no
CPU or PyTorch fallback (the oracle under oracle/ is test infrastructure and is never imported here).
"""
from __future__ import annotations

import ctypes as C
import os

import torch  # noqa: F401  (imported first so that torch's bundled libamdhip64.so.7 is the HIP runtime we bind to)

_HERE = os.path.dirname(os.path.abspath(__file__))
# SCG_LIB_PATH selects an experiment variant built with `python -m scgaussian_amd.build --tag=...` (profiling only)
LIB_PATH = os.environ.get("SCG_LIB_PATH") or os.path.join(_HERE, "libscg_raster.so")

# The headers' integer #defines under their own names minus "SCG_" (include/scg_raster.h, scg_matchloss.h, scg_mono.h).
# tests/test_abi_cpu.py holds every one of them, the enumerators below, the structs and SYMBOLS against the headers' text.
ABI_VERSION = 10
TILE, SPLAT_FLOATS, DSPLAT_FLOATS = 16, 12, 16   # pixels of a tile's edge; floats of a splat record and of a gradient record (64 bytes)
ADAM_MAX_SEGMENTS, ADAM_FORCE_FULL = 16, 1
INIT_STAGE_MAX_STEPS = 4096
SEED_MAX_SEGMENTS = 1024
MONO_MAX_VIEWS, MONO_MAX_SEGMENTS = 1024, 65536
# The option / flag enumerators, named the same way (include/scg_raster.h; DEBUG_*: csrc/scg_debug.h, the library's A/B bits of
# scg_forward's `options`).
FORWARD_NO_BACKWARD_STATE, FORWARD_SKIP_RARE_SORT, FORWARD_RARE_8WAVE, FORWARD_SPLIT_LONG_LISTS = 4, 8, 16, 32
FORWARD_ARM_PARTIAL_SUMS = 64
DEBUG_SEPARATE_SORT, DEBUG_SEPARATE_HIST = 1, 2
BACKWARD_ACCUMULATE, BACKWARD_SH_TAIL_ZERO = 1, 2
BINNING_AUTO, BINNING_GLOBAL_SORT = 0, 1


class ScgFrame(C.Structure):
    _fields_ = [
        ("P", C.c_int32), ("sh_degree", C.c_int32), ("sh_coeffs", C.c_int32),
        ("width", C.c_int32), ("height", C.c_int32),
        ("tanfovx", C.c_float), ("tanfovy", C.c_float), ("scale_modifier", C.c_float),
        ("prefiltered", C.c_int32), ("debug", C.c_int32),
        ("viewmatrix", C.c_void_p), ("projmatrix", C.c_void_p), ("campos", C.c_void_p), ("bg", C.c_void_p),
        ("tile_cost_in", C.c_void_p), ("tile_cost_out", C.c_void_p), ("long_lists_out", C.c_void_p),
        ("bwd_cost_in", C.c_void_p), ("bwd_cost_out", C.c_void_p), ("num_rendered_out", C.c_void_p),
    ]


class ScgWorkspaceLayout(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("splats", "rects", "depth_keys", "clamped", "point_list", "ranges", "final_T",
                                          "n_contrib", "bin_scratch", "total", "partial_words")]


class ScgStageEvents(C.Structure):
    _fields_ = [("begin", C.c_void_p * 3), ("end", C.c_void_p * 3)]


class ScgModelSet(C.Structure):
    """One set of Gaussians in the reference model's raw parameterisation (include/scg_raster.h ScgModelSet)."""
    _fields_ = [("count", C.c_int32)] + [(n, C.c_void_p) for n in ("zval", "rayo", "rayd", "xyz", "features_dc", "features_rest",
                                                                   "opacity", "scaling", "rotation")]


class ScgModel(C.Structure):
    _fields_ = [("ray", ScgModelSet), ("bg", ScgModelSet)]


class ScgModelGradSet(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("zval", "xyz", "features_dc", "features_rest", "opacity", "scaling", "rotation")]


class ScgModelGrads(C.Structure):
    _fields_ = [("ray", ScgModelGradSet), ("bg", ScgModelGradSet)]


class ScgAdamSegment(C.Structure):
    """One parameter tensor of an scg_adam_step launch (include/scg_raster.h ScgAdamSegment)."""
    _fields_ = [(n, C.c_void_p) for n in ("param", "grad", "exp_avg", "exp_avg_sq", "step")] + [
        ("numel", C.c_int64), ("row_len", C.c_int32), ("flags", C.c_int32),
        ("lr", C.c_double), ("beta1", C.c_double), ("beta2", C.c_double), ("eps", C.c_double)]


class ScgInitSegment(C.Structure):
    """One ordered view pair of the init stage's device table (include/scg_matchloss.h ScgInitSegment)."""
    _fields_ = [("offset", C.c_int32), ("count", C.c_int32), ("width", C.c_float), ("height", C.c_float),
                ("intr", C.c_float * 9), ("w2c", C.c_float * 12)]


class ScgDensifyTensors(C.Structure):
    """The six tensors of a background set, or one Adam moment of each (include/scg_raster.h ScgDensifyTensors)."""
    _fields_ = [(n, C.c_void_p) for n in ("xyz", "features_dc", "features_rest", "opacity", "scaling", "rotation")]


class ScgDensifyScatter(C.Structure):
    _fields_ = [("out_rows", C.c_int32)] + [(n, ScgDensifyTensors) for n in ("out", "out_exp_avg", "out_exp_avg_sq", "in_exp_avg",
                                                                             "in_exp_avg_sq")] + [
        (n, C.c_void_p) for n in ("ray_scaling", "ray_scaling_exp_avg", "ray_scaling_exp_avg_sq", "accum", "denom", "max_radii2D",
                                  "noise")]


class ScgSeedSegment(C.Structure):
    """One ordered view pair of the seeding step's table (include/scg_raster.h ScgSeedSegment)."""
    _fields_ = [("offset", C.c_int32), ("count", C.c_int32), ("view", C.c_int32)]


class ScgSeedScatter(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("struct_bytes", "N", "n_out", "V", "H", "W", "nseg")] + [
        (n, C.c_void_p) for n in ("segments", "segments_dev", "rays_o", "rays_d", "z", "color", "uv")] + [("opacity", C.c_float)] + [
        (n, C.c_void_p) for n in ("zval", "rayo", "rayd", "points", "features_dc", "features_rest", "rotation", "opacity_out",
                                  "max_radii2D")]


class ScgMonoView(C.Structure):
    """One view of the scene setup's device table (include/scg_mono.h ScgMonoView)."""
    _fields_ = [("image_off", C.c_int64), ("mask_off", C.c_int64), ("H", C.c_int32), ("W", C.c_int32), ("near_z", C.c_float),
                ("far_z", C.c_float), ("Kinv", C.c_double * 9), ("Rc2w", C.c_double * 9), ("Rw2c", C.c_double * 9),
                ("origin", C.c_double * 3)]


class ScgMonoSegment(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("offset", "count", "view", "partner")]


class ScgMonoGroup(C.Structure):
    _fields_ = [("segment", C.c_int32), ("first", C.c_int32)]


class ScgMono(C.Structure):
    """Everything the three scg_mono_* calls take (include/scg_mono.h ScgMono)."""
    _fields_ = [(n, C.c_int32) for n in ("struct_bytes", "V", "nseg", "ngroups", "N", "reserved")] + [
        (n, C.c_int64) for n in ("image_pixels", "mask_pixels", "max_view_pixels")] + [
        (n, C.c_void_p) for n in ("views", "segments", "groups", "image_bytes", "masks", "match_pixel", "u", "image_color", "uv",
                                  "color", "blender_mask", "rays_o", "rays_d", "cam_rays_d", "cam_z", "z", "uv_t", "valid", "wgt",
                                  "counts")]


# The structs whose size the library reports: query function -> the classes in the order of its `which` argument.  open_library
# compares every one; tests/test_abi_cpu.py walks the same table.
SIZE_CHECKED = {
    "scg_struct_bytes": (ScgFrame, ScgWorkspaceLayout, ScgStageEvents, ScgModel, ScgModelGrads, ScgAdamSegment, ScgInitSegment,
                         ScgDensifyScatter),
    "scg_mono_struct_bytes": (ScgMono, ScgMonoView, ScgMonoSegment, ScgMonoGroup),
}


# name -> (restype, argtypes): every entry point that a header under include/ declares, each declared in exactly one of them
_P = C.c_void_p
SYMBOLS = {
    "scg_last_error": (C.c_char_p, []),
    "scg_abi_version": (C.c_int32, []),
    "scg_struct_bytes": (C.c_size_t, [C.c_int32]),
    "scg_ranges_words": (C.c_size_t, [C.c_int32, C.c_int32]),
    "scg_geometry_scratch_bytes": (C.c_size_t, [C.c_int32]),
    "scg_geometry_forward": (C.c_int, [C.POINTER(ScgFrame)] + [_P] * 7 + [_P] * 6 + [_P, C.c_size_t, _P]),
    "scg_binning_scratch_bytes": (C.c_size_t, [C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_int32]),
    "scg_binning_accepts_bound": (C.c_int32, [C.c_int64, C.c_int32, C.c_int32, C.c_int32]),
    "scg_binning": (C.c_int, [C.POINTER(ScgFrame), C.c_int64] + [_P] * 2 + [_P] * 3 + [C.c_int32, _P, C.c_size_t, _P]),
    "scg_sort_scratch_bytes": (C.c_size_t, [C.c_int64]),
    "scg_sort_pairs": (C.c_int, [_P] * 4 + [C.c_int64, C.c_int32, _P, C.c_size_t, _P]),
    "scg_scan_scratch_bytes": (C.c_size_t, [C.c_int64]),
    "scg_inclusive_scan_u32": (C.c_int, [_P, _P, C.c_int64, _P, _P, C.c_size_t, _P]),
    "scg_blend_forward": (C.c_int, [C.POINTER(ScgFrame)] + [_P] * 3 + [_P] * 5 + [_P, _P]),
    "scg_blend_backward": (C.c_int, [C.POINTER(ScgFrame)] + [_P] * 5 + [_P] * 3 + [_P, C.c_int32, _P]),
    "scg_image_loss_dmaps_bytes": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32]),
    "scg_image_loss_scratch_bytes": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32]),
    "scg_image_loss_forward": (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P, C.c_size_t, _P]),
    "scg_image_loss_backward": (C.c_int, [_P, _P, _P, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P]),
    "scg_image_loss_forward_combined": (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_float, _P, _P, _P, C.c_size_t, _P]),
    "scg_image_loss_backward_combined": (C.c_int, [_P, _P, _P, C.c_int32, C.c_int32, C.c_int32, _P, C.c_float, _P, _P]),
    "scg_dtu_bg_mask": (C.c_int, [_P, C.c_int32, C.c_int32, C.c_float, C.c_int32, _P, _P, _P, _P]),
    "scg_dtu_bg_mask_segment_rows": (C.c_int32, []),
    "scg_masked_mean_scratch_bytes": (C.c_size_t, [C.c_int64]),
    "scg_masked_mean_forward": (C.c_int, [_P, _P, C.c_int64, _P, _P, _P, C.c_size_t, _P]),
    "scg_masked_mean_backward": (C.c_int, [_P, C.c_int64, _P, _P, _P, _P]),
    "scg_eval_metrics_scratch_bytes": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32]),
    "scg_eval_metrics": (C.c_int, [_P, _P, _P, C.c_int32, C.c_int32, C.c_int32, _P, _P, C.c_size_t, _P]),
    "scg_eval_depth_range_scratch_bytes": (C.c_size_t, [C.c_int64]),
    "scg_eval_depth_range": (C.c_int, [_P, C.c_int64, _P, _P, C.c_size_t, _P]),
    "scg_eval_view_tile": (C.c_int32, [C.c_int32]),
    "scg_eval_view": (C.c_int, [_P] * 5 + [C.c_int32, C.c_int32] + [_P] * 9 + [_P]),
    "scg_geocheck_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32]),
    "scg_geocheck_tile": (C.c_int32, [C.c_int32]),
    "scg_geocheck_setup": (C.c_int, [_P, _P, C.c_int32, C.c_int32, _P, C.c_size_t, _P]),
    "scg_geocheck": (C.c_int, [_P] + [C.c_int32] * 4 + [C.c_double, C.c_double, C.c_int32, _P, C.c_size_t, _P, _P, _P, _P]),
    "scg_viz_select_block": (C.c_int32, []),
    "scg_viz_select_scratch_bytes": (C.c_size_t, [C.c_int64]),
    "scg_viz_select": (C.c_int, [_P, _P, C.c_int64, C.c_double, _P, _P, _P, C.c_size_t, _P]),
    "scg_viz_frame": (C.c_int, [_P] * 6 + [C.c_int32, C.c_int32] + [_P] * 5 + [_P]),
    "scg_mono_struct_bytes": (C.c_size_t, [C.c_int32]),
    "scg_mono_block": (C.c_int32, []),
    "scg_mono_images": (C.c_int, [C.POINTER(ScgMono), _P]),
    "scg_mono_matches": (C.c_int, [C.POINTER(ScgMono), _P]),
    "scg_mono_pairs": (C.c_int, [C.POINTER(ScgMono), _P]),
    "scg_match_loss_pair": (C.c_int, [_P, C.c_int32, C.c_int32] + [_P] * 9 + [C.c_int32, C.c_float, C.c_float, _P, _P, _P]),
    "scg_init_stage_partials_bytes": (C.c_size_t, [C.c_int32, C.c_int32]),
    "scg_init_stage_run": (C.c_int, [_P, C.c_int32, C.c_int32] + [_P] * 4 + [_P] * 5 + [C.c_int32, C.c_int32] + [C.c_double] * 4
                           + [C.c_float, _P, _P, _P, C.c_size_t, _P]),
    "scg_knn3_scratch_bytes": (C.c_size_t, [C.c_int64]),
    "scg_knn3_mean_dist2_ws": (C.c_int, [_P, C.c_int64, _P, _P, C.c_size_t, _P]),
    "scg_geometry_backward": (C.c_int, [C.POINTER(ScgFrame)] + [_P] * 7 + [_P] * 3 + [_P] * 8 + [C.c_int32, _P]),
    "scg_workspace_layout": (C.c_int, [C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.POINTER(ScgWorkspaceLayout)]),
    "scg_forward": (C.c_int, [C.POINTER(ScgFrame)] + [_P] * 7 + [C.c_int64, _P, C.c_size_t] + [_P] * 4 + [_P, _P, _P, C.c_int32, _P, _P]),
    "scg_forward_sorts_in_blend": (C.c_int32, [C.c_int64, C.c_int32, C.c_int32, C.c_int32]),
    "scg_wait_num_rendered": (C.c_int64, [_P, _P, C.c_int32]),
    "scg_event_create": (C.c_int, [C.POINTER(C.c_void_p), C.c_int32]),
    "scg_event_destroy": (C.c_int, [_P]),
    "scg_event_elapsed_ms": (C.c_int, [_P, _P, C.POINTER(C.c_float)]),
    "scg_backward": (C.c_int, [C.POINTER(ScgFrame)] + [_P] * 7 + [_P, C.c_int64, _P] + [_P] * 3 + [_P, C.c_int32] + [_P] * 8 + [C.c_int32, _P, _P]),
    "scg_model_activate": (C.c_int, [C.POINTER(ScgModel)] + [_P] * 4 + [_P]),
    "scg_forward_model": (C.c_int, [C.POINTER(ScgFrame), C.POINTER(ScgModel), C.c_int64, _P, C.c_size_t] + [_P] * 4 + [_P, _P, _P, C.c_int32, _P, _P]),
    "scg_backward_model": (C.c_int, [C.POINTER(ScgFrame), C.POINTER(ScgModel), _P, C.c_int64, _P] + [_P] * 3 + [_P, C.c_int32]
                           + [C.POINTER(ScgModelGrads), _P, C.c_int32, _P, _P]),
    "scg_adam_workspace_bytes": (C.c_size_t, [C.c_int32]),
    "scg_adam_step": (C.c_int, [C.POINTER(ScgAdamSegment), C.c_int32, _P, _P, C.c_size_t, _P]),
    "scg_densify_stats": (C.c_int, [C.c_int32, _P, _P, C.c_int64, _P, _P, _P, _P]),
    "scg_densify_workspace_bytes": (C.c_size_t, [C.c_int32]),
    "scg_densify_classify": (C.c_int, [C.POINTER(ScgModel), _P, _P] + [C.c_float] * 4 + [_P, C.c_size_t, _P]),
    "scg_densify_scatter": (C.c_int, [C.POINTER(ScgModel), C.POINTER(ScgDensifyScatter), _P, C.c_size_t, _P]),
    "scg_reset_opacity": (C.c_int, [C.c_int32, _P, _P, _P, C.c_int32, _P, _P, _P, _P]),
    "scg_seed_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int64]),
    "scg_seed_classify": (C.c_int, [_P, C.c_int32, C.c_float, C.c_int64, _P, C.c_size_t, _P]),
    "scg_seed_scatter": (C.c_int, [C.POINTER(ScgSeedScatter), _P, C.c_size_t, _P]),
    "scg_seed_finish": (C.c_int, [C.c_int32, _P, _P, C.c_int32, _P, _P, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P, C.c_size_t, _P]),
}

_lib = None


class ScgError(RuntimeError):
    pass


def open_library(path: str, symbols=None, version=("scg_abi_version", ABI_VERSION), size_checked=None, name="library") -> C.CDLL:
    """dlopen + type + version-check one library.  The defaults are the main library's (the product loads exactly one build of
    it: load(); tools/ab_inproc.py opens several variants side by side for same-process A/B runs).  A side binding passes its own
    SYMBOLS, (version query, value), {size query: structs} and the file name its messages use.  A size query that takes no
    argument reports its one struct."""
    symbols = SYMBOLS if symbols is None else symbols
    size_checked = SIZE_CHECKED if size_checked is None else size_checked
    if not os.path.exists(path):
        raise ScgError(f"{path} not found: the HIP extension is required (python -m scgaussian_amd.build); "
                       "there is no CPU fallback")
    try:
        lib = C.CDLL(path)
    except OSError as e:  # pragma: no cover
        raise ScgError(f"cannot load {path}: {e}") from e
    for sym, (res, args) in symbols.items():
        try:
            fn = getattr(lib, sym)
        except AttributeError as e:
            raise ScgError(f"{path} does not export {sym}") from e
        fn.restype = res
        fn.argtypes = args
    query, want = version
    if getattr(lib, query)() != want:
        raise ScgError(f"ABI version mismatch: {name} {getattr(lib, query)()} != binding {want}")
    for query, structs in size_checked.items():
        fn = getattr(lib, query)
        for which, struct in enumerate(structs):
            got = fn(which) if fn.argtypes else fn()
            if got != C.sizeof(struct):
                raise ScgError(f"struct layout mismatch: {struct.__name__} is {got} bytes in the library, "
                               f"{C.sizeof(struct)} in the binding")
    return lib


def raise_last_error(rc: int, what: str, last_error) -> None:
    """The ScgError of a non-zero return code of `what`, with the text of the library's own *_last_error function."""
    msg = last_error()
    raise ScgError(f"{what} failed (code {rc}): {msg.decode() if msg else ''}")


def load() -> C.CDLL:
    """Load (once) and type the library.  Raises ScgError when it is absent: build it with
    ``python -m scgaussian_amd.build`` (or ``__graft_entry__.build()``)."""
    global _lib
    if _lib is None:
        _lib = open_library(LIB_PATH)
    return _lib


def check(rc: int, what: str) -> None:
    if rc != 0:
        raise_last_error(rc, what, load().scg_last_error)


def ptr(t) -> int:
    """Device pointer of a tensor (None -> NULL)."""
    return None if t is None else t.data_ptr()


def stream_of(t, what: str) -> int:
    """The current stream of the device of `t` (a tensor or a torch.device), as the handle the C entries take.  The one place that
    knows that the kernels need a GPU: anything that is not on one raises, `what` naming the step."""
    dev = getattr(t, "device", t)
    if not isinstance(dev, torch.device) or dev.type != "cuda":
        raise ScgError(f"{what} needs tensors on the ROCm GPU ('cuda'); there is no CPU path")
    return torch.cuda.current_stream(dev).cuda_stream

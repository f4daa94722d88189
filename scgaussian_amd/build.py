"""Build the HIP libraries in-tree with hipcc for gfx950: libscg_raster.so (SOURCES) and, behind it, one side library per entry
of SIDE_LIBRARIES, each with a header directory, an ABI version and an error string of its own.

    python -m scgaussian_amd.build [--force] [--verbose]

    libscg_io.so    include/io    scene files (save_ply / load_ply)
    libscg_img.so   include/img   camera images (Pillow's bicubic resize)
    libscg_mp.so    include/mp    the init stage's snapshot (save_ply_at_matchpoint)
    libscg_vw.so    include/vw    the virtual-view warp loss and the depth smoothness, forward and backward
    libscg_lp.so    include/lp    the LPIPS metric (VGG16 on the fp32 matrix pipe)
    libscg_png.so   include/png   PNG files' zlib streams
    libscg_jpg.so   include/jpg   JPEG files, the frames of a Motion-JPEG video
    libscg_jpegdec.so  include/jpegdec  baseline JPEG files decoded (Pillow's pixels)
    libscg_camgrad.so  include/camgrad  the rasterizer's camera gradients (view, projection, centre)

hipcc cross-compiles without a GPU; the libraries are git-ignored.  A source whose results are held to another
implementation's bits is compiled with -ffp-contract=off, one rounding per operation: the comment next to each such source in the
tables says what is held to what.  The 8-bit quantiser the image kernels share (csrc/pixel_rules.h) turns contraction off in its
own body and does not depend on the flag.
"""
from __future__ import annotations

import glob
import hashlib
import os
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
INCLUDE = os.path.join(os.path.dirname(HERE), "include")
OBJ_DIR = os.path.join(CSRC, "build")
LIB_PATH = os.path.join(HERE, "libscg_raster.so")
EXPORTS_MAP = os.path.join(CSRC, "exports.map")           # global: scg_*; local: everything else

ARCH = "gfx950"
COMMON = ["--offload-arch=" + ARCH, "-O3", "-std=c++17", "-fPIC", "-fvisibility=hidden", "-munsafe-fp-atomics", "-Wall",
          "-Wno-unused-function", "-I", INCLUDE]
SOURCES = {
    "api.hip": [],
    "geometry.hip": ["-ffp-contract=off"],        # bit-exact tile assignment
    "binning.hip": [],
    "binning_tiles.hip": [],
    # measured (tools/probes/valu_rate.hip): v_pk_*_f32 costs 1.67 issue slots, so the SLP vectoriser's packing of the
    # per-pixel scalar math (plus the v_mov shuffles it needs) loses; the explicit f32x2 accumulators still pack
    "blend.hip": ["-fno-slp-vectorize"],
    "knn.hip": [],
    "loss.hip": [],
    "dtumask.hip": [],                            # DTU scenes: background mask, alpha term, masked metrics (scg_loss.h)
    # (the 8-bit quantiser pins its own contraction, csrc/pixel_rules.h: in the next two files the flag is there for the rest)
    "evalview.hip": ["-ffp-contract=off"],        # test-set evaluation (scg_eval.h): the masked images and the error map's products as torch rounds them
    "matchloss.hip": [],
    "optim.hip": ["-ffp-contract=off"],           # Adam in torch's order, one rounding per operation (no fused multiply-adds; torch itself fuses its lerp)
    "initstage.hip": ["-ffp-contract=off"],       # the init stage's Adam: the same arithmetic (csrc/adam_math.h)
    "densify.hip": ["-ffp-contract=off"],         # clone xyz = rayo + rayd * zval and the / 1.6 rounded as torch rounds them
    "seed.hip": ["-ffp-contract=off"],            # create_from_pcd: points = rays_o + rays_d * z as torch's two operators round it
    "geocheck.hip": ["-ffp-contract=off"],        # cross-view depth check (scg_geocheck.h): numpy's float64 products and sums, none fused
    "mono.hip": ["-ffp-contract=off"],            # create_from_mono (scg_mono.h): torch's grid_sample in fp32 and the ray chain in fp64, none fused
    "depthviz.hip": ["-ffp-contract=off"],        # depth colour maps and video frames (scg_viz.h): numpy's percentile, matplotlib's Normalize
}
# The side libraries: short name -> (header directory under include/, {source: extra flags}).  The library is libscg_<name>.so;
# its entry points are not part of libscg_raster.so's ABI.  The same COMMON flags, the same export map, no variants.
SIDE_LIBRARIES = {
    "io": ("io", {      # include/io/scg_ply.h
        "plypack.hip": ["-ffp-contract=off"],     # save_ply / load_ply: x = rayo + rayd * zval and the colour bytes, one rounding per operation
    }),
    "img": ("img", {    # include/img/scg_resample.h
        "resample.hip": [],                       # integer arithmetic; its one float operation (byte / 255) is an explicitly rounded division
    }),
    "mp": ("mp", {      # include/mp/scg_matchpoint.h
        "matchpoint.hip": ["-ffp-contract=off"],  # xyz = rays_o + rays_d * z, depth = z * cam_z, (d - min) / (max - min): one rounding per operation
    }),
    "vw": ("vw", {      # include/vw/scg_virtualwarp.h
        "virtualwarp.hip": ["-ffp-contract=off"],  # the warp, torch's bilinear sampler and the 5x5 statistics: every product and sum rounded on its own
    }),
    "lp": ("lp", {      # include/lp/scg_lpips.h
        "lpips.hip": [],                          # its convolution sums are explicit fma chains (the fp32 MFMA, fmaf); the file turns contraction off for the rest
    }),
    "png": ("png", {    # include/png/scg_png.h
        "pngpack.hip": [],                        # integer arithmetic only
    }),
    "jpg": ("jpg", {    # include/jpg/scg_jpeg.h
        "jpegpack.hip": ["-ffp-contract=off"],    # integer arithmetic only; the flag says that the bytes are held to libjpeg's
    }),
    "jpegdec": ("jpegdec", {    # include/jpegdec/scg_jpegdec.h
        "jpegunpack.hip": ["-ffp-contract=off"],  # integer arithmetic only; the flag says, as for the packer, that the bytes are held to another implementation's (Pillow's pixels)
    }),
    "camgrad": ("camgrad", {    # include/camgrad/scg_camgrad.h
        # it recomputes the forward's colour clamp and must take the forward's decision, i.e. evaluate geometry.hip's chain of
        # single fp32 operations (csrc/geometry_math.h, csrc/sh_eval.h)
        "camgrad.hip": ["-ffp-contract=off"],
    }),
}


def side_library(key: str):
    """(path of libscg_<key>.so, its {source: extra flags}) of one entry of SIDE_LIBRARIES.  An unknown key raises KeyError."""
    return os.path.join(HERE, f"libscg_{key}.so"), SIDE_LIBRARIES[key][1]


def _h(*parts):
    return sorted(glob.glob(os.path.join(*parts, "*.h")))


HEADERS = _h(CSRC) + _h(INCLUDE) + [h for d, _ in SIDE_LIBRARIES.values() for h in _h(INCLUDE, d)]    # every object depends on all


def _hipcc() -> str:
    for cand in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError("hipcc not found (set HIPCC or install ROCm)")


def _digest(paths, extra: str) -> str:
    h = hashlib.sha256(extra.encode())
    for p in paths:
        with open(p, "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()


# The one variant that ships next to the product: the blend kernels with the COMPILER-written forward trip and backward walk
# instead of the hand-written ISA (csrc/blend.hip SCG_FWD_TRIP_CXX).  tests/test_gpu_parity.py renders with both and demands
# bit-identical outputs, and differentiates through both (gradients equal up to the order of the float atomics) — the guard of
# the hand-written code's hard-coded registers against a toolchain change.
CXX_TRIP_TAG = "cxx"


def build_cxx_trip_variant(verbose: bool = False) -> str:
    build(verbose=verbose)
    return build(verbose=verbose, tag=CXX_TRIP_TAG, defines=("SCG_FWD_TRIP_CXX",), only=("blend.hip",))


# The probe build: every wave of the geometry, scatter, forward-blend and blend-backward kernels logs the wall clock at the
# boundaries of its phases (csrc/probe_timeline.h; tools/probes/*_timeline.py read the log).  Not part of the default build;
# tests/test_probe_timeline_cpu.py compiles it, so that a kernel change that breaks it is noticed.
PROBE_TIMELINE_TAG = "tl"
PROBE_TIMELINE_SOURCES = ("geometry.hip", "binning_tiles.hip", "blend.hip")       # the sources that include the header


def build_probe_timeline_variant(verbose: bool = False) -> str:
    build(verbose=verbose)
    return build(verbose=verbose, tag=PROBE_TIMELINE_TAG, defines=("SCG_PROBE_TIMELINE",), only=PROBE_TIMELINE_SOURCES)


def _compile(hipcc: str, src: str, extra, obj: str, force: bool, verbose: bool) -> bool:
    """Compile csrc/<src> to `obj` unless its stamp says that source, headers and flags are the ones it was built from."""
    src_path = os.path.join(CSRC, src)
    stamp = obj + ".sha"
    dig = _digest([src_path] + HEADERS, " ".join(COMMON + extra))
    if not force and os.path.exists(obj) and os.path.exists(stamp) and open(stamp).read() == dig:
        return False
    cmd = [hipcc] + COMMON + extra + ["-c", src_path, "-o", obj]
    if verbose:
        print(" ".join(cmd), flush=True)
    subprocess.run(cmd, check=True)
    with open(stamp, "w") as fh:
        fh.write(dig)
    return True


def _link(hipcc: str, lib_path: str, objs, verbose: bool) -> None:
    cmd = [hipcc, "--offload-arch=" + ARCH, "-shared", "-fPIC", "-Wl,--version-script=" + EXPORTS_MAP, "-o", lib_path] + objs
    if verbose:
        print(" ".join(cmd), flush=True)
    subprocess.run(cmd, check=True)


def build_side(key: str, force: bool = False, verbose: bool = False) -> str:
    """libscg_<key>.so from its entry of SIDE_LIBRARIES."""
    lib_path, sources = side_library(key)
    os.makedirs(OBJ_DIR, exist_ok=True)
    hipcc = _hipcc()
    objs, rebuilt = [], False
    for src, extra in sources.items():
        obj = os.path.join(OBJ_DIR, os.path.basename(src).replace(".hip", ".o"))
        objs.append(obj)
        rebuilt |= _compile(hipcc, src, list(extra), obj, force, verbose)
    if rebuilt or force or not os.path.exists(lib_path):
        _link(hipcc, lib_path, objs, verbose)
    return lib_path


def build(force: bool = False, verbose: bool = False, tag: str = "", defines=(), flags=(), only=None) -> str:
    """tag/defines build a VARIANT libscg_raster_<tag>.so (selected at run time with SCG_LIB_PATH); the default build has
    neither and builds every side library behind the main one.  `only`: the sources the defines / flags apply to — the others
    are linked from the default build's objects."""
    os.makedirs(OBJ_DIR, exist_ok=True)
    hipcc = _hipcc()
    objs = []
    rebuilt = False
    lib_path = LIB_PATH if not tag else LIB_PATH.replace(".so", f"_{tag}.so")
    for src, extra in SOURCES.items():
        variant = bool(tag) and (only is None or src in only)
        if variant:
            extra = list(extra) + ["-D" + d for d in defines] + list(flags)
        obj = os.path.join(OBJ_DIR, src.replace(".hip", (f"_{tag}" if variant else "") + ".o"))
        objs.append(obj)
        rebuilt |= _compile(hipcc, src, list(extra), obj, force, verbose)
    if rebuilt or force or not os.path.exists(lib_path):
        _link(hipcc, lib_path, objs, verbose)
    if not tag:
        for key in SIDE_LIBRARIES:
            build_side(key, force=force, verbose=verbose)
    return lib_path


if __name__ == "__main__":
    tag, defines, flags = "", [], []
    for a in sys.argv[1:]:
        if a.startswith("--tag="):
            tag = a.split("=", 1)[1]
        elif a.startswith("-D"):
            defines.append(a[2:])
        elif a.startswith(("-f", "-m")):          # experiment variants: extra compiler flags for every source
            flags.append(a)
    path = build(force="--force" in sys.argv, verbose="--verbose" in sys.argv or "-v" in sys.argv, tag=tag,
                 defines=defines, flags=flags)
    print(path)

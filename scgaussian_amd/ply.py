"""GaussianModel.save_ply / load_ply on the GPU (csrc/plypack.hip, libscg_io.so): one launch and one copy each way.

The reference stores a scene with `plyfile`, one Python tuple per Gaussian (scene/gaussian_model.py:565-609), and loads it
property by property (:653-756); ply_io.py does the same with numpy on the host, about fifteen device-to-host copies for a model
that lives on the GPU.  The work is a re-layout, so here the three file bodies are built where the model lies:

    from scgaussian_amd import ply
    ply.install(gaussians)                 # gaussians.save_ply / .load_ply now run here: scene.save(iteration) (train.py:187) and
                                           # Scene(..., load_iteration=...) (scene/__init__.py:91-95) run unchanged, without plyfile

    packed = ply.pack(gaussians)           # one launch: the bodies of point_cloud.ply, point_cloud_bg.ply, point_cloud_color.ply
    packed.to_host()                       # the ONE device-to-host copy, into pinned memory
    packed.write(path)                     # headers + bodies; the bg file only when there are background Gaussians

The files are those of ply_io.save_ply byte for byte (tests/test_gpu_ply.py), quirks included: the colour file's bytes are numpy's
array cast of f_dc * 255 on x86-64 — the low 8 bits of the truncated value, 0 beyond int32 and for NaN.  The reference's own
storePly gives the same bytes under the numpy 1.x of its environment.yml; under numpy >= 2 its tuple assignment raises
OverflowError for a value outside 0..255 and ValueError for NaN.  Parity with bytes written by `plyfile` itself is not pinned
(the package is not available; ply_io.py says the same).

load_ply's device path takes what this project and the reference write: binary_little_endian, first element `vertex`, every
property 4 bytes wide, the needed ones `float`, any order, extra properties allowed (a column table built from the header
tells the kernel where each value lies).  Any other PLY file (ascii, big-endian, narrower or wider properties) goes through
ply_io.read_vertex_ply and one upload per tensor and gives the same tensors.  What the kernels do not take raises ScgError.
"""
from __future__ import annotations

import ctypes as C
import functools
import os
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from . import _lib, _lib_io, model_path, ply_io

TILE_ROWS = _lib_io.PLY_TILE_ROWS
RAY_FLOATS, BG_FLOATS, COLOR_BYTES = _lib_io.PLY_RAY_FLOATS, _lib_io.PLY_BG_FLOATS, _lib_io.PLY_COLOR_BYTES
RAY_NAMES = ply_io._attribute_names(3, 45)
BG_NAMES = ply_io._attribute_names(3, 45, prefix="b", ray_bound=False)
COLOR_NAMES = ["x", "y", "z", "nx", "ny", "nz", "red", "green", "blue"]
COLOR_TYPES = ["float"] * 6 + ["uchar"] * 3

_RAY_SHAPES = (("zval", (1,)), ("rayo", (3,)), ("rayd", (3,)), ("features_dc", (1, 3)), ("features_rest", (15, 3)),
               ("opacity", (1,)), ("scaling", (3,)), ("rotation", (4,)))
_BG_SHAPES = (("bg_xyz", (3,)), ("bg_features_dc", (1, 3)), ("bg_features_rest", (15, 3)), ("bg_opacity", (1,)),
              ("bg_scaling", (3,)), ("bg_rotation", (4,)))


def _err(msg: str):
    return _lib.ScgError("ply: " + msg)


def header(names: List[str], n: int, types: Optional[List[str]] = None) -> bytes:
    """The header ply_io.write_vertex_ply writes for `n` vertices with these properties."""
    types = types or ["float"] * len(names)
    lines = ["ply", "format binary_little_endian 1.0", f"element vertex {n}"]
    lines += [f"property {t} {nm}" for nm, t in zip(names, types)]
    lines.append("end_header")
    return ("\n".join(lines) + "\n").encode("ascii")


# --------------------------------------------------------------------------------------------------------------------------------
# the model's raw tensors as the library takes them
# --------------------------------------------------------------------------------------------------------------------------------
def _model_of(gaussians) -> Tuple[_lib.ScgModel, int, int, torch.device, tuple]:
    """(ScgModel, nr, nb, device, the tensors it points at) of a reference GaussianModel, a stand-in with its attribute names or a
    ply_io.RayBoundModel (model_path.tensors_of)."""
    t = model_path.tensors_of(gaussians)
    if t is None:
        raise _err("the model does not carry the reference's raw tensors (_zval, _rayo, _rayd, _features_dc, ...)")
    dev = t["zval"].device
    if dev.type != "cuda":
        raise _err("the model must be on the ROCm GPU ('cuda'); there is no CPU path (ply_io handles host models)")
    nr, nb = int(t["zval"].shape[0]), int(t["bg_xyz"].shape[0])
    m = _lib.ScgModel()
    m.ray.count, m.bg.count = nr, nb
    keep = []
    for shapes, rows, dst in ((_RAY_SHAPES, nr, m.ray), (_BG_SHAPES, nb, m.bg)):
        for name, tail in shapes:
            x = t[name].detach()
            if rows == 0:
                if x.shape[0] != 0:
                    raise _err(f"{name} has {x.shape[0]} rows in an empty set")
                continue
            if x.device != dev or x.dtype != torch.float32 or tuple(x.shape) != (rows,) + tail or not x.is_contiguous():
                raise _err(f"{name} must be a contiguous fp32 tensor of shape {(rows,) + tail} on {dev}, not {x.dtype} "
                           f"{tuple(x.shape)} on {x.device}")
            setattr(dst, name[3:] if name.startswith("bg_") else name, x.data_ptr())
            keep.append(x)
    return m, nr, nb, dev, tuple(keep)


class PackedScene:
    """The three file bodies of a scene in ONE device buffer (include/io/scg_ply.h ScgPlyLayout)."""

    def __init__(self, nr: int, nb: int, layout: _lib_io.ScgPlyLayout, buffer: torch.Tensor):
        self.nr, self.nb, self.layout, self.buffer = nr, nb, layout, buffer
        self.host: Optional[torch.Tensor] = None

    def to_host(self) -> torch.Tensor:
        """The step's one device-to-host copy: the whole buffer in one transfer into pinned memory."""
        if self.host is None:
            if self.buffer.numel():
                self.host = self.buffer.to("cpu", non_blocking=True)             # (a non-blocking copy to the host lands in pinned memory)
                torch.cuda.current_stream(self.buffer.device).synchronize()
            else:
                self.host = torch.empty(0, dtype=torch.uint8)
        return self.host

    def bodies(self) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """(ray-bound, background, colour) bodies as uint8 arrays, the colour body without its padding."""
        h, l = self.to_host().numpy(), self.layout
        return (h[l.ray_offset:l.ray_offset + l.ray_bytes], h[l.bg_offset:l.bg_offset + l.bg_bytes],
                h[l.color_offset:l.color_offset + (self.nr + self.nb) * COLOR_BYTES])

    def write(self, path: str) -> None:
        """`path` is .../point_cloud.ply; point_cloud_bg.ply (only with background Gaussians) and point_cloud_color.ply go next to
        it, as GaussianModel.save_ply places them.  The directory is created if missing."""
        ray, bg, color = self.bodies()
        folder = os.path.dirname(os.path.abspath(path))
        os.makedirs(folder, exist_ok=True)
        files = [(path, header(RAY_NAMES, self.nr), ray)]
        if self.nb > 0:
            files.append((os.path.join(folder, "point_cloud_bg.ply"), header(BG_NAMES, self.nb), bg))
        files.append((os.path.join(folder, "point_cloud_color.ply"), header(COLOR_NAMES, self.nr + self.nb, COLOR_TYPES), color))
        for p, head, body in files:
            with open(p, "wb") as fh:
                fh.write(head)
                fh.write(memoryview(body))


@torch.no_grad()
def pack(gaussians) -> PackedScene:
    """One launch, no host read: capturable in a graph at fixed counts (the buffer comes from the graph's pool)."""
    m, nr, nb, dev, _keep = _model_of(gaussians)
    lib = _lib_io.load()
    lay = _lib_io.ScgPlyLayout()
    _lib_io.check(lib.scg_ply_layout(nr, nb, C.byref(lay)), "scg_ply_layout")
    buf = torch.empty(int(lay.total), dtype=torch.uint8, device=dev)
    if nr + nb:
        with torch.cuda.device(dev):
            _lib_io.check(lib.scg_ply_pack(C.byref(m), buf.data_ptr(), buf.numel(), _lib.stream_of(dev, "ply.pack")), "scg_ply_pack")
    return PackedScene(nr, nb, lay, buf)


def save_ply(gaussians, path: str) -> None:
    """GaussianModel.save_ply(path): pack + one copy + the three writes."""
    packed = pack(gaussians)
    packed.to_host()
    packed.write(path)


@torch.no_grad()
def save_color_pcd(gaussians, camera_center, folder: str, sh_degree: Optional[int] = None) -> None:
    """`<folder>/point_cloud_color.ply` with the view-dependent colour of render(..., save_color_pcd=True)
    (gaussian_renderer/__init__.py:89-96) as seen from `camera_center`: one launch, one copy."""
    m, nr, nb, dev, _keep = _model_of(gaussians)
    deg = int(gaussians.active_sh_degree if sh_degree is None else sh_degree)
    cam = torch.as_tensor(camera_center, dtype=torch.float32).reshape(3).to(dev).contiguous()
    P = nr + nb
    buf = torch.empty((P * COLOR_BYTES + 3) // 4 * 4, dtype=torch.uint8, device=dev)
    if P:
        with torch.cuda.device(dev):
            _lib_io.check(_lib_io.load().scg_ply_pack_color_view(C.byref(m), deg, cam.data_ptr(), buf.data_ptr(), buf.numel(),
                                                                 _lib.stream_of(dev, "ply.save_color_pcd")),
                          "scg_ply_pack_color_view")
        host = buf.to("cpu", non_blocking=True)
        torch.cuda.current_stream(dev).synchronize()
    else:
        if not 0 <= deg <= 3:
            raise _err(f"SH degree {deg} is not 0..3")
        host = torch.empty(0, dtype=torch.uint8)
    os.makedirs(folder, exist_ok=True)
    with open(os.path.join(folder, "point_cloud_color.ply"), "wb") as fh:
        fh.write(header(COLOR_NAMES, P, COLOR_TYPES))
        fh.write(memoryview(host.numpy()[:P * COLOR_BYTES]))


# --------------------------------------------------------------------------------------------------------------------------------
# loading
# --------------------------------------------------------------------------------------------------------------------------------
def read_header(fh, path: str) -> dict:
    """The header of a PLY file: {format, element (name of the first), count, props [(name, numpy code)]}; fh is left at the first
    byte of the body.  Raises ValueError like ply_io.read_vertex_ply."""
    if fh.readline().strip() != b"ply":
        raise ValueError(f"{path}: not a PLY file")
    fmt, element, count, props, seen = None, None, None, [], 0
    while True:
        line = fh.readline()
        if not line:
            raise ValueError(f"{path}: header without end_header")
        tok = line.decode("ascii", "replace").split()
        if not tok or tok[0] in ("comment", "obj_info"):
            continue
        if tok[0] == "format":
            fmt = tok[1]
        elif tok[0] == "element":
            seen += 1
            if seen == 1:
                element, count = tok[1], int(tok[2])
        elif tok[0] == "property" and seen == 1:
            if tok[1] == "list":
                raise ValueError(f"{path}: list properties are not part of the SCGaussian format")
            props.append((tok[2], ply_io._PLY_TYPES[tok[1]]))
        elif tok[0] == "end_header":
            break
    if fmt is None or count is None:
        raise ValueError(f"{path}: incomplete PLY header")
    return {"format": fmt, "element": element, "count": count, "props": props}


def _suffixed(names: List[str], prefix: str, want: int, what: str) -> List[str]:
    """The properties `<prefix><int>` ordered by their integer suffix (scene/gaussian_model.py:666-703, ply_io._columns)."""
    got = [n for n in names if n.startswith(prefix) and n[len(prefix):].lstrip("_").isdigit()]
    got.sort(key=lambda n: int(n.split("_")[-1]))
    if not got:
        raise ValueError(f"PLY file has no '{prefix}*' properties")
    if len(got) != want:
        raise ValueError(f"expected {want} {prefix}* properties{what}, found {len(got)}")
    return got


def column_table(names: List[str], bg: bool = False, max_sh_degree: int = 3) -> np.ndarray:
    """int32 (69,) or (62,): for every column of this project's own record the index of the file's property it is loaded from.
    The columns nothing is loaded from (positions and normals of a ray-bound file, the normals of a background file) get 0."""
    b = "b" if bg else ""
    want = 3 * (max_sh_degree + 1) ** 2 - 3
    if want != 45:
        raise ValueError(f"the kernels hold SH degree 3 (45 f_rest properties), not degree {max_sh_degree}")
    src: List[Optional[str]] = ([b + "x", b + "y", b + "z"] if bg else [None] * 3) + [None] * 3
    src += _suffixed(names, b + "f_dc_", 3, "")
    src += _suffixed(names, b + "f_rest_", want, f" for SH degree {max_sh_degree}")
    src += [b + "opacity"] + _suffixed(names, b + "scale_", 3, "") + _suffixed(names, b + "rot", 4, "")
    if not bg:
        src += _suffixed(names, "zval", 1, "") + _suffixed(names, "rayo", 3, "") + _suffixed(names, "rayd", 3, "")
    index = {n: i for i, n in enumerate(names)}
    for s in src:
        if s is not None and s not in index:
            raise ValueError(f"PLY file has no '{s}' property")
    return np.array([0 if s is None else index[s] for s in src], dtype=np.int32)


def _empty_set(rows: int, bg: bool, dev) -> Dict[str, torch.Tensor]:
    shapes = _BG_SHAPES if bg else _RAY_SHAPES
    return {n: torch.empty((rows,) + tail, dtype=torch.float32, device=dev) for n, tail in shapes}


def _device_path(head: dict, max_sh_degree: int) -> bool:
    return (head["format"] == "binary_little_endian" and head["element"] == "vertex" and max_sh_degree == 3
            and 0 < len(head["props"]) <= _lib_io.PLY_MAX_STRIDE and head["count"] < 2 ** 31
            and all(np.dtype(t).itemsize == 4 for _n, t in head["props"]))


def _load_file(path: str, bg: bool, max_sh_degree: int, dev) -> Tuple[Dict[str, torch.Tensor], bool]:
    """({name: tensor on dev} of one file, whether the device path took it)."""
    with open(path, "rb") as fh:
        head = read_header(fh, path)
        if _device_path(head, max_sh_degree):
            names = [n for n, _t in head["props"]]
            table = column_table(names, bg, max_sh_degree)
            used = (table[6:] if not bg else np.concatenate((table[:3], table[6:])))
            if all(head["props"][i][1] == "f4" for i in used):
                rows, stride = head["count"], len(names)
                body = rows * stride * 4
                staged = torch.empty(body + table.nbytes, dtype=torch.uint8, pin_memory=True)
                view = staged.numpy()
                if fh.readinto(memoryview(view[:body])) != body:
                    raise ValueError(f"{path}: truncated vertex data")
                view[body:] = table.view(np.uint8)
                out = _empty_set(rows, bg, dev)
                if rows:
                    upload = staged.to(dev, non_blocking=True)                        # the file's ONE upload
                    m = _lib.ScgModel()
                    dst = m.bg if bg else m.ray
                    dst.count = rows
                    for n, t in out.items():
                        setattr(dst, n[3:] if bg else n, t.data_ptr())
                    with torch.cuda.device(dev):
                        _lib_io.check(_lib_io.load().scg_ply_unpack(
                            upload.data_ptr(), body, table.ctypes.data_as(C.POINTER(C.c_int32)), rows, stride, int(bg), C.byref(m),
                            _lib.stream_of(dev, "ply.load_ply")), "scg_ply_unpack")
                return out, True
    # any other PLY file: the host reader, one upload per tensor
    props = ply_io.read_vertex_ply(path)
    b = "b" if bg else ""
    dc, rest = ply_io._sh_from_columns(props, b + "f_dc_", b + "f_rest_", max_sh_degree)
    if (b + "opacity") not in props:
        raise ValueError(f"PLY file has no '{b}opacity' property")
    host = {"features_dc": dc, "features_rest": rest,
            "opacity": torch.from_numpy(props[b + "opacity"].astype(np.float32)[:, None].copy()),
            "scaling": torch.from_numpy(ply_io._columns(props, b + "scale_")),
            "rotation": torch.from_numpy(ply_io._columns(props, b + "rot"))}
    if bg:
        for k in ("bx", "by", "bz"):
            if k not in props:
                raise ValueError(f"PLY file has no '{k}' property")
        host["xyz"] = torch.from_numpy(np.stack((props["bx"], props["by"], props["bz"]), axis=1).astype(np.float32))
        return {"bg_" + n: t.to(dev) for n, t in host.items()}, False
    for k in ("zval", "rayo", "rayd"):
        host[k] = torch.from_numpy(ply_io._columns(props, k))
    return {n: t.to(dev) for n, t in host.items()}, False


@torch.no_grad()
def load_ply(gaussians, path: str, device="cuda") -> Dict[str, bool]:
    """GaussianModel.load_ply(path) (scene/gaussian_model.py:653-756): sets `_features_dc (P,1,3)`, `_features_rest (P,15,3)`,
    `_opacity`, `_scaling`, `_rotation`, `_zval` as nn.Parameter with requires_grad, `_rayo` / `_rayd` as plain tensors,
    `active_sh_degree = max_sh_degree`, and the six `bg_*` parameters only when point_cloud_bg.ply lies next to `path`.  On a
    ply_io.RayBoundModel the same tensors are set under its names (plain tensors).  Per file: one upload, one launch.
    Returns {"ray": took the device path, "bg": ... (absent without a background file)}."""
    dev = torch.device(device)
    if dev.type != "cuda":
        raise _err("load_ply builds the model on the ROCm GPU ('cuda'); ply_io.load_ply loads to the host")
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    max_sh = int(getattr(gaussians, "max_sh_degree", 3))
    took = {}
    ray, took["ray"] = _load_file(path, False, max_sh, dev)
    bg_path = os.path.join(os.path.dirname(os.path.abspath(path)), "point_cloud_bg.ply")
    bg = None
    if os.path.exists(bg_path):
        bg, took["bg"] = _load_file(bg_path, True, max_sh, dev)
    if isinstance(gaussians, ply_io.RayBoundModel):
        for n, t in ray.items():
            setattr(gaussians, n, t)
        for n, t in (bg or {}).items():
            setattr(gaussians, n, t)
    else:
        for n, t in ray.items():
            setattr(gaussians, "_" + n, t if n in ("rayo", "rayd") else torch.nn.Parameter(t.requires_grad_(True)))
        for n, t in (bg or {}).items():
            setattr(gaussians, n, torch.nn.Parameter(t.requires_grad_(True)))
    gaussians.active_sh_degree = max_sh
    if hasattr(gaussians, "__dict__"):
        gaussians.__dict__.pop("_scg_model_args", None)            # the render path's cache holds the old tensors alive
    return took


def install(gaussians) -> None:
    """Bind save_ply and load_ply as methods of this model instance under the reference's names: scene.save(iteration)
    (train.py:187) and Scene(..., load_iteration=...) run unchanged, and without plyfile."""
    gaussians.save_ply = functools.partial(save_ply, gaussians)
    gaussians.load_ply = functools.partial(load_ply, gaussians)

"""The scene files' bodies restated in numpy, for tests/test_ply_cpu.py and tests/test_gpu_ply.py (include/io/scg_ply.h).

A model is a dict of float32 arrays keyed like model_path.ARG_NAMES: zval (n,1), rayo / rayd (n,3), features_dc (n,1,3),
features_rest (n,15,3), opacity (n,1), scaling (n,3), rotation (n,4) and bg_xyz, bg_features_dc, ... for the background set.
Everything that is copied moves as uint32; what is computed is fp32, one numpy operation per rounding.
"""
import numpy as np

f32, u32 = np.float32, np.uint32
RAY_KEYS = ("zval", "rayo", "rayd", "features_dc", "features_rest", "opacity", "scaling", "rotation")
BG_KEYS = ("bg_xyz", "bg_features_dc", "bg_features_rest", "bg_opacity", "bg_scaling", "bg_rotation")
TAILS = {"zval": (1,), "rayo": (3,), "rayd": (3,), "features_dc": (1, 3), "features_rest": (15, 3), "opacity": (1,),
         "scaling": (3,), "rotation": (4,), "bg_xyz": (3,), "bg_features_dc": (1, 3), "bg_features_rest": (15, 3),
         "bg_opacity": (1,), "bg_scaling": (3,), "bg_rotation": (4,)}

# the byte-rule values of the issue; the second list is fixed by the rule alone (never compared with numpy's cast at run time)
PLANTED = [-450.3, -256, -255.9, -1, -0.5, -0.0, 0, 0.999, 1, 254.7, 255, 255.9, 256, 257.5, 450.2, 65536.7, 2147483520]
PLANTED_BEYOND = [2.0 ** 31, -2.0 ** 31, 3e9, -3e9, 2.0 ** 32, 1e19, 3e38, np.inf, -np.inf, np.nan]


def names(bg=False):
    p = "b" if bg else ""
    out = [p + "x", p + "y", p + "z", p + "nx", p + "ny", p + "nz"] + [f"{p}f_dc_{i}" for i in range(3)]
    out += [f"{p}f_rest_{i}" for i in range(45)] + [p + "opacity"] + [f"{p}scale_{i}" for i in range(3)]
    out += [f"{p}rot_{i}" for i in range(4)]
    if not bg:
        out += ["zval_0"] + [f"rayo_{i}" for i in range(3)] + [f"rayd_{i}" for i in range(3)]
    return out


COLOR_NAMES = ["x", "y", "z", "nx", "ny", "nz", "red", "green", "blue"]


def header(prop_names, n, types=None):
    types = types or ["float"] * len(prop_names)
    lines = ["ply", "format binary_little_endian 1.0", f"element vertex {n}"]
    lines += [f"property {t} {nm}" for nm, t in zip(prop_names, types)] + ["end_header"]
    return ("\n".join(lines) + "\n").encode("ascii")


def make_model(nr, nb, seed=0):
    rng = np.random.default_rng(seed)
    m = {}
    for keys, n in ((RAY_KEYS, nr), (BG_KEYS, nb)):
        for k in keys:
            m[k] = rng.normal(size=(n,) + TAILS[k]).astype(f32)
    return m


def bits(a):
    return np.ascontiguousarray(a, dtype=f32).view(u32)


def byte_rule(x):
    """B(x) in integer arithmetic on the bits of the float32 values: the low 8 bits of the two's-complement int32 of trunc(x) for
    a finite |x| < 2^31, 0 for everything else."""
    b = bits(np.asarray(x, dtype=f32)).astype(np.int64)
    sign, expo, mant = b >> 31, (b >> 23) & 0xFF, (b & 0x7FFFFF) | 0x800000
    e = expo - 127                                            # |x| = mant * 2^(e - 23) for a normal number
    up = np.clip(e - 23, 0, 8)                                # e <= 30: at most 7 places to the left
    down = np.clip(23 - e, 0, 63)
    mag = (mant << up) >> down                                # trunc(|x|); 0 for |x| < 1 (denormals included: expo 0, e = -127)
    mag = np.where((expo == 255) | (e >= 31) | (e < 0), 0, mag)
    return (np.where(sign == 1, -mag, mag) & 0xFF).astype(np.uint8)


def ray_xyz(m):
    prod = m["rayd"] * m["zval"]                              # one rounding
    return (m["rayo"] + prod).astype(f32)                     # and another


def _sh_channel_major(rest):
    """(n, 15, 3) -> (n, 45) with column c * 15 + j = element (j, c)."""
    return bits(rest).transpose(0, 2, 1).reshape(rest.shape[0], 45)


def pack_ray(m):
    """(nr, 69) uint32."""
    n = m["zval"].shape[0]
    return np.concatenate((bits(ray_xyz(m)), np.zeros((n, 3), u32), bits(m["features_dc"]).reshape(n, 3),
                           _sh_channel_major(m["features_rest"]), bits(m["opacity"]), bits(m["scaling"]), bits(m["rotation"]),
                           bits(m["zval"]), bits(m["rayo"]), bits(m["rayd"])), axis=1)


def pack_bg(m):
    """(nb, 62) uint32."""
    n = m["bg_xyz"].shape[0]
    return np.concatenate((bits(m["bg_xyz"]), np.zeros((n, 3), u32), bits(m["bg_features_dc"]).reshape(n, 3),
                           _sh_channel_major(m["bg_features_rest"]), bits(m["bg_opacity"]), bits(m["bg_scaling"]),
                           bits(m["bg_rotation"])), axis=1)


def all_xyz_bits(m):
    return np.concatenate((bits(ray_xyz(m)), bits(m["bg_xyz"])))


def _color_records(xyz_bits, rgb_bytes):
    n = xyz_bits.shape[0]
    rec = np.zeros((n, 27), np.uint8)
    rec[:, :12] = np.ascontiguousarray(xyz_bits).view(np.uint8).reshape(n, 12)
    rec[:, 24:] = rgb_bytes
    return rec


def pack_color(m):
    """(nr + nb, 27) uint8: colour = B(f_dc * 255), the product rounded to fp32."""
    dc = np.concatenate((m["features_dc"], m["bg_features_dc"])).reshape(-1, 3)
    with np.errstate(all="ignore"):
        prod = (dc * f32(255.0)).astype(f32)
    return _color_records(all_xyz_bits(m), byte_rule(prod))


C0 = f32(0.28209479177387814)
C1 = f32(0.4886025119029199)
C2 = [f32(v) for v in (1.0925484305920792, -1.0925484305920792, 0.31539156525252005, -1.0925484305920792, 0.5462742152960396)]
C3 = [f32(v) for v in (-0.5900435899266435, 2.890611442640554, -0.4570457994644658, 0.3731763325901154, -0.4570457994644658,
                       1.445305721320277, -0.5900435899266435)]


def eval_sh(deg, sh, x, y, z):
    """csrc/sh_eval.h in numpy fp32, operation by operation: sh (n, 16, 3) coefficient-major; returns (n, 3)."""
    two, three, four = f32(2.0), f32(3.0), f32(4.0)
    out = []
    for c in range(3):
        s = [sh[:, k, c] for k in range(16)]
        res = C0 * s[0]
        if deg > 0:
            res = res - (C1 * y) * s[1] + (C1 * z) * s[2] - (C1 * x) * s[3]
            if deg > 1:
                xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
                res = (res + (C2[0] * xy) * s[4] + (C2[1] * yz) * s[5] + (C2[2] * (two * zz - xx - yy)) * s[6]
                       + (C2[3] * xz) * s[7] + (C2[4] * (xx - yy)) * s[8])
                if deg > 2:
                    res = (res + ((C3[0] * y) * (three * xx - yy)) * s[9] + ((C3[1] * xy) * z) * s[10]
                           + ((C3[2] * y) * (four * zz - xx - yy)) * s[11]
                           + ((C3[3] * z) * (two * zz - three * xx - three * yy)) * s[12]
                           + ((C3[4] * x) * (four * zz - xx - yy)) * s[13] + ((C3[5] * z) * (xx - yy)) * s[14]
                           + ((C3[6] * x) * (xx - three * yy)) * s[15])
        out.append(res)
    return np.stack(out, axis=1).astype(f32)


def view_color(m, campos, deg):
    """max(eval_sh(deg, sh, dir) + 0.5, 0) * 255 in fp32 (n, 3), before the byte rule."""
    xyz = all_xyz_bits(m).view(f32)
    sh = np.concatenate((np.concatenate((m["features_dc"], m["bg_features_dc"])),
                         np.concatenate((m["features_rest"], m["bg_features_rest"]))), axis=1)
    cam = np.asarray(campos, dtype=f32).reshape(3)
    with np.errstate(all="ignore"):
        dx, dy, dz = xyz[:, 0] - cam[0], xyz[:, 1] - cam[1], xyz[:, 2] - cam[2]
        length = np.sqrt((dx * dx + dy * dy) + dz * dz)
        rgb = eval_sh(deg, sh, dx / length, dy / length, dz / length)
        r = rgb + f32(0.5)
        return (np.where(r < 0, f32(0.0), r) * f32(255.0)).astype(f32)


def pack_color_view(m, campos, deg):
    return _color_records(all_xyz_bits(m), byte_rule(view_color(m, campos, deg)))


def _suffixed(prop_names, prefix):
    got = [n for n in prop_names if n.startswith(prefix) and n[len(prefix):].lstrip("_").isdigit()]
    return sorted(got, key=lambda n: int(n.split("_")[-1]))


def column_table(prop_names, bg=False):
    """For each of the 69 (62) columns of names(bg): the index in prop_names it is loaded from (0 where nothing is loaded)."""
    b = "b" if bg else ""
    src = ([b + "x", b + "y", b + "z"] if bg else [None] * 3) + [None] * 3
    src += _suffixed(prop_names, b + "f_dc_") + _suffixed(prop_names, b + "f_rest_") + [b + "opacity"]
    src += _suffixed(prop_names, b + "scale_") + _suffixed(prop_names, b + "rot")
    if not bg:
        src += _suffixed(prop_names, "zval") + _suffixed(prop_names, "rayo") + _suffixed(prop_names, "rayd")
    assert len(src) == (62 if bg else 69), len(src)
    return np.array([0 if s is None else prop_names.index(s) for s in src], dtype=np.int32)


def unpack(body, table, bg=False):
    """body (rows, stride) uint32 + table -> {key: uint32 array shaped like the tensor}."""
    rows = body.shape[0]
    col = body[:, table]                                               # (rows, 69 or 62) in this project's own column order
    out = {"features_dc": col[:, 6:9].reshape(rows, 1, 3),
           "features_rest": col[:, 9:54].reshape(rows, 3, 15).transpose(0, 2, 1),
           "opacity": col[:, 54:55], "scaling": col[:, 55:58], "rotation": col[:, 58:62]}
    if bg:
        out["xyz"] = col[:, 0:3]
        return {"bg_" + k: np.ascontiguousarray(v) for k, v in out.items()}
    out.update(zval=col[:, 62:63], rayo=col[:, 63:66], rayd=col[:, 66:69])
    return {k: np.ascontiguousarray(v) for k, v in out.items()}

"""Records tests/golden/ref_depthviz.npz: what the libraries the reference's `visualization` calls (render.py:97-110,
render_video.py:98-113) produce on small planes.  Own calls of np.percentile, ndarray.min, matplotlib.colors.Normalize,
cm.ScalarMappable(cmap='turbo').to_rgba and the truncating casts; recorded with numpy 2.2.6 and matplotlib 3.10.8.

    python tests/golden/make_golden_depthviz.py

Per case <name>: <name>_x (H,W) fp32, <name>_p the percentile, <name>_vmin, <name>_vmax fp32 scalars, <name>_rgb (H,W,3) uint8.
`names` lists the cases.  frame_render (3,H,W) fp32 and frame_bgr (H,W,3) uint8: render_video.py:132,148 on a NaN-free image."""
import os
import warnings

import matplotlib as mpl
import matplotlib.cm as cm
import numpy as np

f32 = np.float32
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "ref_depthviz.npz")


def visualization(depth, p):
    """the reference's function with the percentile as a parameter and the file left out"""
    vmax = np.percentile(depth, p)
    vmin = depth.min()
    normalizer = mpl.colors.Normalize(vmin=vmin, vmax=vmax)
    mapper = cm.ScalarMappable(norm=normalizer, cmap='turbo')
    colormapped_im = (mapper.to_rgba(depth)[:, :, :3] * 255).astype(np.uint8)
    return f32(vmin), f32(vmax), colormapped_im


def normalised(d):
    return ((d - d.min()) / (d.max() - d.min())).astype(f32)


def cases():
    rng = np.random.default_rng(20)
    u = lambda h, w: rng.random((h, w), dtype=f32)          # noqa: E731
    out = {}
    out["one"] = (np.array([[0.37]], f32), 98)
    out["pair"] = (np.array([[0.75, 0.25]], f32), 98)
    out["rand_3x3"] = (u(3, 3), 98)
    out["rand_17x65"] = (u(17, 65), 98)
    base = u(9, 13)
    for p in (0, 50, 98, 100):
        out[f"p{p}_9x13"] = (base, p)
    out["constant"] = (np.full((5, 7), 0.625, f32), 98)
    x = u(6, 7); x[2, 3] = np.nan
    out["one_nan"] = (x, 98)
    out["all_nan"] = (np.full((4, 4), np.nan, f32), 98)
    x = u(5, 5); x[1, 1] = np.inf                            # n = 25: rank hi is the last one
    out["pos_inf_at_hi"] = (x, 98)
    x = u(10, 20); x[4, 4] = np.inf                          # n = 200: rank hi = 196, the +inf lies above it
    out["pos_inf_above"] = (x, 98)
    x = u(6, 6); x[0, 5] = -np.inf
    out["neg_inf_min"] = (x, 98)
    out["ties"] = ((np.floor(u(12, 11) * 6) / 8).astype(f32), 98)
    out["ties_p50"] = ((np.floor(u(12, 11) * 3) / 4).astype(f32), 50)
    out["mixed_sign"] = (((u(11, 9) - f32(0.5)) * f32(100)).astype(f32), 98)
    x = np.zeros((4, 6), f32); x[::2] = -0.0; x[1, 2] = 0.5; x[3, 3] = -0.25
    out["signed_zeros"] = (x, 50)
    x = (u(5, 8) * f32(1e-39)).astype(f32); x[0, 0] = 0
    out["denormals"] = (x, 98)
    yy, xx = np.mgrid[0:24, 0:32]
    out["depth_ramp"] = (normalised((3 + 0.1 * yy + 0.03 * xx + 0.2 * np.sin(xx / 3.0)).astype(f32)), 98)
    out["raw_depth"] = ((2 + 30 * u(13, 17) ** 2).astype(f32), 98)
    x = np.zeros((8, 25), f32); x.reshape(-1)[150:] = 1       # n = 200: ranks 195 and 196 inside the run of ones
    out["zero_one"] = (x, 98)
    return out


def main():
    warnings.simplefilter("ignore")
    rec = {}
    names = []
    with np.errstate(all="ignore"):
        for name, (x, p) in cases().items():
            x = np.ascontiguousarray(x, dtype=f32)
            vmin, vmax, rgb = visualization(x, p)
            assert rgb.shape == x.shape + (3,) and rgb.dtype == np.uint8
            names.append(name)
            rec.update({f"{name}_x": x, f"{name}_p": np.float64(p), f"{name}_vmin": vmin, f"{name}_vmax": vmax, f"{name}_rgb": rgb})
    rng = np.random.default_rng(21)
    render = (rng.random((3, 7, 9), dtype=f32) * f32(1.6) - f32(0.3)).astype(f32)
    render[:, 0, :4] = np.array([0.0, 1.0, 254.5 / 255, 1 / 255], f32)
    rec["frame_render"] = render
    rec["frame_bgr"] = np.ascontiguousarray((np.clip(render, 0., 1.).transpose(1, 2, 0) * 255.).astype(np.uint8)[..., ::-1])
    rec["names"] = np.array(names)
    np.savez_compressed(OUT, **rec)
    print(OUT, os.path.getsize(OUT), "bytes,", len(names), "cases")


if __name__ == "__main__":
    main()

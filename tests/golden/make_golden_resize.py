"""Records tests/golden/ref_resize.npz: what the reference's own PILtoTorch (utils/general_utils.py:22-28) returns for small `L` and
`RGB` images — Pillow's Image.resize with its default filter, / 255.0, permute.

    python tests/golden/make_golden_resize.py [path of the reference checkout]

Per case <name>: <name>_src uint8 (H, W) or (H, W, 3), <name>_res int64 (2,) = (width, height), <name>_out float32 (C, h, w).
`names` lists the cases, `pillow` is the version of Pillow that recorded them.  No source is larger than 64 x 48."""
import os
import sys

import numpy as np
from PIL import Image, __version__ as PILLOW

REFERENCE = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
sys.path.insert(0, REFERENCE)
from utils.general_utils import PILtoTorch  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "ref_resize.npz")


def step(h, w, c):
    y, x = np.mgrid[0:h, 0:w]
    planes = [(((x >= w // 2 - 3 + 3 * i) ^ (y >= h // 2 + 2 * i)) * 255).astype(np.uint8) for i in range(max(c, 1))]
    return np.stack(planes, axis=2) if c else planes[0]


def cases():
    rng = np.random.default_rng(19)
    u = lambda h, w, c: rng.integers(0, 256, (h, w, c) if c else (h, w), dtype=np.uint8)          # noqa: E731
    out = {}
    out["rgb_8x"] = (u(48, 64, 3), (8, 6))
    out["rgb_4x"] = (u(48, 64, 3), (16, 12))
    out["l_8x"] = (u(48, 64, 0), (8, 6))
    out["rgb_odd"] = (u(37, 53, 3), (7, 5))
    out["l_odd"] = (u(37, 53, 0), (11, 9))
    out["rgb_step_8x"] = (step(48, 64, 3), (8, 6))
    out["l_step_4x"] = (step(48, 64, 0), (16, 12))
    out["rgb_up"] = (u(5, 7, 3), (20, 9))
    out["rgb_width_only"] = (u(12, 40, 3), (13, 12))
    out["l_height_only"] = (u(30, 17, 0), (17, 7))
    out["rgb_same"] = (u(6, 5, 3), (5, 6))
    out["l_one"] = (u(1, 1, 0), (3, 2))
    out["rgb_to_one"] = (u(20, 33, 3), (1, 1))
    return out


def main():
    rec = {"names": np.array(sorted(cases())), "pillow": np.array(PILLOW)}
    for name, (src, res) in cases().items():
        assert src.shape[0] <= 48 and src.shape[1] <= 64
        got = PILtoTorch(Image.fromarray(src), res)
        rec[name + "_src"] = src
        rec[name + "_res"] = np.array(res, dtype=np.int64)
        rec[name + "_out"] = got.numpy().astype(np.float32, copy=False)
        assert got.dtype.is_floating_point and got.numpy().dtype == np.float32
    np.savez_compressed(OUT, **rec)
    print(OUT, os.path.getsize(OUT), "bytes; Pillow", PILLOW)


if __name__ == "__main__":
    main()

"""Records tests/golden/ref_jpegdec.npz: a handful of small baseline JPEG files with the pixels Pillow decodes them to, and one of
them through the reference's own PILtoTorch (utils/general_utils.py:22-28) as loadCam calls it on an opened file.

    python tests/golden/make_golden_jpegdec.py [path of the reference checkout]

Per case <name>: <name>_file uint8 (bytes of the file), <name>_pixels uint8 (H, W, 3) or (H, W) = np.asarray(Image.open(file)).
`names` lists the cases, `pillow` and `libjpeg` are the versions that recorded them.  piltotorch_res int64 (2,) = (width, height)
and piltotorch_out float32 (C, h, w) are PILtoTorch(Image.open(<rgb_420 written to disk>), res).  No image is larger than 40 x 56."""
import io
import os
import sys
import tempfile

import numpy as np
from PIL import Image, features, __version__ as PILLOW

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import jpegdec_refs as R  # noqa: E402

REFERENCE = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
sys.path.insert(0, REFERENCE)
from utils.general_utils import PILtoTorch  # noqa: E402

OUT = os.path.join(HERE, "ref_jpegdec.npz")


def cases():
    return {
        "rgb_420": R.pillow_file(R.image(40, 56, 3, "noise"), 90, "4:2:0"),
        "rgb_422_rst": R.pillow_file(R.image(37, 53, 3, "ramp"), 100, "4:2:2", restart_blocks=1),
        "rgb_444_opt": R.pillow_file(R.image(17, 33, 3, "noise"), 20, "4:4:4", optimize=True),
        "rgb_420_even": R.pillow_file(R.image(10, 10, 3, "noise"), 90, "4:2:0"),
        "l_odd": R.pillow_file(R.image(9, 9, 1, "noise"), 90),
        "rgb_one": R.pillow_file(R.image(1, 1, 3, "noise"), 90, "4:2:0"),
    }


def main():
    rec = {"names": np.array(sorted(cases())), "pillow": np.array(PILLOW), "libjpeg": np.array(str(features.version("jpg")))}
    for name, data in cases().items():
        rec[name + "_file"] = np.frombuffer(data, dtype=np.uint8)
        rec[name + "_pixels"] = np.asarray(Image.open(io.BytesIO(data)))
    res = (7, 5)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "rgb_420.jpg")
        with open(path, "wb") as fh:
            fh.write(cases()["rgb_420"])
        got = PILtoTorch(Image.open(path), res)
    rec["piltotorch_res"] = np.array(res, dtype=np.int64)
    rec["piltotorch_out"] = got.numpy().astype(np.float32, copy=False)
    np.savez_compressed(OUT, **rec)
    print(OUT, os.path.getsize(OUT), "bytes; Pillow", PILLOW)


if __name__ == "__main__":
    main()

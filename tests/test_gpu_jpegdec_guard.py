"""The JPEG decoder's compute entry under guard bands (tests/guarded_alloc.py): no 4096-byte band around a buffer is touched, every
device pointer the library is handed lies inside a guarded body, and the results with both fills and without a guard agree — which a
coefficient buffer, a counter or a state assumed clean would break, since every body starts poisoned.  Among the inputs are the
streams that lead threads into wrong states: a garbage tail, a file cut in the middle, and a first batch of sync rounds too short
to settle the states, after which count and write run from them."""
import functools

import numpy as np
import pytest
import torch

import jpegdec_refs as R
from guarded_alloc import FILL_A, FILL_B, guarded, traced
from scgaussian_amd import _lib_jpegdec, jpeg_decode

pytestmark = pytest.mark.gpu
DEV = "cuda"
POINTERS = {1: "header_dev", 2: "segment_dev", 4: "out", 6: "workspace"}          # the device pointers of scg_jpegdec_decode; 10: the stream


@functools.lru_cache(maxsize=None)
def _inputs():
    good = R.pillow_file(R.image(37, 53, 3, "noise"), 90, "4:2:0") if R.pillow_has_jpeg() else R.planted()["three_components_4:2:2"][0]
    info = jpeg_decode.parse(good)
    half = info.segment_start + (info.segment_end - info.segment_start) // 2
    out = {name: R.planted()[name][0] for name in ("ff00_across_border", "block_over_two_subsequences", "restart_every_mcu_row",
                                                   "three_components_4:4:4", "zigzag_63_and_dc_size_11")}
    out["one byte"] = R.segment_of_length(1)
    out["an encoder's file"] = good
    out["garbage tail"] = good[:info.segment_end] + bytes(range(1, 200)) * 3 + good[info.segment_end:]
    out["cut in the middle"] = good[:half] + b"\xff\xd9"
    out["cut inside a restart interval"] = (lambda d: d[:len(d) // 2] + b"\xff\xd9")(R.planted()["restart_every_mcu_row"][0])
    rng = np.random.default_rng(11)
    n = 900                                         # about 40 KB: a second workgroup, the smallest stream with rounds across them
    out["several workgroups"] = R.write_file(8, 8 * n, R.random_blocks(rng, n, 0.5, 30))
    return out


def _run(data, fill, first_rounds):
    jpeg_decode._PLANS.clear()                      # the workspace is allocated inside this run
    jpeg_decode.LAST.clear()
    info = jpeg_decode.parse(data)
    assert info is not None
    staged = jpeg_decode.stage(info, data)
    real, calls = _lib_jpegdec.load(), []
    _lib_jpegdec._lib = traced(real, calls)
    old = jpeg_decode.FIRST_ROUNDS
    jpeg_decode.FIRST_ROUNDS = first_rounds
    try:
        if fill is None:
            out, status = jpeg_decode.decode_staged(info, staged.to(DEV))
            torch.cuda.synchronize()
        else:
            with guarded(fill) as reg:
                upload = reg.rehome(staged.to(DEV))
                out, status = jpeg_decode.decode_staged(info, upload)
                torch.cuda.synchronize()
                touched = reg.check()
                assert touched == [], f"fill {fill}: {len(touched)} band(s) touched: {touched[:8]}"
                decodes = [c for c in calls if c.name == "scg_jpegdec_decode"]
                assert decodes
                for c in decodes:
                    seen = dict((path[0], value) for path, value in c.pointers)
                    for i, name in POINTERS.items():
                        assert seen.get(i) and reg.covers(seen[i]), f"{name} = {seen.get(i)} lies in no guarded body"
                out = out.cpu()
    finally:
        _lib_jpegdec._lib = real
        jpeg_decode.FIRST_ROUNDS = old
        jpeg_decode._PLANS.clear()
    return out.cpu().numpy(), [int(v) for v in status], len([c for c in calls if c.name == "scg_jpegdec_decode"])


NAMES = ("ff00_across_border", "block_over_two_subsequences", "restart_every_mcu_row", "three_components_4:4:4",
         "zigzag_63_and_dc_size_11", "one byte", "an encoder's file", "garbage tail", "cut in the middle", "cut inside a restart interval",
         "several workgroups")


def test_the_names_are_the_inputs():
    assert sorted(NAMES) == sorted(_inputs())


@pytest.mark.parametrize("name", NAMES)
def test_no_band_touched_every_pointer_guarded_and_the_fills_agree(name):
    data = _inputs()[name]
    damaged = name in ("garbage tail", "cut in the middle", "cut inside a restart interval")
    want = None if damaged else R.decode(data)
    for first_rounds in ((3, 1) if name == "several workgroups" else (3,)):
        runs = {fill: _run(data, fill, first_rounds) for fill in (FILL_A, FILL_B, None)}
        pixels, status, launches = runs[None]
        for fill in (FILL_A, FILL_B):
            assert runs[fill][1] == status and runs[fill][2] == launches, (name, fill, runs[fill][1:], status)
            assert np.array_equal(runs[fill][0], pixels), (name, fill, "the pixels depend on what lay in a buffer before the call")
        assert (status[0] != 0) == damaged, (name, status)
        if not damaged:
            assert np.array_equal(pixels, want), name
            assert launches == (2 if first_rounds == 1 else 1)

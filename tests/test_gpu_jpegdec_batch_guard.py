"""The batched JPEG decoder's compute entry under guard bands (tests/guarded_alloc.py), as tests/test_gpu_jpegdec_guard.py holds the
single entry: no 4096-byte band around a buffer is touched, every device pointer the library is handed lies inside a guarded body,
and the pixels and status words with both fills and without a guard agree.  Among the inputs are the wrong-state paths, where a
thread follows a false state: a garbage tail, two cut files, and ONE sync round on a stream of several workgroups."""
import functools

import numpy as np
import pytest
import torch

import jpegdec_refs as R
from guarded_alloc import FILL_A, FILL_B, guarded, traced
from scgaussian_amd import _lib_jpegdec, jpeg_decode

pytestmark = pytest.mark.gpu
DEV = "cuda"
POINTERS = {3: "table_dev", 4: "upload_dev", 6: "out", 8: "workspace"}          # the device pointers of scg_jpegdec_decode_batch


@functools.lru_cache(maxsize=None)
def _batches():
    good = R.pillow_file(R.image(37, 53, 3, "noise"), 90, "4:2:0") if R.pillow_has_jpeg() else R.planted()["three_components_4:2:2"][0]
    info = jpeg_decode.parse(good)
    half = info.segment_start + (info.segment_end - info.segment_start) // 2
    planted = R.planted()
    rows = planted["restart_every_mcu_row"][0]
    rng = np.random.default_rng(11)
    several = R.write_file(8, 8 * 900, R.random_blocks(rng, 900, 0.5, 30))          # about 40 KB: a second workgroup
    mixed = [planted[name][0] for name in ("ff00_across_border", "block_over_two_subsequences", "restart_every_mcu_row",
                                           "three_components_4:4:4", "zigzag_63_and_dc_size_11")]
    mixed += [R.segment_of_length(1), good, several, R.segment_of_length(129)]
    damaged = [R.segment_of_length(1), good[:info.segment_end] + bytes(range(1, 200)) * 3 + good[info.segment_end:], good,
               good[:half] + b"\xff\xd9", rows[:len(rows) // 2] + b"\xff\xd9", planted["ff00_across_border"][0]]
    # (name: files, sync rounds (None: max_rounds), the members whose status must not be 0)
    return {"mixed": (mixed, None, ()), "damaged": (damaged, None, (1, 3, 4)), "one round": ([good, several, R.segment_of_length(1)], 1, (1,))}


def _run(files, rounds, fill):
    infos = [jpeg_decode.parse(f) for f in files]
    assert all(i is not None for i in infos)
    stage = jpeg_decode.BatchStage(infos, files).plan()
    staged = torch.empty(stage.nbytes, dtype=torch.uint8, pin_memory=True)
    stage.fill(staged.numpy())
    rounds = stage.max_rounds if rounds is None else rounds
    real, calls = _lib_jpegdec.load(), []
    _lib_jpegdec._lib = traced(real, calls)
    try:
        if fill is None:
            upload = staged.to(DEV)
            out = torch.empty(stage.out_bytes, dtype=torch.uint8, device=DEV)
            ws = torch.empty(stage.workspace_bytes, dtype=torch.uint8, device=DEV)
            jpeg_decode.launch_batch(stage, upload, out, ws, rounds)
            torch.cuda.synchronize()
        else:
            with guarded(fill) as reg:
                upload = reg.rehome(staged.to(DEV))
                out = torch.empty(stage.out_bytes, dtype=torch.uint8, device=DEV)          # both start poisoned
                ws = torch.empty(stage.workspace_bytes, dtype=torch.uint8, device=DEV)
                jpeg_decode.launch_batch(stage, upload, out, ws, rounds)
                torch.cuda.synchronize()
                touched = reg.check()
                assert touched == [], f"fill {fill}: {len(touched)} band(s) touched: {touched[:8]}"
                batch = [c for c in calls if c.name == "scg_jpegdec_decode_batch"]
                assert len(batch) == 1
                seen = dict((path[0], value) for path, value in batch[0].pointers)
                for i, name in POINTERS.items():
                    assert seen.get(i) and reg.covers(seen[i]), f"{name} = {seen.get(i)} lies in no guarded body"
                out, ws = out.cpu(), ws[:16 * stage.n].cpu()
    finally:
        _lib_jpegdec._lib = real
    status = ws[:16 * stage.n].cpu().view(torch.int32).numpy().astype(np.int64).reshape(stage.n, 4) & 0xFFFFFFFF
    host = out.cpu().numpy()
    pixels = []
    for i in range(stage.n):
        at, shape = int(stage.out_offsets[i]), stage.shape(i)
        pixels.append(host[at:at + int(np.prod(shape))].reshape(shape).copy())
    return pixels, status


@pytest.mark.parametrize("name", ("mixed", "damaged", "one round"))
def test_no_band_touched_every_pointer_guarded_and_the_fills_agree(name):
    files, rounds, bad = _batches()[name]
    runs = {fill: _run(files, rounds, fill) for fill in (FILL_A, FILL_B, None)}
    pixels, status = runs[None]
    for fill in (FILL_A, FILL_B):
        assert np.array_equal(runs[fill][1], status), (name, fill, runs[fill][1].tolist(), status.tolist())
        for i, (a, b) in enumerate(zip(runs[fill][0], pixels)):
            assert np.array_equal(a, b), (name, fill, i, "the pixels depend on what lay in a buffer before the call")
    for i, data in enumerate(files):
        assert (int(status[i][0]) != 0) == (i in bad), (name, i, status.tolist())
        if i not in bad:
            assert np.array_equal(pixels[i], R.decode(data)), (name, i)
    if name == "one round":
        assert int(status[1][0]) & _lib_jpegdec.JPEGDEC_BAD_SYNC

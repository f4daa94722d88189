"""The JPEG decoder on the GPU (csrc/jpegunpack.hip through scgaussian_amd.jpeg_decode), held for EQUALITY OF BYTES to the numpy
restatement of its rule (tests/jpegdec_refs.py), to Pillow's pixels where Pillow reads JPEG, and to the recorded pixels of
tests/golden/ref_jpegdec.npz.  No tolerance exists in this file."""
import contextlib
import io
import os

import numpy as np
import pytest
import torch

import jpegdec_refs as R
from scgaussian_amd import _lib_jpegdec, images, jpeg, jpeg_decode

pytestmark = pytest.mark.gpu
DEV = "cuda"
S = R.SUBSEQ
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_jpegdec.npz")
HAS_PILLOW_JPEG = R.pillow_has_jpeg()
needs_pillow_jpeg = pytest.mark.skipif(not HAS_PILLOW_JPEG, reason="Pillow without JPEG")

# the issue's sizes, and two even ones that are no multiple of the MCU: only there does the last chroma sample of a row / the last
# chroma row reach a pixel through the edge rule
SIZES = [(1, 1), (2, 2), (7, 9), (8, 8), (16, 16), (17, 33), (8, 24), (24, 8), (9, 9), (3, 50), (37, 53), (10, 10), (12, 6)]


@contextlib.contextmanager
def host_reads():
    """Every transfer that leaves the device while the context is active, as (method, bytes): torch.Tensor.cpu / to / item / tolist
    of a device tensor that give something on the host, and copy_ from a device tensor into a host one (the idiom of
    tests/test_gpu_jpeg.py and tests/test_gpu_png.py).  Independent of what jpeg_decode reports about itself in LAST."""
    reads = []
    real = {n: getattr(torch.Tensor, n) for n in ("copy_", "cpu", "to", "item", "tolist")}

    def copy_(self, src, *a, **k):
        if not self.is_cuda and isinstance(src, torch.Tensor) and src.is_cuda:
            reads.append(("copy_", src.numel() * src.element_size()))
        return real["copy_"](self, src, *a, **k)

    def counted(name):
        def f(self, *a, **k):
            out = real[name](self, *a, **k)
            if self.is_cuda and not (isinstance(out, torch.Tensor) and out.is_cuda):
                reads.append((name, self.numel() * self.element_size()))
            return out
        return f

    try:
        torch.Tensor.copy_ = copy_
        for name in ("cpu", "to", "item", "tolist"):
            setattr(torch.Tensor, name, counted(name))
        yield reads
    finally:
        for name, fn in real.items():
            setattr(torch.Tensor, name, fn)


STATUS_READ = ("cpu", 16)                           # the four status words


def device_pixels(data, **kw):
    """decode() on the device route, or a failure: a test of the kernels must not pass through Pillow."""
    with host_reads() as reads:
        got = jpeg_decode.decode(data, DEV, **kw)
    assert jpeg_decode.LAST["route"] == "device" and jpeg_decode.LAST["status"] == 0, dict(jpeg_decode.LAST)
    assert reads == [STATUS_READ], reads            # the ordinary path: exactly ONE host read, of the status words
    assert jpeg_decode.LAST["host_reads"] == 1      # (what the module says of itself: a diagnostic)
    return got.cpu().numpy()


def check(data, what, pillow=True):
    want = R.decode(data)
    got = device_pixels(data)
    assert got.shape == want.shape and got.dtype == np.uint8, what
    assert np.array_equal(got, want), (what, int((got != want).sum()), "bytes differ from the restatement")
    if pillow and HAS_PILLOW_JPEG:
        assert np.array_equal(got, R.pillow_pixels(data)), (what, "differs from Pillow")
    return got


# ---- files an encoder wrote --------------------------------------------------------------------------------------------------------
@needs_pillow_jpeg
@pytest.mark.parametrize("quality", (20, 90, 100))
def test_sizes_samplings_and_one_component(quality):
    for (H, W) in SIZES:
        for sampling in R.SAMPLINGS:
            for restart_blocks in (0, 1):
                check(R.pillow_file(R.image(H, W, 3, "noise"), quality, sampling, restart_blocks), (H, W, sampling, quality, restart_blocks))
        check(R.pillow_file(R.image(H, W, 1, "noise"), quality), (H, W, "one component", quality))
        check(R.pillow_file(R.image(H, W, 3, "ramp"), quality, "4:2:0", optimize=True), (H, W, "optimize", quality))


def test_golden_files_and_the_references_own_piltotorch(tmp_path):
    z = np.load(GOLDEN)
    for name in z["names"]:
        data = z[f"{name}_file"].tobytes()
        got = device_pixels(data)
        assert np.array_equal(got, z[f"{name}_pixels"]), name
        assert np.array_equal(got, R.decode(data)), name
    path = str(tmp_path / "rgb_420.jpg")
    with open(path, "wb") as fh:
        fh.write(z["rgb_420_file"].tobytes())
    got = images.load_image(path, tuple(int(v) for v in z["piltotorch_res"]), DEV)
    assert jpeg_decode.LAST["route"] == "device"
    assert got.dtype == torch.float32 and np.array_equal(got.cpu().numpy().view(np.uint32), z["piltotorch_out"].view(np.uint32))


# ---- segment lengths ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("length", (1, S - 1, S, S + 1, 2 * S + 1))
def test_segment_lengths_around_the_subsequence(length):
    data = R.segment_of_length(length)
    assert R.segment_bytes(data) == length
    check(data, length)
    assert jpeg_decode.LAST["rounds"] == 1 and jpeg_decode.LAST["launched"] == 1          # one workgroup: one launch


@needs_pillow_jpeg
def test_a_segment_longer_than_one_workgroup_needs_rounds_across_workgroups(monkeypatch):
    data = R.pillow_file(R.image(160, 160, 3, "noise"), 100, "4:4:4")
    n = R.segment_bytes(data)
    assert n > 2 * R.THREADS * S and b"\xff\xd0" not in data                              # several workgroups, no restart marker
    want = check(data, "160 x 160 noise")
    rounds = jpeg_decode.LAST["rounds"]
    print(f"\n160 x 160 noise at quality 100: {n} bytes, {-(-n // S)} subsequences, sync settled after {rounds} launches")
    assert 1 < rounds <= 3
    # the result does not depend on the rounds run beyond convergence, nor on how they were batched
    for first, reads in ((8, 1), (1, 2), (2, 2)):
        monkeypatch.setattr(jpeg_decode, "FIRST_ROUNDS", first)
        with host_reads() as seen:
            got = jpeg_decode.decode(data, DEV)
        assert jpeg_decode.LAST["route"] == "device" and jpeg_decode.LAST["rounds"] == rounds, dict(jpeg_decode.LAST)
        assert seen == [STATUS_READ] * reads, (first, seen)                            # one more read per further batch of rounds
        assert jpeg_decode.LAST["host_reads"] == reads, (first, dict(jpeg_decode.LAST))
        assert np.array_equal(got.cpu().numpy(), want), first


# ---- planted streams ---------------------------------------------------------------------------------------------------------------
PLANTED = {"ff00_across_border": ["ff00_across_border", "code_16_bits"],
           "symbols_across_borders": ["code_across_border", "value_across_border"],
           "block_ends_on_border": ["block_ends_on_border"],
           "block_over_two_subsequences": ["block_over_two_subsequences"],
           "zigzag_63_and_dc_size_11": ["only_zigzag_63", "dc_size_11"],
           "restart_at_border": ["restart_at_border"],
           "restart_every_mcu": ["restart_index_wraps"],
           "restart_every_mcu_row": ["restart_index_wraps"],
           "three_components_4:4:4": ["code_across_border"],
           "three_components_4:2:2": ["code_across_border"]}


@pytest.mark.parametrize("name", sorted(PLANTED))
def test_planted_streams(name):
    data, stats = R.planted()[name]
    assert all(stats[c] > 0 for c in PLANTED[name]), (name, dict(stats))
    # (the writer's streams are no encoder's: the restatement is the reference; Pillow's range table may wrap where the rule saturates)
    check(data, name, pillow=False)
    print(f"\n{name}: {R.segment_bytes(data)} bytes, sync settled after {jpeg_decode.LAST['rounds']} launch(es)")


def test_the_planted_set_is_the_whole_list():
    assert set(R.planted()) == set(PLANTED)


# ---- damaged files -----------------------------------------------------------------------------------------------------------------
def _pillow_says(data):
    from PIL import Image
    try:
        return np.array(Image.open(io.BytesIO(data))), None
    except Exception as e:      # noqa: BLE001  (whatever Pillow raises is the behaviour to match)
        return None, type(e)


def _decode_says(data):
    try:
        return jpeg_decode.decode(data, DEV).cpu().numpy(), None
    except Exception as e:      # noqa: BLE001
        return None, type(e)


@needs_pillow_jpeg
def test_damaged_files_take_the_host_route_and_behave_as_pillow_does():
    good = R.pillow_file(R.image(37, 53, 3, "noise"), 90, "4:2:0")
    info = jpeg_decode.parse(good)
    truncated = good[:info.segment_start + (info.segment_end - info.segment_start) // 2]
    cut_with_eoi = truncated + b"\xff\xd9"                                  # parse accepts it: the kernels must find the blocks missing
    garbage_tail = good[:info.segment_end] + bytes(range(1, 200)) + good[info.segment_end:]
    cases = {"truncated": truncated, "cut, then EOI": cut_with_eoi, "garbage tail": garbage_tail}
    # a restart marker in front of the first block: no marker is due there, whatever its index
    rst = R.pillow_file(R.image(16, 32, 3, "noise"), 90, "4:4:4", restart_blocks=1)
    at = jpeg_decode.parse(rst).segment_start
    cases["RST7 in front of the first block"] = rst[:at] + b"\xff\xd7" + rst[at:]
    assert jpeg_decode.parse(cases["RST7 in front of the first block"]) is not None
    # a flipped bit that leaves a code word no table holds
    flipped = None
    for at in range(info.segment_start + 8, info.segment_end - 8):
        bad = bytearray(good)
        bad[at] ^= 0x7E
        if bad[at] == 0xFF or bad[at - 1] == 0xFF:
            continue
        bad = bytes(bad)
        if jpeg_decode.parse(bad) is None:
            continue
        _out, status = jpeg_decode.decode_staged(jpeg_decode.parse(bad), jpeg_decode.stage(jpeg_decode.parse(bad), bad).to(DEV))
        if int(status[0]) & _lib_jpegdec.JPEGDEC_BAD_CODE:
            flipped = bad
            break
    assert flipped is not None, "no flipped bit gave an invalid code"
    cases["flipped bit"] = flipped
    for what, data in cases.items():
        want, want_error = _pillow_says(data)
        got, got_error = _decode_says(data)
        assert jpeg_decode.LAST.get("route") != "device", what
        assert got_error is want_error, (what, got_error, want_error)
        if want is not None:
            assert np.array_equal(got, want), what
    assert jpeg_decode.parse(cut_with_eoi) is not None and jpeg_decode.parse(garbage_tail) is not None


# ---- the project's own videos ------------------------------------------------------------------------------------------------------
@needs_pillow_jpeg
def test_round_trip_of_the_projects_motion_jpeg(tmp_path):
    frames = [torch.from_numpy(R.image(37, 53, 3, kind, seed)).to(DEV) for kind, seed in (("noise", 1), ("ramp", 2), ("noise", 3))]
    for sub in ("4:2:0", "4:4:4"):
        files = jpeg.encode(frames, quality=90, subsampling=sub).files()
        path = str(tmp_path / f"v{sub[-1]}.avi")
        jpeg.write_avi(path, files, 24, 53, 37)
        back = jpeg.read_avi(path)
        assert back == files
        for f in back:
            assert jpeg_decode.parse(f).restart_interval == -(-53 // (16 if sub == "4:2:0" else 8))          # one interval per MCU row
            check(f, ("mjpeg", sub))


# ---- stability ---------------------------------------------------------------------------------------------------------------------
@needs_pillow_jpeg
def test_two_runs_a_side_stream_and_an_out_tensor_agree():
    data = R.pillow_file(R.image(120, 200, 3, "noise"), 95, "4:2:0")
    first = device_pixels(data)
    assert np.array_equal(first, R.pillow_pixels(data))
    jpeg_decode._PLANS.clear()                                               # a fresh workspace ...
    assert np.array_equal(device_pixels(data), first)
    assert np.array_equal(device_pixels(data), first)                        # ... and the one the first call left
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        got = jpeg_decode.decode(data, DEV)
    side.synchronize()
    assert np.array_equal(got.cpu().numpy(), first)
    out = torch.full((120, 200, 3), 7, dtype=torch.uint8, device=DEV)
    assert jpeg_decode.decode(data, DEV, out=out) is out and np.array_equal(out.cpu().numpy(), first)
    with pytest.raises(Exception, match="out must be"):
        jpeg_decode.decode(data, DEV, out=torch.empty((120, 200), dtype=torch.uint8, device=DEV))


# ---- images ------------------------------------------------------------------------------------------------------------------------
def _piltotorch(pil_image, resolution):
    """What PILtoTorch computes (utils/general_utils.py:22-28), stated here: Pillow's resize, / 255.0, channels first."""
    t = torch.from_numpy(np.array(pil_image.resize(resolution))) / 255.0
    return t.permute(2, 0, 1) if t.dim() == 3 else t.unsqueeze(dim=-1).permute(2, 0, 1)


def _bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.uint32)


@needs_pillow_jpeg
def test_images_decode_on_the_device_equals_piltotorch_and_the_default_route(tmp_path):
    from PIL import Image
    res = (63, 47)
    rng = np.random.default_rng(4)
    photo = np.clip(R.image(378, 504, 3, "ramp").astype(np.int64) + rng.integers(-24, 25, size=(378, 504, 3)), 0, 255).astype(np.uint8)
    for name, img in (("rgb.jpg", photo), ("l.jpg", photo[:, :, 1])):
        path = str(tmp_path / name)
        Image.fromarray(img).save(path, quality=90)
        want = _piltotorch(Image.open(path), res).to(DEV)
        images.load_image(path, res, DEV)                                        # (warm: the resize tables of this shape are uploaded once)
        with host_reads() as seen:
            direct = images.load_image(path, res, DEV)
        assert jpeg_decode.LAST["route"] == "device" and seen == [STATUS_READ], seen
        lazy = Image.open(path)
        assert images.lazily_opened_jpeg(lazy)
        with host_reads() as seen:
            through = images.pil_to_torch(lazy, res, DEV, decode="device")
        assert seen == [STATUS_READ], seen
        default = images.pil_to_torch(Image.open(path), res, DEV)
        for got in (direct, through, default):
            assert got.shape == want.shape and np.array_equal(_bits(got), _bits(want)), name
        loaded = Image.open(path)
        loaded.load()
        assert not images.lazily_opened_jpeg(loaded)

    class Module:
        PILtoTorch = None
    images.install(Module, decode="device")
    assert np.array_equal(_bits(Module.PILtoTorch(Image.open(path), res)), _bits(want))
    images.install(Module)
    assert Module.PILtoTorch is images.pil_to_torch


@needs_pillow_jpeg
def test_images_other_files_take_the_host_route_with_the_same_tensor(tmp_path):
    from PIL import Image
    res = (21, 13)
    rng = np.random.default_rng(5)
    rgba = rng.integers(0, 256, size=(40, 60, 4), dtype=np.uint8)
    png, prog = str(tmp_path / "a.png"), str(tmp_path / "p.jpg")
    Image.fromarray(rgba, "RGBA").save(png)
    Image.fromarray(rgba[:, :, :3]).save(prog, quality=90, progressive=True)
    for path in (png, prog):
        jpeg_decode.LAST.clear()
        want = _piltotorch(Image.open(path), res).to(DEV)
        got = images.load_image(path, res, DEV)
        assert jpeg_decode.LAST.get("route") != "device"
        assert got.shape == want.shape and np.array_equal(_bits(got), _bits(want)), path
        assert np.array_equal(_bits(images.pil_to_torch(Image.open(path), res, DEV, decode="device")), _bits(want))
    assert np.array_equal(jpeg_decode.decode(prog, DEV).cpu().numpy(), np.asarray(Image.open(prog)))
    assert jpeg_decode.LAST["route"] == "host"

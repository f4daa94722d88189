"""JPEG files packed on the GPU (scgaussian_amd/jpeg.py, csrc/jpegpack.hip) against the numpy restatement of tests/jpeg_refs.py
(held to Pillow's libjpeg by tests/test_jpeg_cpu.py) and, where Pillow has the codec, against Pillow itself.

The feature is integer arithmetic from end to end, so there is no tolerance anywhere: the device's file equals the restatement's and
Pillow's byte for byte.  Shapes are the smallest at which a path can go wrong: one block, one MCU, images that are no multiple of the
MCU, every kind of dummy block, segments of T - 1, T, T + 1 and 2 T + some blocks (T = 256 blocks per round, so that DC predictors
and dummy sources lie in the round before), a restart index past 7, a segment longer than the LDS window."""
import os

import numpy as np
import pytest
import torch

import jpeg_refs as R
from scgaussian_amd import _lib_jpg, jpeg

pytestmark = pytest.mark.gpu
DEV = "cuda"
T = _lib_jpg.JPEG_THREADS
u8 = np.uint8
PILLOW = R.pillow_has_jpeg()
SIZES = [(1, 1), (7, 9), (8, 8), (16, 16), (17, 33), (8, 24), (24, 8), (9, 9), (150, 17)]
QUALITIES = (1, 20, 50, 75, 95, 100)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=u8)).to(DEV)


def noise(rng, H, W, c=3):
    return rng.integers(0, 256, (H, W) if c == 1 else (H, W, c), dtype=u8)


def smooth(H, W, c=3, seed=0):
    yy, xx = np.mgrid[0:H, 0:W]
    a = ((np.sin(xx / 9.0 + seed) + np.cos(yy / 7.0)) * 60 + 128).astype(u8)
    return a if c == 1 else np.stack([a, a[::-1, ::-1], 255 - a], axis=2)


def check_files(files, images, quality=90, sub="4:2:0", bgr=False, stats=None, what=""):
    assert len(files) == len(images)
    for i, (f, a) in enumerate(zip(files, images)):
        want = R.encode(a, quality, sub, bgr, stats)
        assert f == want, f"{what} image {i} {np.shape(a)} q{quality} {sub}: {len(f)} bytes, the restatement has {len(want)}; first " \
                          f"difference at {next((k for k, (x, y) in enumerate(zip(f, want)) if x != y), min(len(f), len(want)))}"
        if PILLOW:
            assert f == R.pillow_encode(a, quality, sub, bgr), f"{what} image {i}: not Pillow's file"


def run(images, quality=90, sub="4:2:0", bgr=False, stats=None, what=""):
    packed = jpeg.encode([_t(a) for a in images], quality, sub, bgr)
    check_files(packed.files(), images, quality, sub, bgr, stats, what)
    return packed


# ---- sizes and qualities -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("quality", QUALITIES)
def test_small_sizes_both_subsamplings_and_one_component(quality):
    """Every size of the list in one batch per mode; 1 x 1 and its like need more than header + 3 H W bytes, so the batch also walks
    the overflow and retry path.  150 x 17 has 10 (4:2:0) and 19 (4:4:4) segments: the restart index passes 7."""
    rng = np.random.default_rng(quality)
    st = R.Stats()
    rgb = [noise(rng, H, W) for H, W in SIZES] + [smooth(17, 33)]
    for sub in R.SUBSAMPLINGS:
        packed = run(rgb, quality, sub, stats=st, what=sub)
        assert packed.retried
    run([noise(rng, H, W, 1) for H, W in SIZES] + [smooth(17, 33, 1)[:, :, None]], quality, "4:4:4", stats=st, what="one component")
    assert st["dummy_right"] and st["dummy_bottom"] and st["dummy_corner"] and st["segments"] > 2 * (19 + 10)


def test_segments_around_the_blocks_of_a_round():
    """One-component rows of T - 1, T and T + 1 blocks; 8 x 680 and 8 x 688 at 4:4:4 (255 and 258 blocks); 4:2:0 rows of 258 and 516
    blocks of height 8, where the bottom dummies' source and every predictor of a round's first blocks lie in the round before."""
    rng = np.random.default_rng(11)
    st = R.Stats()
    run([noise(rng, 8, 8 * n, 1) for n in (T - 1, T, T + 1)], 90, "4:4:4", stats=st, what="one component")
    run([noise(rng, 8, 680), noise(rng, 8, 688), smooth(8, 688)], 90, "4:4:4", stats=st, what="4:4:4")
    run([noise(rng, 8, 688), noise(rng, 8, 1376), smooth(24, 1370)], 90, "4:2:0", stats=st, what="4:2:0")
    assert st["dummy_bottom"] >= 2 * (43 + 86)


def test_planted_blocks_walk_every_branch_of_the_coder():
    rng = np.random.default_rng(12)
    st = R.Stats()
    run([np.full((8, 24), 77, u8), R.checkerboard(8, 16), R.dc_swing(8, 32)], 100, "4:4:4", stats=st, what="flat, checkerboard, swing")
    assert st["dc_diff0"] and st["ac_size10"] and st["dc_size11"]
    run([R.checkerboard(16, 32, 3)], 100, "4:2:0", stats=st)
    run([R.last_coefficient(3)], 75, "4:4:4", stats=st, what="zigzag 63 alone")
    assert st["zrl"] >= 9 and st["no_eob"] >= 3
    run([noise(np.random.default_rng(5), 8, 8, 1)], 100, "4:4:4", stats=st, what="a pad byte of FF")
    assert st["pad_ff"]
    before = st["long_segments"]
    run([noise(rng, 8, 1376), noise(rng, 16, 1376)], 100, "4:4:4", stats=st, what="noise at quality 100")
    run([noise(rng, 16, 1376)], 100, "4:2:0", stats=st, what="noise at quality 100")
    assert st["code16"] and st["ff_stuffed"] and st["long_segments"] - before >= 4 and st["window_straddle"] >= 4


def test_bgr_reads_the_bytes_in_reverse():
    rng = np.random.default_rng(13)
    imgs = [noise(rng, 17, 33), smooth(40, 56)]
    for sub in R.SUBSAMPLINGS:
        a = run(imgs, 90, sub, bgr=True).files()
        b = run([np.ascontiguousarray(x[:, :, ::-1]) for x in imgs], 90, sub).files()
        assert a == b != run(imgs, 90, sub).files()
    run([noise(rng, 9, 9, 1)], 90, "4:2:0", bgr=True)               # one component: subsampling and bgr change nothing


# ---- batches, capacity -----------------------------------------------------------------------------------------------------------------
def test_unequal_batch_starts_at_multiples_of_16_and_leaves_the_gaps():
    rng = np.random.default_rng(14)
    images = [smooth(40, 56), noise(rng, 24, 8), smooth(9, 100, 1), noise(rng, 33, 17), smooth(150, 17)]
    plan = jpeg.JpegPlan([a.shape for a in images], DEV, 85, "4:2:0", own_inputs=False)
    plan.out.fill_(0xEE)
    packed = plan.encode([_t(a) for a in images])
    files = packed.files()
    check_files(files, images, 85, "4:2:0")
    table, n = packed.table_host, len(images)
    out = plan.out.cpu().numpy()
    at = 0
    for i in range(n):
        off, size, need, flag = (int(v) for v in table[i])
        assert off == at and off % 16 == 0 and size == need == len(files[i]) and flag == 0
        at = (off + size + 15) // 16 * 16
        assert (out[off + size:min(at, out.size)] == 0xEE).all()
    assert [int(v) for v in table[n]] == [at, n, 0, 0] and (out[at:] == 0xEE).all() and at <= plan.layout.capacity


def test_a_file_that_does_not_fit_is_flagged_not_written_and_encoded_again():
    rng = np.random.default_rng(15)
    images = [smooth(40, 56), noise(rng, 24, 40), smooth(33, 17)]
    ts = [_t(a) for a in images]
    want = [R.encode(a, 100, "4:4:4") for a in images]
    caps = [len(want[0]), len(want[1]) - 1, len(want[2]) + 5]        # exact, one byte short, some room
    plan = jpeg.JpegPlan([a.shape for a in images], DEV, 100, "4:4:4", capacities=caps, own_inputs=False)
    plan.out.fill_(0xEE)
    packed = plan.encode(ts).to_host(retry=False)
    table = packed.table_host
    assert [int(v) for v in table[1]] == [(len(want[0]) + 15) // 16 * 16, 0, len(want[1]), 1]          # the need is still there
    assert [int(v) for v in table[0]] == [0, len(want[0]), len(want[0]), 0]
    assert [int(v) for v in table[2]] == [(len(want[0]) + 15) // 16 * 16, len(want[2]), len(want[2]), 0]   # it took no room
    assert packed.files() == [want[0], b"", want[2]] and packed.overflowed == [1] and int(table[3, 2]) == 1
    out = plan.out.cpu().numpy()
    written = np.zeros(out.size, bool)
    for off, size, _need, _flag in table[:3]:
        written[int(off):int(off) + int(size)] = True
    assert (out[~written] == 0xEE).all()                             # no byte of it, and none outside the neighbours' files
    again = jpeg.encode(ts, 100, "4:4:4", capacities=caps)
    assert again.files() == want and again.retried and again.overflowed == []
    assert not jpeg.encode(ts[::2], 100, "4:4:4").to_host().retried  # the default capacity holds the smooth ones


def test_empty_batch():
    packed = jpeg.encode([])
    assert packed.files() == [] and len(packed) == 0
    packed.write([])
    assert jpeg.encode(torch.zeros((0, 8, 8, 3), dtype=torch.uint8, device=DEV)).files() == []


# ---- determinism, streams, graphs, host reads ----------------------------------------------------------------------------------------
def test_two_runs_give_the_same_bytes_and_a_side_stream_works():
    rng = np.random.default_rng(2)
    images = [smooth(80, 210), noise(rng, 20, 20), smooth(33, 47, 1)]
    ts = [_t(a) for a in images]
    a, b = jpeg.encode(ts).files(), jpeg.encode(ts).files()
    assert a == b
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        c = jpeg.encode(ts).files()
    torch.cuda.current_stream().wait_stream(side)
    assert c == a
    check_files(a, images)
    batch = torch.stack([_t(smooth(24, 40, seed=s)) for s in range(3)])          # one (N, H, W, 3) tensor
    check_files(jpeg.encode(batch, 75, "4:4:4").files(), [smooth(24, 40, seed=s) for s in range(3)], 75, "4:4:4")


def test_encode_is_captured_and_replayed_on_rewritten_pixels():
    """The capture itself proves that encode reads nothing on the host: a synchronising call inside it would fail."""
    rng = np.random.default_rng(8)
    first = [smooth(40, 300), smooth(50, 60, 1), noise(rng, 24, 24)]
    second = [smooth(40, 300, seed=3), noise(rng, 50, 60, 1), noise(rng, 24, 24)]
    plan = jpeg.JpegPlan([a.shape for a in first], DEV, 90, "4:2:0")
    for t, a in zip(plan.inputs, first):
        t.copy_(_t(a).view(t.shape))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        plan.encode()                                           # warm: library loaded, tables uploaded
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        packed = plan.encode()
    for t, a in zip(plan.inputs, second):
        t.copy_(_t(a).view(t.shape))
    graph.replay()
    torch.cuda.synchronize()
    check_files(packed.files(), second)


def test_exactly_two_host_reads_per_batch(monkeypatch):
    rng = np.random.default_rng(4)
    images = [smooth(30, 100), noise(rng, 19, 19, 1), smooth(64, 64, 1)]
    ts = [_t(a) for a in images]
    jpeg.encode(ts).files()                                     # warm
    reads = []
    real_copy, real_cpu, real_to, real_item, real_tolist = (torch.Tensor.copy_, torch.Tensor.cpu, torch.Tensor.to, torch.Tensor.item,
                                                            torch.Tensor.tolist)

    def copy_(self, src, *a, **k):
        if not self.is_cuda and isinstance(src, torch.Tensor) and src.is_cuda:
            reads.append(("copy_", src.numel() * src.element_size()))
        return real_copy(self, src, *a, **k)

    def counted(name, real):
        def f(self, *a, **k):
            out = real(self, *a, **k)
            if self.is_cuda and not (isinstance(out, torch.Tensor) and out.is_cuda):
                reads.append((name, self.numel() * self.element_size()))
            return out
        return f

    monkeypatch.setattr(torch.Tensor, "copy_", copy_)
    for name, real in (("cpu", real_cpu), ("to", real_to), ("item", real_item), ("tolist", real_tolist)):
        monkeypatch.setattr(torch.Tensor, name, counted(name, real))
    packed = jpeg.encode(ts)
    assert reads == []                                          # the launches read nothing
    files = packed.files()
    total = int(packed.table_host[len(ts), 0])
    assert reads == [("copy_", 16 * (len(ts) + 1)), ("copy_", total)], reads
    packed.files(), packed.overflowed                           # no further read
    assert len(reads) == 2 and packed.host.is_pinned() and not packed.retried
    monkeypatch.undo()
    check_files(files, images)


def test_what_the_entry_points_refuse(tmp_path):
    from scgaussian_amd._lib import ScgError
    for bad in (torch.zeros((4, 4), dtype=torch.uint8), torch.zeros((4, 4), dtype=torch.float32, device=DEV),
                torch.zeros((4, 4, 2), dtype=torch.uint8, device=DEV), torch.zeros((8, 8, 3), dtype=torch.uint8, device=DEV)[:, ::2]):
        with pytest.raises(ScgError):
            jpeg.encode([bad])
    with pytest.raises(ScgError):
        jpeg.encode([_t(np.zeros((4, 4), u8))], quality=0)
    with pytest.raises(ScgError):
        jpeg.encode([_t(np.zeros((4, 4, 3), u8))], subsampling="4:2:2")
    img = smooth(21, 34)
    jpeg.save_jpeg(str(tmp_path / "a.jpg"), _t(img), 80, "4:4:4")
    check_files([open(tmp_path / "a.jpg", "rb").read()], [img], 80, "4:4:4")
    if PILLOW:
        jpeg.save_jpeg(str(tmp_path / "b.jpg"), torch.from_numpy(img), 80, "4:4:4")
        assert open(tmp_path / "b.jpg", "rb").read() == open(tmp_path / "a.jpg", "rb").read()


# ---- end to end ------------------------------------------------------------------------------------------------------------------------
def test_render_video_writes_two_motion_jpeg_files(tmp_path):
    import test_gpu_png as P
    from scgaussian_amd import video
    views, model, pipe, bg = P._scene()
    frames, depths = [], []
    oa = video.render_video(views, model, pipe, bg, out_dir=str(tmp_path / "a"), iteration=7)
    ob = video.render_video(views, model, pipe, bg, out_dir=str(tmp_path / "b"), iteration=7, video="mjpeg", fps=24, jpeg_quality=85,
                            frame_sink=frames.append, depth_sink=depths.append)
    assert all(np.array_equal(oa[k], ob[k]) for k in video.VIDEO_KEYS)
    ta, tb = P._tree(tmp_path / "a"), P._tree(tmp_path / "b")
    assert not any(r.endswith(".avi") for r in ta) and len(ta) == 9          # the default call writes no video
    base = os.path.join("video", "ours_7")
    assert sorted(tb) == sorted(list(ta) + [os.path.join(base, "render_video.avi"), os.path.join(base, "depth_video.avi")])
    for rel in ta:
        assert open(ta[rel], "rb").read() == open(tb[rel], "rb").read(), rel
    assert len(frames) == len(depths) == len(views) and all(np.array_equal(f, g) for f, g in zip(frames, ob["frames_bgr"]))
    H, W = ob["frames_bgr"].shape[1:3]
    for name, key in (("render_video.avi", "frames_bgr"), ("depth_video.avi", "depth_frames_bgr")):
        avi = R.parse_avi(open(tb[os.path.join(base, name)], "rb").read())
        assert avi["avih"]["total_frames"] == len(views) and (avi["avih"]["width"], avi["avih"]["height"]) == (W, H)
        assert (avi["strh"]["rate"], avi["strh"]["scale"], avi["strh"]["handler"]) == (24, 1, b"MJPG") and len(avi["index"]) == len(views)
        check_files([f for _p, f in avi["frames"]], list(ob[key]), 85, "4:2:0", bgr=True, what=name)
        if PILLOW:
            import io

            from PIL import Image
            assert Image.open(io.BytesIO(avi["frames"][0][1])).size == (W, H)
    with pytest.raises(ValueError):
        video.render_video(views, model, pipe, bg, video="mp4")
    from scgaussian_amd._lib import ScgError
    with pytest.raises(ScgError):
        video.render_video(views, model, pipe, bg, video="mjpeg", jpeg_quality=0)

"""PNG files packed on the GPU (scgaussian_amd/png.py, csrc/pngpack.hip) against the numpy restatement of tests/png_refs.py (held to
zlib and Pillow by tests/test_png_cpu.py).

Every image is checked three ways: the device's file equals the restatement's file bit for bit; zlib.decompress of its IDAT equals
the filtered stream (which verifies the Adler-32); Pillow's decode equals the source.  The feature is integer arithmetic from end to
end, so there is no tolerance anywhere.  Shapes are the smallest at which a path can go wrong: streams of one to three chunks of
C = 32768 bytes, a thread's 128-byte segment, a match's 258 bytes.  A one-channel 1 x W image under filter None without
gray_as_rgb has the stream [0, pixels...], so the tests plant streams directly (png_refs.image_of_stream)."""
import os
import types
import zlib

import numpy as np
import pytest
import torch

import png_refs as R
from scgaussian_amd import _lib_png, png

pytestmark = pytest.mark.gpu
DEV = "cuda"
C = _lib_png.PNG_CHUNK
u8 = np.uint8


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=u8)).to(DEV)


def check_files(files, images, filt=R.UP, gray=True, what=""):
    """The three checks per image; returns the restatement's per-chunk dicts, per image."""
    infos = []
    assert len(files) == len(images)
    for i, (f, a) in enumerate(zip(files, images)):
        ch = []
        want = R.png_file(a, filt, gray, ch)
        assert f == want, f"{what} image {i} {np.shape(a)} filter {filt}: {len(f)} bytes, the restatement has {len(want)}; first " \
                          f"difference at {next((k for k, (x, y) in enumerate(zip(f, want)) if x != y), min(len(f), len(want)))}"
        assert zlib.decompress(R.idat_of(f)) == R.filtered_stream(a, filt, gray).tobytes()
        assert np.array_equal(R.decode_with_pillow(f), R.expected_pixels(a, gray))
        infos.append(ch)
    return infos


def run(images, filt=R.UP, gray=True, what=""):
    packed = png.encode([_t(a) for a in images], filter=filt, gray_as_rgb=gray)
    infos = check_files(packed.files(), images, filt, gray, what)
    if images:                                                  # what the count kernel left per chunk, stored chunks included
        flat = [c for ch in infos for c in ch]
        lengths, info = packed.plan.chunk_lengths(), packed.plan.chunk_info()
        assert lengths.shape == (len(flat), 288) and (lengths[:, 286:] == 1).all()
        assert [list(row[:286]) for row in lengths] == [c["lengths"] for c in flat], what
        assert [int(b) for b in info[:, 0]] == [c["bytes"] for c in flat]
    return packed, infos


def planted(d):
    """(packed, the chunk dicts) of the stream d as a one-channel image under filter None."""
    packed, infos = run([R.image_of_stream(d)], R.NONE, False)
    return packed, infos[0]


def noise(rng, *shape):
    return rng.integers(0, 256, shape, dtype=u8)


def smooth(H, W, channels=3, seed=0):
    yy, xx = np.mgrid[0:H, 0:W]
    planes = [((np.sin(xx / (9.0 + k + seed)) + np.cos(yy / (7.0 + 2 * k))) * 60 + 128).astype(u8) for k in range(channels)]
    return np.stack(planes, axis=2) if channels == 3 else planes[0]


# ---- stream lengths at the chunk border ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [C - 1, C, C + 1, 2 * C - 1, 2 * C, 2 * C + 2])
def test_stream_lengths_around_one_and_two_chunks(S):
    """One-channel 1 x W images at W = S - 1.  Behind two chunks the first stream an image can have is 2 C + 2, as two rows:
    2 C + 1 = 65537 is prime, so only 1 x 65536 would give it, and W ends at 65535."""
    rng = np.random.default_rng(S)
    H = 2 if S == 2 * C + 2 else 1
    W = S // H - 1
    img = (rng.integers(0, 4, (H, W)) * (rng.random((H, W)) < 0.3)).astype(u8)                  # short runs and single bytes
    for filt in (R.NONE, R.SUB):
        _packed, infos = run([img], filt, False, f"S={S}")
        assert len(infos[0]) == -(-S // C) and [c["n"] for c in infos[0]][-1] == S - (len(infos[0]) - 1) * C


@pytest.mark.parametrize("W", [10922, 10923])
def test_rgb_rows_at_the_chunk_border(W):
    """1 + 3 W = 32767 and 32770: a row that ends one byte before the chunk's end, and one that crosses it."""
    img = smooth(3, W, 3)
    for filt in (R.UP, R.PAETH):
        run([img], filt, True, f"W={W}")


# ---- image shapes, filters, wrapping ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("filt", R.FILTERS)
def test_small_shapes_every_filter_and_wrapping_bytes(filt):
    rng = np.random.default_rng(filt)
    wrap = np.array([[0, 255, 0, 255, 1], [255, 0, 255, 0, 254], [0, 0, 255, 255, 128]], dtype=u8)       # differences that wrap
    images = [np.zeros((1, 1), u8), np.full((1, 1, 3), 255, u8), noise(rng, 1, 37), noise(rng, 37, 1), noise(rng, 1, 9, 3),
              noise(rng, 9, 1, 3), wrap, np.stack([wrap, wrap[::-1], 255 - wrap], axis=2), smooth(31, 45, 3), smooth(31, 45, 1),
              noise(rng, 5, 7, 1)]
    for gray in (True, False):
        run(images, filt, gray, f"gray_as_rgb={gray}")


def test_paeth_first_row_first_column_and_ties():
    """The first row predicts from the left alone, the first column from above alone; a == b == c and the two-way ties take left,
    then up."""
    rng = np.random.default_rng(3)
    tie = np.array([[10, 10, 10], [10, 10, 20], [20, 10, 10], [7, 9, 8]], dtype=u8)
    run([tie, np.repeat(tie[:, :, None], 3, axis=2), noise(rng, 6, 5, 3), smooth(40, 300, 3)], R.PAETH, True)


# ---- run lengths -----------------------------------------------------------------------------------------------------------------
def test_run_lengths_around_the_literal_and_match_thresholds():
    lengths = [1, 2, 3, 4, 5, 258, 259, 260, 261, 262, 263] + [1 + 2 * 258 + k for k in range(4)] + [127, 128, 129, 1, 1, 300]
    d = R.runs_stream(lengths)
    _packed, info = planted(d)
    assert info[0]["kind"] == "dynamic" and info[0]["matches"] > 0
    # the same runs in another order, so that every one of them meets other thread borders
    planted(R.runs_stream(lengths[::-1]))


def test_runs_at_the_chunk_border():
    """A run that ends exactly at a chunk's end with the next one starting on the next chunk's first byte; a run that crosses the
    border (it is cut there: nothing refers across); short runs on both sides."""
    planted(R.runs_stream([C - 300, 300, 500, 3, 2, 700]))
    planted(R.runs_stream([C - 100, 400, 5, 1, 600]))
    planted(R.runs_stream([C - 2, 1, 1, 1, 1, 2000]))
    planted(R.runs_stream([C - 3, 6, 40]))


def test_a_whole_chunk_of_one_value_and_a_chunk_without_a_match():
    _p, info = planted(np.zeros(C, u8))
    assert info[0]["tokens"] == 1 + (C - 1) // 258 + 1 and info[0]["matches"] == (C - 1) // 258 and info[0]["bytes"] < 200
    d = (np.arange(C) % 3).astype(u8)                                    # three values in turn: no run of two, every token a literal
    _p, info = planted(d)
    assert info[0]["matches"] == 0 and info[0]["tokens"] == C and info[0]["kind"] == "dynamic"


# ---- histograms ------------------------------------------------------------------------------------------------------------------
def test_one_literal_value_gives_two_codes_of_one_bit():
    for n in (2, 3):                                                    # below four bytes a run is literals
        _p, info = planted(np.zeros(n, u8))
        assert sorted(l for l in info[0]["lengths"] if l) == [1, 1] and info[0]["matches"] == 0


def test_fibonacci_and_lucas_chunks():
    """The planted histograms.  Under the rule's "leaf on a tie" the Fibonacci counts, which tie at every step, give an unlimited
    tree 11 deep; the Lucas counts tie nowhere, give a chain 19 deep and so bring the limit of 15 and the repair into play."""
    _p, info = planted(R.fibonacci_stream())
    assert info[0]["n"] == 28656 and info[0]["deepest"] == 11 and info[0]["kind"] == "dynamic"
    _p, info = planted(R.lucas_stream())
    assert info[0]["deepest"] > 15 and max(info[0]["lengths"]) == 15 and info[0]["kind"] == "dynamic"


# ---- stored fallback -------------------------------------------------------------------------------------------------------------
def test_noise_is_stored_and_mixtures_fall_on_both_sides():
    rng = np.random.default_rng(11)
    packed, infos = run([noise(rng, 60, 200, 3), noise(rng, 1, C - 1)], R.NONE, False)
    assert all(c["kind"] == "stored" for ch in infos for c in ch)
    assert (packed.plan.chunk_info()[:, 1] == _lib_png.PNG_KIND_STORED).all()
    images = []
    for share in (0.5, 0.9, 0.96, 0.98, 0.99, 0.995, 1.0):             # the share of noise in a chunk; the rest one run of zeros
        d = np.zeros(C, u8)
        k = int(share * (C - 1))
        d[C - k:] = noise(rng, k)
        images.append(R.image_of_stream(d))
    d = np.concatenate([noise(rng, C), np.zeros(C, u8), noise(rng, C)])                        # stored, dynamic, stored in one image
    d[0] = 0                                                   # two rows of 1.5 C bytes: the second filter byte lies among the zeros
    three = np.ascontiguousarray(d.reshape(2, 3 * C // 2)[:, 1:])
    packed, infos = run(images + [three], R.NONE, False)
    kinds = [c["kind"] for ch in infos for c in ch]
    assert "stored" in kinds and "dynamic" in kinds and kinds[0] == "dynamic" and kinds[6] == "stored"
    assert [c["kind"] for c in infos[-1]] == ["stored", "dynamic", "stored"]
    assert [("dynamic", "stored")[k] for k in packed.plan.chunk_info()[:, 1]] == kinds
    for ch in infos:
        for c in ch:
            assert c["bytes"] <= c["n"] + 5


def test_adler_sums_of_a_full_chunk_of_ff():
    """255 * 32768 * 32769 / 2 exceeds 32 bits: the weighted sum of one chunk is formed in 64."""
    d = np.full(2 * C, 255, u8)
    d[0] = 0
    _p, info = planted(d)
    assert len(info) == 2


# ---- batches ---------------------------------------------------------------------------------------------------------------------
def test_an_empty_batch_and_one_image():
    packed = png.encode([])
    assert len(packed) == 0 and packed.files() == [] and packed.to_host().host is None
    packed.write([])
    run([smooth(20, 30, 3)])


def test_unequal_images_whose_chunks_interleave():
    rng = np.random.default_rng(5)
    images = [smooth(70, 200, 3), noise(rng, 3, 5, 3), smooth(130, 300, 1), np.zeros((1, 1), u8), smooth(64, 171, 3, seed=4),
              (rng.random((90, 400)) < 0.5).astype(u8) * 255]
    packed, infos = run(images, R.UP, True)
    assert [len(ch) for ch in infos] == [2, 1, 4, 1, 2, 4]
    # a short image between two long ones, every filter
    for filt in R.FILTERS:
        run([smooth(60, 200, 3), noise(rng, 2, 2, 3), smooth(60, 200, 3, seed=2)], filt, True)


def test_1025_images_of_one_pixel():
    """More images and chunks than one pass of the scan workgroup holds (256 per pass, four passes and one more)."""
    rng = np.random.default_rng(9)
    images = [noise(rng, 1, 1, 3 if i % 3 == 0 else 1) for i in range(1025)]
    packed, _ = run(images, R.UP, True)
    table = packed.table_host
    assert int(table[1025, 1]) == 1025 and (table[:1025, 0] == 16 * np.arange(1025)).all()


def test_streams_start_at_multiples_of_16_and_gaps_are_nobodys():
    rng = np.random.default_rng(6)
    images = [smooth(50, 223, 3), noise(rng, 7, 11, 1), smooth(1, 5000, 1), noise(rng, 1, 1, 1), smooth(33, 77, 3)]
    plan = png.PngPlan([a.shape for a in images], DEV, png.UP, True, own_inputs=False)
    plan.out.fill_(0xEE)
    packed = plan.encode([_t(a) for a in images]).to_host()
    check_files(packed.files(), images)
    table, host = packed.table_host, packed.host.numpy()
    n = len(images)
    assert (table[:n, 0] % 16 == 0).all() and table[0, 0] == 0
    for i in range(n):
        end = int(table[i, 0]) + int(table[i, 1])
        nxt = int(table[i + 1, 0]) if i + 1 < n else int(table[n, 0])
        assert nxt == (end + 15) // 16 * 16 and (host[end:nxt] == 0xEE).all()                # never written, never in a file
        assert end - int(table[i, 0]) <= R.stream_geometry(*R.as_hwc(images[i]).shape, True)[1] + 5 * len(
            range(R.stream_geometry(*R.as_hwc(images[i]).shape, True)[2])) + 6
    assert host.size == int(table[n, 0]) <= plan.layout.capacity
    dev_out = plan.out.cpu().numpy()
    assert (dev_out[int(table[n, 0]):] == 0xEE).all()                                          # nothing behind the total either


# ---- determinism, streams, graphs, host reads --------------------------------------------------------------------------------------
def test_two_runs_give_the_same_bytes_and_a_side_stream_works():
    rng = np.random.default_rng(2)
    images = [smooth(80, 210, 3), (rng.random((100, 350)) < 0.02).astype(u8) * 200, noise(rng, 20, 20, 3)]
    ts = [_t(a) for a in images]
    a, b = png.encode(ts).files(), png.encode(ts).files()
    assert a == b
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        c = png.encode(ts).files()
    torch.cuda.current_stream().wait_stream(side)
    assert c == a
    check_files(a, images)


def test_encode_is_captured_and_replayed_on_rewritten_pixels():
    """The capture itself proves that encode reads nothing on the host: a synchronising call inside it would fail."""
    rng = np.random.default_rng(8)
    first = [smooth(40, 300, 3), smooth(50, 60, 1), noise(rng, 4, 4, 3)]
    second = [smooth(40, 300, 3, seed=3), (rng.random((50, 60)) < 0.1).astype(u8) * 255, noise(rng, 4, 4, 3)]
    plan = png.PngPlan([a.shape for a in first], DEV)
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
    images = [smooth(30, 100, 3), noise(rng, 9, 9, 1), smooth(64, 64, 1)]
    ts = [_t(a) for a in images]
    png.encode(ts).files()                                      # warm
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
    packed = png.encode(ts)
    assert reads == []                                          # the launches read nothing
    files = packed.files()
    total = int(packed.table_host[len(ts), 0])
    assert reads == [("copy_", 8 * (len(ts) + 1)), ("copy_", total)], reads
    packed.files(), packed.streams()                            # no further read
    assert len(reads) == 2 and packed.host.is_pinned()
    monkeypatch.undo()
    check_files(files, images)


# ---- gray_as_rgb -----------------------------------------------------------------------------------------------------------------
def test_gray_as_rgb_decodes_to_three_equal_channels_without_an_expanded_tensor():
    img = smooth(200, 300, 1)
    t = _t(img)
    png.encode([t]).files()                                     # warm
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    packed = png.encode([t], gray_as_rgb=True)
    torch.cuda.synchronize()
    grown = torch.cuda.max_memory_allocated() - before
    plan = packed.plan
    own = plan.out.numel() + plan.workspace.numel() + plan.images_dev.numel() + plan.chunks_dev.numel()
    assert grown <= own + 4 * 512, (grown, own)                 # the plan's four buffers (rounded to the allocator's 512) and nothing
    assert 3 * img.size > 16 * 512                              # ... where an expanded copy would be 180 000 bytes
    f = packed.files()[0]
    px = R.decode_with_pillow(f)
    assert px.shape == (200, 300, 3) and (px == img[:, :, None]).all()
    check_files([f], [img], R.UP, True)
    g = png.encode([t], gray_as_rgb=False).files()[0]
    assert R.decode_with_pillow(g).shape == (200, 300) and len(g) < len(f)
    check_files([g], [img], R.UP, False)


def test_what_the_entry_points_refuse(tmp_path):
    from scgaussian_amd._lib import ScgError
    with pytest.raises(ScgError):
        png.encode([torch.zeros((4, 4), dtype=torch.uint8)])                       # a host tensor
    with pytest.raises(ScgError):
        png.encode([torch.zeros((4, 4), dtype=torch.float32, device=DEV)])
    with pytest.raises(ScgError):
        png.encode([torch.zeros((4, 4, 2), dtype=torch.uint8, device=DEV)])
    with pytest.raises(ScgError):
        png.encode([_t(np.zeros((4, 4), u8))], filter=3)                           # Average is not offered
    # save_png: the kernels for what they take, Pillow for the rest
    img = smooth(21, 34, 3)
    png.save_png(str(tmp_path / "a.png"), _t(img))
    png.save_png(str(tmp_path / "b.png"), torch.from_numpy(img))
    check_files([open(tmp_path / "a.png", "rb").read()], [img])
    assert np.array_equal(R.decode_with_pillow(open(tmp_path / "b.png", "rb").read()), img)


# ---- end to end ------------------------------------------------------------------------------------------------------------------
def _scene(W=56, H=40):
    from scgaussian_amd import render as rmod
    from scgaussian_amd import synthetic as syn
    sc = syn.make_scene(1500, W, H, seed=5)
    model = syn.make_raw_model(sc).to(DEV)
    model.active_sh_degree = 3
    bg = torch.zeros(3, device=DEV)
    pipe = rmod.PipelineParams()
    views = []
    for i, yaw in enumerate((0.0, 8.0, -6.0)):
        cam = syn.orbit_camera(W, H, yaw, -2.0, 7.0).to(DEV)
        gt = torch.rand(3, H, W, device=DEV, generator=torch.Generator(DEV).manual_seed(i))
        mask = (torch.rand(1, H, W, device=DEV, generator=torch.Generator(DEV).manual_seed(10 + i)) < 0.7).float() if i == 1 else None
        views.append(types.SimpleNamespace(**cam._asdict(), original_image=gt, dtumask=mask, idx=i))
    return views, model, pipe, bg


def _tree(root):
    out = {}
    for folder, _dirs, names in os.walk(root):
        for n in names:
            path = os.path.join(folder, n)
            out[os.path.relpath(path, root)] = path
    return out


def _same_trees(a, b, count):
    ta, tb = _tree(a), _tree(b)
    assert sorted(ta) == sorted(tb) and len(ta) == count
    for rel in ta:
        fa, fb = open(ta[rel], "rb").read(), open(tb[rel], "rb").read()
        pa, pb = R.decode_with_pillow(fa), R.decode_with_pillow(fb)
        assert pa.shape == pb.shape and pa.dtype == pb.dtype and np.array_equal(pa, pb), rel
        assert zlib.decompress(R.idat_of(fb))                                      # one IDAT, every CRC right
        assert fb == R.png_file(pa, R.UP, True), rel                               # and the device's file is the rule's


def test_render_set_writes_the_same_tree_either_way(tmp_path):
    from scgaussian_amd import evaluate
    views, model, pipe, bg = _scene()
    ra = evaluate.render_set(views, model, pipe, bg, out_dir=str(tmp_path / "a"), iteration=7, color_depth=True)
    rb = evaluate.render_set(views, model, pipe, bg, out_dir=str(tmp_path / "b"), iteration=7, color_depth=True, png="device")
    assert ra[0] == rb[0] and ra[1] == rb[1]
    _same_trees(tmp_path / "a", tmp_path / "b", 3 * 5 + 1)                         # one view has a mask
    with pytest.raises(ValueError):
        evaluate.render_set(views, model, pipe, bg, png="zlib")


def test_render_video_writes_the_same_tree_either_way(tmp_path):
    from scgaussian_amd import video
    views, model, pipe, bg = _scene()
    oa = video.render_video(views, model, pipe, bg, out_dir=str(tmp_path / "a"), iteration=7)
    ob = video.render_video(views, model, pipe, bg, out_dir=str(tmp_path / "b"), iteration=7, png="device")
    assert all(np.array_equal(oa[k], ob[k]) for k in video.VIDEO_KEYS)
    _same_trees(tmp_path / "a", tmp_path / "b", 9)


def test_snapshot_writes_the_same_planes_either_way(tmp_path):
    import matchpoint_refs as MR
    from scgaussian_amd import matchpoint
    arena = MR.random_arena([30, 20, 25], [0, 1, 1], [(24, 31), (17, 40)])
    t = {k: torch.from_numpy(np.ascontiguousarray(arena[k], dtype=np.float32)).to(DEV) for k in MR.IN_KEYS}
    inputs = matchpoint.MatchpointInputs.from_flat(t["rays_o"], t["rays_d"], t["z"], t["color"], t["uv"], t["cam_z"], arena["counts"],
                                                   arena["seg_view"], arena["sizes"])
    snap = matchpoint.pack(inputs)
    snap.write(str(tmp_path / "a" / "p.ply"))
    snap.write(str(tmp_path / "b" / "p.ply"), png="device")
    ta, tb = _tree(tmp_path / "a"), _tree(tmp_path / "b")
    assert sorted(ta) == sorted(tb)
    pngs = [r for r in ta if r.endswith(".png")]
    assert len(pngs) == 2
    for rel in ta:
        fa, fb = open(ta[rel], "rb").read(), open(tb[rel], "rb").read()
        if rel.endswith(".png"):
            assert np.array_equal(R.decode_with_pillow(fa), R.decode_with_pillow(fb))
        else:
            assert fa == fb

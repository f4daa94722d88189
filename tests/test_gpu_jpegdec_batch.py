"""The batched JPEG decoder on the GPU (scg_jpegdec_decode_batch through jpeg_decode.decode_batch, images.load_images and
images.install_batched), held for EQUALITY OF BYTES to Pillow's pixels, to the restatement of the rule (tests/jpegdec_refs.py), to
jpeg_decode.decode of each file alone and to the recorded pixels of tests/golden/ref_jpegdec.npz.  No tolerance exists in this file."""
import functools
import io
import os
import types

import numpy as np
import pytest
import torch

import jpegdec_refs as R
from scgaussian_amd import _lib_jpegdec, images, jpeg, jpeg_decode
from test_gpu_jpegdec import PLANTED, SIZES, host_reads

pytestmark = pytest.mark.gpu
DEV = "cuda"
S = R.SUBSEQ
HERE = os.path.dirname(os.path.abspath(__file__))
HAS_PILLOW_JPEG = R.pillow_has_jpeg()
needs_pillow_jpeg = pytest.mark.skipif(not HAS_PILLOW_JPEG, reason="Pillow without JPEG")
BAD_SYNC = _lib_jpegdec.JPEGDEC_BAD_SYNC


def clean_batch(files, **kw):
    """decode_batch on the device route for every member, or a failure: ONE upload, ONE host read of the 4 n status words."""
    with host_reads() as reads:
        got = jpeg_decode.decode_batch(files, DEV, **kw)
    last = dict(jpeg_decode.LAST)
    assert last["route"] == ["device"] * len(files) and last["status"] == [0] * len(files), last
    chunks = last["chunks"]
    assert last["uploads"] == chunks and last["host_reads"] == chunks and len(reads) == chunks, (last, reads)
    assert sum(nbytes for _how, nbytes in reads) == 16 * len(files) and all(how == "cpu" for how, _n in reads), reads
    return [g.cpu().numpy() for g in got], got


def alone(data):
    got = jpeg_decode.decode(data, DEV)
    assert jpeg_decode.LAST["route"] == "device", dict(jpeg_decode.LAST)
    return got.cpu().numpy()


@functools.lru_cache(maxsize=None)
def big():
    """The 160 x 160 quality-100 noise file: four workgroups, no restart marker."""
    data = R.pillow_file(R.image(160, 160, 3, "noise"), 100, "4:4:4")
    assert R.segment_bytes(data) > 3 * R.THREADS * S and b"\xff\xd0" not in data
    return data


@functools.lru_cache(maxsize=None)
def big_pixels():
    return R.pillow_pixels(big())


@functools.lru_cache(maxsize=None)
def small(k):
    """Files of one subsequence."""
    return R.pillow_file(R.image(8, 8, 3, "noise", seed=k), 90, ("4:4:4", "4:2:2", "4:2:0")[k % 3])


# ---- one mixed batch ---------------------------------------------------------------------------------------------------------------
@needs_pillow_jpeg
@pytest.mark.parametrize("quality", (20, 90, 100))
def test_one_mixed_batch(quality):
    files = []
    for (H, W) in SIZES:
        for sampling in R.SAMPLINGS:
            for restart_blocks in (0, 1):
                files.append(R.pillow_file(R.image(H, W, 3, "noise"), quality, sampling, restart_blocks))
        files.append(R.pillow_file(R.image(H, W, 1, "noise"), quality))
        files.append(R.pillow_file(R.image(H, W, 3, "ramp"), quality, "4:2:0", optimize=True))
    z = np.load(os.path.join(HERE, "golden", "ref_jpegdec.npz"))
    golden = {z[f"{name}_file"].tobytes(): z[f"{name}_pixels"] for name in z["names"]}
    files += [f for f in golden if f not in files]
    got, _t = clean_batch(files)
    in_golden = 0
    for i, (data, g) in enumerate(zip(files, got)):
        assert g.dtype == np.uint8 and np.array_equal(g, R.pillow_pixels(data)), (i, "differs from Pillow")
        assert np.array_equal(g, alone(data)), (i, "differs from decode() alone")
        if data in golden:
            assert np.array_equal(g, golden[data]), (i, "differs from the recorded pixels")
            in_golden += 1
    assert in_golden == len(golden) == 6


# ---- image borders in the entropy grid ---------------------------------------------------------------------------------------------
@needs_pillow_jpeg
def test_pixels_do_not_depend_on_position_or_neighbours():
    a, b, c = small(0), small(1), small(2)
    base = [big(), a, big(), b, big(), big(), c, big()]          # first, between two small ones, two side by side, last
    want = {big(): big_pixels(), a: R.pillow_pixels(a), b: R.pillow_pixels(b), c: R.pillow_pixels(c)}
    alone(big())
    need = jpeg_decode.LAST["rounds"]                            # the sync launches the file takes alone
    assert 1 < need <= 3
    for files in (base, base[::-1], base[3:] + base[:3], [a, big(), b], [a, b, c, big()]):
        got, _t = clean_batch(files)
        assert jpeg_decode.LAST["rounds"] == [need if f is big() else 1 for f in files], dict(jpeg_decode.LAST)
        for i, (data, g) in enumerate(zip(files, got)):
            assert np.array_equal(g, want[data]), (len(files), i)


# ---- the C entry -------------------------------------------------------------------------------------------------------------------
def run_staged(files, rounds=None, stream=None):
    """One scg_jpegdec_decode_batch on buffers of this call's own: (pixels per image, status (n, 4), the stage)."""
    infos = [jpeg_decode.parse(f) for f in files]
    assert all(i is not None for i in infos)
    stage = jpeg_decode.BatchStage(infos, files).plan()
    staged = torch.empty(stage.nbytes, dtype=torch.uint8, pin_memory=True)
    stage.fill(staged.numpy())
    with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):
        upload = staged.to(DEV, non_blocking=True)
        out = torch.empty(stage.out_bytes, dtype=torch.uint8, device=DEV)
        ws = torch.empty(stage.workspace_bytes, dtype=torch.uint8, device=DEV)
        jpeg_decode.launch_batch(stage, upload, out, ws, stage.max_rounds if rounds is None else rounds)
        status = ws[:16 * stage.n].view(torch.int32).cpu().numpy().astype(np.int64).reshape(stage.n, 4) & 0xFFFFFFFF
        host = out.cpu().numpy()
    pixels = []
    for i in range(stage.n):
        at, shape = int(stage.out_offsets[i]), stage.shape(i)
        pixels.append(host[at:at + int(np.prod(shape))].reshape(shape))
    return pixels, status, stage


@needs_pillow_jpeg
def test_rounds_through_the_c_entry():
    files = [small(0), big(), small(1), small(2)]
    info = jpeg_decode.parse(big())
    _out, single = jpeg_decode.decode_staged(info, jpeg_decode.stage(info, big()).to(DEV))
    need = int(single[1])
    assert int(single[0]) == 0 and 1 < need <= 3
    max_rounds = jpeg_decode.BatchStage([jpeg_decode.parse(f) for f in files], files).plan().max_rounds
    assert max_rounds == jpeg_decode.sizes(info.frame, info.segment_end - info.segment_start)[2] == 5
    for rounds in (1, 2, 3, max_rounds):
        pixels, status, _stage = run_staged(files, rounds)
        print(f"\nrounds = {rounds}: status {status.tolist()}")
        for i in (0, 2, 3):                                     # the others: right whatever the big one needs
            assert list(status[i][:2]) == [0, 1] and np.array_equal(pixels[i], R.pillow_pixels(files[i])), (rounds, i)
        if rounds < need:                                       # too few: the last launch still changed a state
            assert int(status[1][0]) & BAD_SYNC, (rounds, status[1])
        else:
            assert [int(v) for v in status[1][:3]] == [0, int(single[1]), int(single[2])], (rounds, status[1], single)
            assert np.array_equal(pixels[1], big_pixels()), rounds


def test_short_segments_in_one_batch():
    files = [R.segment_of_length(n) for n in (1, S - 1, S, S + 1, 2 * S + 1)]
    assert [R.segment_bytes(f) for f in files] == [1, S - 1, S, S + 1, 2 * S + 1]
    got, _t = clean_batch(files)
    for data, g in zip(files, got):
        assert np.array_equal(g, R.decode(data)), R.segment_bytes(data)


def test_every_planted_stream_in_one_batch():
    planted = R.planted()
    names = sorted(PLANTED)
    for name in names:
        assert all(planted[name][1][c] > 0 for c in PLANTED[name]), name
    files = [planted[name][0] for name in names]
    got, _t = clean_batch(files)
    for name, data, g in zip(names, files, got):
        assert np.array_equal(g, R.decode(data)), name


@needs_pillow_jpeg
def test_one_file_and_no_file():
    data = R.pillow_file(R.image(37, 53, 3, "noise"), 90, "4:2:0")
    got, _t = clean_batch([data])
    assert np.array_equal(got[0], alone(data)) and np.array_equal(got[0], R.pillow_pixels(data))
    assert jpeg_decode.decode_batch([], DEV) == []
    assert jpeg_decode.LAST["uploads"] == 0 and jpeg_decode.LAST["host_reads"] == 0 and jpeg_decode.LAST["chunks"] == 0


@needs_pillow_jpeg
def test_a_videos_frames_share_one_header_block(tmp_path):
    frames = [torch.from_numpy(R.image(37, 53, 3, kind, seed)).to(DEV) for kind, seed in (("noise", 1), ("ramp", 2), ("noise", 3))]
    files = jpeg.encode(frames, quality=90, subsampling="4:2:0").files()
    path = str(tmp_path / "v.avi")
    jpeg.write_avi(path, files, 24, 53, 37)
    back = jpeg.read_avi(path)
    got, _t = clean_batch(back)
    assert jpeg_decode.LAST["headers"] == 1
    for f, g in zip(back, got):
        assert np.array_equal(g, alone(f)) and np.array_equal(g, R.pillow_pixels(f))


# ---- bad members -------------------------------------------------------------------------------------------------------------------
def _says(fn, data):
    try:
        return fn(data), None
    except Exception as e:      # noqa: BLE001  (whatever is raised is the behaviour to match)
        return None, type(e)


@needs_pillow_jpeg
def test_bad_members_behave_as_decode_does_and_leave_the_others_alone(tmp_path):
    from PIL import Image
    good = R.pillow_file(R.image(37, 53, 3, "noise"), 90, "4:2:0")
    info = jpeg_decode.parse(good)
    truncated = good[:info.segment_start + (info.segment_end - info.segment_start) // 2]
    cut = truncated + b"\xff\xd9"
    garbage = good[:info.segment_end] + bytes(range(1, 200)) + good[info.segment_end:]
    flipped = None
    for at in range(info.segment_start + 8, info.segment_end - 8):
        bad = bytearray(good)
        bad[at] ^= 0x7E
        if bad[at] == 0xFF or bad[at - 1] == 0xFF or jpeg_decode.parse(bytes(bad)) is None:
            continue
        _p, status, _s = run_staged([bytes(bad)])
        if int(status[0][0]) & _lib_jpegdec.JPEGDEC_BAD_CODE:
            flipped = bytes(bad)
            break
    assert flipped is not None, "no flipped bit gave an invalid code"
    rgb = R.image(24, 40, 3, "noise")
    progressive = R.pillow_file(rgb, 90, "4:2:0", progressive=True)
    buf = io.BytesIO()
    Image.fromarray(rgb).save(buf, format="PNG")
    png = buf.getvalue()
    neighbours = [small(0), small(1), big(), small(2)]
    pillow = lambda d: np.array(Image.open(io.BytesIO(d)))                                   # noqa: E731
    for what, data, host in (("cut inside its segment", cut, False), ("garbage tail", garbage, False), ("flipped bit", flipped, False),
                             ("progressive", progressive, True), ("png", png, True), ("truncated", truncated, True)):
        want, want_error = _says(lambda d: jpeg_decode.decode(d, DEV).cpu().numpy(), data)
        assert (want is None) == (_says(pillow, data)[0] is None), what
        files = neighbours[:2] + [data] + neighbours[2:]
        got, got_error = _says(lambda fs: jpeg_decode.decode_batch(fs, DEV), files)
        assert got_error is want_error, (what, got_error, want_error)
        if got is None:
            continue
        last = dict(jpeg_decode.LAST)
        assert np.array_equal(got[2].cpu().numpy(), want), what
        assert last["route"][2] != "device" and (last["status"][2] is None) == host, (what, last)
        assert [last["status"][i] for i in (0, 1, 3, 4)] == [0] * 4 and [last["route"][i] for i in (0, 1, 3, 4)] == ["device"] * 4, (what, last)
        for i, f in zip((0, 1, 3, 4), neighbours):
            assert np.array_equal(got[i].cpu().numpy(), R.pillow_pixels(f)), (what, i)
    # the first failing source in order raises
    with pytest.raises(_says(pillow, truncated)[1]):
        jpeg_decode.decode_batch([small(0), truncated, b"not an image at all"], DEV)


# ---- cost, chunks, stacking --------------------------------------------------------------------------------------------------------
@needs_pillow_jpeg
def test_two_chunks_give_the_same_pixels_with_two_uploads_and_reads():
    files = [small(0), big(), small(1), small(2), big(), small(3)]
    one, _t = clean_batch(files)
    assert jpeg_decode.LAST["chunks"] == 1 and jpeg_decode.LAST["uploads"] == 1 and jpeg_decode.LAST["host_reads"] == 1
    whole = jpeg_decode.BatchStage([jpeg_decode.parse(f) for f in files], files).plan().workspace_bytes
    first = jpeg_decode.BatchStage([jpeg_decode.parse(f) for f in files[:3]], files[:3]).plan().workspace_bytes
    assert first < whole - 1
    two, _t = clean_batch(files, max_workspace_bytes=whole - 1)
    assert jpeg_decode.LAST["chunks"] == 2 and jpeg_decode.LAST["uploads"] == 2 and jpeg_decode.LAST["host_reads"] == 2
    for a, b in zip(one, two):
        assert np.array_equal(a, b)


@needs_pillow_jpeg
def test_equal_shapes_of_a_chunk_are_views_of_one_tensor_at_a_constant_stride():
    files = [R.pillow_file(R.image(16, 24, 3, "noise", seed=k), 90, "4:2:0") for k in range(4)]
    odd = R.pillow_file(R.image(7, 9, 3, "noise"), 90, "4:4:4")                          # 189 bytes: padded to the next 16
    host, got = clean_batch(files[:2] + [odd] + files[2:] + [odd, odd])
    storage = got[0].untyped_storage().data_ptr()
    assert all(g.untyped_storage().data_ptr() == storage and g.is_contiguous() for g in got)
    offsets = [g.storage_offset() for g in got]
    assert offsets == sorted(offsets) and all(o % 16 == 0 for o in offsets)              # input order, 16-byte aligned
    nbytes = 16 * 24 * 3
    assert offsets[1] - offsets[0] == offsets[4] - offsets[3] == nbytes                  # neighbours of one shape: tight
    assert offsets[6] - offsets[5] == 192
    host, got = clean_batch(files)
    offsets = [g.storage_offset() for g in got]
    assert [b - a for a, b in zip(offsets, offsets[1:])] == [nbytes] * 3
    stacked = torch.as_strided(got[0], (4, 16, 24, 3), (nbytes, 72, 3, 1), offsets[0])   # ONE contiguous (k, H, W, 3) tensor
    assert stacked.is_contiguous() and np.array_equal(stacked.cpu().numpy(), np.stack(host))


@needs_pillow_jpeg
def test_two_runs_a_fresh_plan_and_a_side_stream_give_the_same_bytes():
    files = [small(0), big(), R.pillow_file(R.image(37, 53, 1, "noise"), 90), small(1)]
    first, _t = clean_batch(files)
    again, _t = clean_batch(files)                                                       # the buffers the first call left
    jpeg_decode._BATCH_BUFFERS.clear()
    fresh, _t = clean_batch(files)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        streamed = [g.cpu().numpy() for g in jpeg_decode.decode_batch(files, DEV)]
    side.synchronize()
    own, status, _s = run_staged(files, stream=side)
    assert not status[:, 0].any()
    for runs in zip(first, again, fresh, streamed, own):
        assert all(np.array_equal(runs[0], r) for r in runs[1:])


# ---- images ------------------------------------------------------------------------------------------------------------------------
def _bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.uint32)


def _piltotorch(pil_image, resolution):
    """What PILtoTorch computes (utils/general_utils.py:22-28): Pillow's resize, / 255.0, channels first."""
    t = torch.from_numpy(np.array(pil_image.resize(resolution))) / 255.0
    return t.permute(2, 0, 1) if t.dim() == 3 else t.unsqueeze(dim=-1).permute(2, 0, 1)


@pytest.fixture(scope="module")
def scene(tmp_path_factory):
    """Paths and target sizes: unequal sources and targets, two groups of equal ones, the 378 x 504 -> 47 x 63 photograph, a
    reduction beyond ksize 129, a grey file, a progressive file and a PNG."""
    from PIL import Image
    folder = tmp_path_factory.mktemp("scene")
    rng = np.random.default_rng(4)
    photo = np.clip(R.image(378, 504, 3, "ramp").astype(np.int64) + rng.integers(-24, 25, size=(378, 504, 3)), 0, 255).astype(np.uint8)
    items = []

    def add(name, img, res, **kw):
        path = str(folder / name)
        Image.fromarray(img).save(path, **kw)
        items.append((path, res))

    add("photo.jpg", photo, (63, 47), quality=90)
    for k in range(3):
        add(f"a{k}.jpg", R.image(48, 64, 3, "noise", seed=k), (16, 12), quality=90)          # 9216 bytes each: side by side
    for k in range(2):
        add(f"b{k}.jpg", R.image(37, 53, 3, "ramp", seed=k), (7, 5), quality=95, subsampling="4:4:4")      # padded: gathered
    add("grey.jpg", R.image(40, 56, 1, "noise"), (14, 10), quality=90)
    add("a_other_target.jpg", R.image(48, 64, 3, "noise", seed=9), (8, 6), quality=90)
    add("far.jpg", R.image(2, 160, 3, "ramp"), (2, 2), quality=90)                            # 80x: ksize 323, Pillow resizes
    add("progressive.jpg", R.image(24, 40, 3, "noise"), (10, 6), quality=90, progressive=True)
    add("picture.png", R.image(24, 40, 3, "noise"), (10, 6))
    return items


@needs_pillow_jpeg
def test_load_images_equals_load_image_bit_for_bit(scene):
    from PIL import Image
    paths, targets = [p for p, _r in scene], [r for _p, r in scene]
    assert not images.plan_of((160, 2), (2, 2), 3).device_route and images.ksize_of(160, 2) > 129
    want = [images.load_image(p, r, DEV) for p, r in scene]
    with host_reads() as reads:
        got = images.load_images(paths, targets, DEV)
    last = dict(jpeg_decode.LAST)
    assert len(got) == len(want)
    for (path, res), g, w in zip(scene, got, want):
        assert g.dtype == torch.float32 and g.shape == w.shape and np.array_equal(_bits(g), _bits(w)), path
        assert np.array_equal(_bits(g), _bits(_piltotorch(Image.open(path), res))), path
    # photo, a0..a2, b0, b1, grey, a_other_target in ONE batch; progressive went through decode() behind it
    assert last["chunks"] == 1 and last["route"][:8] == ["device"] * 8 and last["route"][8] == "single host", last
    assert last["status"][8] is None and [r for r in reads if r[0] == "cpu"] == [("cpu", 16 * 8)], reads      # (parse refused the ninth)
    # one resolution for every path
    same = images.load_images(paths[1:4], (16, 12), DEV)
    for g, w in zip(same, want[1:4]):
        assert np.array_equal(_bits(g), _bits(w))
    assert images.load_images([], [], DEV) == []
    # the recorded PILtoTorch tensor of the reference for the golden 4:2:0 file
    z = np.load(os.path.join(HERE, "golden", "ref_jpegdec.npz"))
    path = os.path.join(os.path.dirname(paths[0]), "golden_420.jpg")
    with open(path, "wb") as fh:
        fh.write(z["rgb_420_file"].tobytes())
    res = tuple(int(v) for v in z["piltotorch_res"])
    got = images.load_images([path, path], [res, res], DEV)
    assert all(np.array_equal(_bits(g), z["piltotorch_out"].view(np.uint32)) for g in got)


def _stand_in():
    """A module with a loadCam / cameraList_from_camInfos pair shaped like utils/camera_utils.py."""
    m = types.ModuleType("camera_utils_stand_in")
    m.PILtoTorch = _piltotorch

    def loadCam(args, id, cam_info, resolution_scale):
        orig_w, orig_h = cam_info.image.size
        if args.resolution in [1, 2, 4, 8]:
            resolution = round(orig_w / (resolution_scale * args.resolution)), round(orig_h / (resolution_scale * args.resolution))
        else:
            global_down = (orig_w / 1600 if orig_w > 1600 else 1) if args.resolution == -1 else orig_w / args.resolution
            scale = float(global_down) * float(resolution_scale)
            resolution = (int(orig_w / scale), int(orig_h / scale))
        resized = m.PILtoTorch(cam_info.image, resolution)
        return types.SimpleNamespace(uid=id, image=resized[:3, ...], image_name=cam_info.image_name)

    def cameraList_from_camInfos(cam_infos, resolution_scale, args):
        return [m.loadCam(args, id, c, resolution_scale) for id, c in enumerate(cam_infos)]

    m.loadCam, m.cameraList_from_camInfos = loadCam, cameraList_from_camInfos
    return m


@needs_pillow_jpeg
def test_install_batched_loads_a_scene_with_one_upload_and_one_read(scene):
    from PIL import Image
    paths = [p for p, _r in scene if "far" not in p and "progressive" not in p]           # JPEG cameras and one PNG camera
    infos = lambda: [types.SimpleNamespace(image=Image.open(p), image_name=os.path.basename(p)) for p in paths]      # noqa: E731
    module = _stand_in()
    original = module.cameraList_from_camInfos
    served = []
    real = images.pil_to_torch

    def counted(pil_image, resolution, *a, **k):
        served.append(getattr(pil_image, "format", None))
        return real(pil_image, resolution, *a, **k)

    for resolution, scale in ((2, 1.0), (20, 0.5)):             # halves; 40 columns (the photograph: 12.6x, within the kernels)
        args = types.SimpleNamespace(resolution=resolution)
        images.install(module, decode="device")
        want = module.cameraList_from_camInfos(infos(), scale, args)
        module.PILtoTorch = _piltotorch
        previous = images.install_batched(module)
        assert previous is original and module.cameraList_from_camInfos is not original
        images.pil_to_torch = counted
        try:
            with host_reads() as reads:
                got = module.cameraList_from_camInfos(infos(), scale, args)
        finally:
            images.pil_to_torch = real
        last = dict(jpeg_decode.LAST)
        assert module.PILtoTorch is _piltotorch                                           # bound only while the loop ran
        assert [c.image_name for c in got] == [c.image_name for c in want]
        for g, w in zip(got, want):
            assert g.image.shape == w.image.shape and np.array_equal(_bits(g.image), _bits(w.image)), g.image_name
        n = len(paths) - 1
        assert last["uploads"] == 1 and last["host_reads"] == 1 and last["route"] == ["device"] * n, last
        assert [r for r in reads if r[0] == "cpu"] == [("cpu", 16 * n)], reads
        assert served == ["PNG"], served                                                  # the non-JPEG camera alone
        served.clear()
        module.cameraList_from_camInfos = previous                                        # restored by assigning it back
        assert module.cameraList_from_camInfos is original

"""The batched JPEG decoder without a GPU: scg_jpegdec_batch_plan's records, regions and prefix tables against scg_jpegdec_sizes and
the header's layout, every argument code of both new entries without a launch, and the staging layout of jpeg_decode.BatchStage."""
import ctypes as C

import numpy as np
import pytest

import jpegdec_refs as R
from scgaussian_amd import _lib, _lib_jpegdec, jpeg_decode

W = _lib_jpegdec.JPEGDEC_IMAGE_WORDS
T, S = _lib_jpegdec.JPEGDEC_THREADS, _lib_jpegdec.JPEGDEC_SUBSEQ
P64, P32, PI32 = C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.POINTER(C.c_int32)


def _frame(H=16, W_=16, comps=3, h=2, v=2, ri=0, last=0):
    t = (0, 1, 1) if comps == 3 else (0, 0, 0)
    return [H, W_, comps, h, v, ri, *t, *t, *t, last]


# (frame, segment bytes): one and three components, every sampling, one and several workgroups, a restart interval
MIXED = [(_frame(16, 16), 1000), (_frame(37, 53, 3, 2, 1), 128 * 256 + 1), (_frame(9, 9, 1, 1, 1), 1), (_frame(160, 160, 3, 1, 1), 4 * 128 * 256),
         (_frame(1, 1, 3, 1, 1, ri=2), 129), (_frame(16, 16), 1000)]


class Plan:
    def __init__(self, items, header_at=None, segment_at=None, upload_bytes=None, n=None, table_words=None):
        self.n = len(items) if n is None else n
        m = len(items)
        self.frames = np.array([f for f, _s in items], dtype=np.int32).reshape(m, 16)
        self.seg = np.array([s for _f, s in items], dtype=np.uint64)
        # one header block shared by all (a shared offset is accepted), the segments behind it at 16-byte offsets
        self.hdr = np.array([4096] * m if header_at is None else header_at, dtype=np.uint64)
        at, seg_at = 8192, []
        for _f, s in items:
            seg_at.append(at)
            at = (at + s + 15) // 16 * 16
        self.sat = np.array(seg_at if segment_at is None else segment_at, dtype=np.uint64)
        self.upload_bytes = at if upload_bytes is None else upload_bytes
        words = jpeg_decode.table_words(m)
        self.table = np.zeros(words, dtype=np.uint32)
        self.table_words = words if table_words is None else table_words
        self.out_at = np.zeros(m, dtype=np.uint64)
        self.ws, self.ob, self.mr = C.c_uint64(), C.c_uint64(), C.c_int32()

    def call(self, **null):
        lib = _lib_jpegdec.load()
        a = dict(frames=self.frames.ctypes.data_as(PI32), seg=self.seg.ctypes.data_as(P64), hdr=self.hdr.ctypes.data_as(P64),
                 sat=self.sat.ctypes.data_as(P64), table=self.table.ctypes.data_as(P32), out_at=self.out_at.ctypes.data_as(P64),
                 ws=C.byref(self.ws), ob=C.byref(self.ob), mr=C.byref(self.mr))
        a.update(null)
        return lib.scg_jpegdec_batch_plan(self.n, a["frames"], a["seg"], a["hdr"], a["sat"], self.upload_bytes, a["table"], self.table_words,
                                          a["out_at"], a["ws"], a["ob"], a["mr"])

    def record(self, i):
        return self.table[i * W:(i + 1) * W]

    def word64(self, i, at):
        r = self.record(i)
        return int(r[at]) | (int(r[at + 1]) << 32)


def _groups(frame, seg):
    H, W_, comps, h, v = frame[:5]
    mcus = -(-W_ // (8 * h)) * -(-H // (8 * v))
    nblocks = mcus * (h * v + (2 if comps == 3 else 0))
    nsub = -(-seg // S)
    return -(-nsub // T), -(-nblocks // (T // 8)), -(-(W_ * comps) // (4 * T)) * H, nsub, nblocks, mcus


def test_batch_plan_of_a_mixed_list():
    p = Plan(MIXED)
    assert p.call() == 0, _lib_jpegdec.load().scg_jpegdec_last_error()
    n = len(MIXED)
    regions, rounds, out_end, single_ws = [], [], 0, 0
    most = max(jpeg_decode.sizes(np.array(f, dtype=np.int32), s)[2] for f, s in MIXED)
    for i, (frame, seg) in enumerate(MIXED):
        ws, ob, mr = jpeg_decode.sizes(np.array(frame, dtype=np.int32), seg)
        rounds.append(mr)
        single_ws += ws
        r = p.record(i)
        assert list(r[:16].astype(np.int32)) == frame and int(r[16]) == seg and int(r[17]) == 0 and not r[44:].any()
        assert p.word64(i, 18) == 4096 and p.word64(i, 20) == int(p.sat[i])
        out_at = p.word64(i, 22)
        assert out_at == int(p.out_at[i]) and out_at % 16 == 0 and out_at >= out_end          # input order, aligned, disjoint
        out_end = out_at + ob
        assert ob == frame[0] * frame[1] * frame[2]
        nwg, _ig, _cg, nsub, nblocks, mcus = _groups(frame, seg)
        h, v = frame[3], frame[4]
        chroma = 64 * mcus if frame[2] == 3 else 0
        need = [4 * most, 8 * nsub, 8 * nsub, 16 * nwg, 4 * nsub, 16 * nsub, 128 * nblocks, 64 * mcus * h * v, chroma, chroma]
        where = [p.word64(i, 24 + 2 * k) for k in range(10)]
        if frame[2] == 1:
            assert where[8] == where[9] == where[7]
        for k, (at, nb) in enumerate(zip(where, need)):
            assert at % 16 == 0, (i, k)
            if nb:
                regions.append((at, at + nb, (i, k)))
    assert p.mr.value == max(rounds) == most == 5                                                     # four workgroups + 1
    assert p.ob.value >= out_end and p.ob.value - out_end < 16
    # every region inside the total, behind the status words, and disjoint from every other
    regions.append((0, 16 * n, "status"))
    regions.sort()
    for (a0, a1, what), (b0, _b1, what_b) in zip(regions, regions[1:]):
        assert a1 <= b0, (what, what_b)
    assert regions[-1][1] <= p.ws.value
    # the change counters lie side by side behind the status words, the coefficient buffers side by side at the end (one clear each)
    ctl = sorted(r for r in regions if r[2] != "status" and r[2][1] == 0)
    assert ctl[0][0] == 16 * n and all(b[0] - a[1] < 16 for a, b in zip(ctl, ctl[1:]))
    coef = sorted(r for r in regions if r[2] != "status" and r[2][1] == 6)
    assert coef[-1][1] <= p.ws.value and all(r[1] <= coef[0][0] for r in regions if r not in coef)
    assert p.ws.value < single_ws + 4096 * n
    # the prefix tables: monotone, first entry 0, last entry the grid
    for k in range(3):
        pre = p.table[n * W + k * (n + 1):n * W + (k + 1) * (n + 1)].astype(np.int64)
        assert pre[0] == 0 and list(np.diff(pre)) == [_groups(f, s)[k] for f, s in MIXED], k


def test_every_argument_code_of_the_plan():
    err = _lib_jpegdec.load().scg_jpegdec_last_error
    assert Plan(MIXED).call() == 0
    for name in ("frames", "seg", "hdr", "sat", "table", "out_at", "ws", "ob", "mr"):
        assert Plan(MIXED).call(**{name: None}) == -1, name
    assert Plan(MIXED, n=0).call() == -2 and Plan(MIXED, n=-1).call() == -2 and b"images" in err()
    assert Plan(MIXED, n=_lib_jpegdec.JPEGDEC_MAX_BATCH + 1).call() == -2
    bad = list(MIXED)
    bad[2] = (_frame(9, 9, 2, 1, 1), 1)
    assert Plan(bad).call() == -2 and b"image 2" in err() and b"components" in err()
    bad[2] = (_frame(9, 9, 1, 1, 1), 0)
    assert Plan(bad).call() == -2 and b"image 2" in err() and b"segment" in err()
    good = Plan(MIXED)
    hdr = [4096] * len(MIXED)
    assert Plan(MIXED, header_at=hdr[:3] + [4104] + hdr[4:]).call() == -5 and b"image 3" in err()
    assert Plan(MIXED, header_at=hdr[:3] + [good.upload_bytes - 4080] + hdr[4:]).call() == -2 and b"header block" in err()
    sat = [int(v) for v in good.sat]
    assert Plan(MIXED, segment_at=sat[:1] + [sat[1] + 4] + sat[2:]).call() == -5
    assert Plan(MIXED, upload_bytes=good.upload_bytes - 16).call() == -2 and b"segment" in err()          # the last segment leaves the upload
    assert Plan(MIXED, table_words=good.table_words - 1).call() == -4 and b"table" in err()


def test_every_argument_code_of_decode_batch_without_a_launch():
    lib = _lib_jpegdec.load()
    err = lib.scg_jpegdec_last_error
    p = Plan(MIXED)
    assert p.call() == 0
    fake = 0x10000

    def call(n=p.n, frames=p.frames, table=p.table, table_dev=fake, upload=fake, upload_bytes=p.upload_bytes, out=fake, nout=None, work=fake,
             nwork=None, rounds=1):
        return lib.scg_jpegdec_decode_batch(n, None if frames is None else frames.ctypes.data_as(PI32),
                                            None if table is None else table.ctypes.data_as(P32), table_dev, upload, upload_bytes, out,
                                            p.ob.value if nout is None else nout, work, p.ws.value if nwork is None else nwork, rounds, None)

    assert call(frames=None) == -1 and call(table=None) == -1
    assert call(n=0) == -2 and call(n=-3) == -2 and call(n=_lib_jpegdec.JPEGDEC_MAX_BATCH + 1) == -2
    frames = p.frames.copy()
    frames[2, 2] = 2                                                                          # a bad frame among good ones
    assert call(frames=frames) == -2 and b"image 2" in err()
    frames = p.frames.copy()
    frames[1, 0] += 1                                                                         # a good frame that is not the table's
    assert call(frames=frames) == -2 and b"batch_plan" in err()

    def patched(word, value, image=3):
        t = p.table.copy()
        t[image * W + word] = value
        return t

    assert call(table=patched(18, 4104)) == -5                                                # header offset unaligned
    assert call(table=patched(18, p.upload_bytes)) == -2 and b"header block" in err()
    assert call(table=patched(20, int(p.sat[3]) + 8)) == -5
    assert call(upload_bytes=p.upload_bytes - 16) == -2 and b"segment" in err()               # a segment leaves the upload
    # a host table that disagrees with the plan: an output offset, a workspace region, a reserved word, a prefix entry
    for word in (22, 24, 36, 38, 17, 47):
        assert call(table=patched(word, int(p.table[3 * W + word]) + 16)) == -2 and b"batch_plan" in err(), word
    for at in (p.n * W + 1, p.n * W + p.n, p.n * W + 2 * (p.n + 1) + p.n):
        t = p.table.copy()
        t[at] += 1
        assert call(table=t) == -2 and b"batch_plan" in err(), at
    assert call(table_dev=None) == -1 and b"table_dev is NULL" in err() and call(table_dev=fake + 8) == -5
    assert call(upload=None) == -1 and call(upload=fake + 4) == -5
    assert call(out=None) == -1 and call(out=fake + 4) == -5
    assert call(nout=p.ob.value - 1) == -4 and b"out of" in err()
    assert call(work=None) == -1 and call(work=fake + 8) == -5
    assert call(nwork=p.ws.value - 1) == -4 and b"workspace of" in err()
    assert call(rounds=0) == -2 and call(rounds=p.mr.value + 1) == -2 and b"rounds" in err()


def test_decode_batch_refuses_without_a_gpu():
    with pytest.raises(_lib.ScgError, match="ROCm GPU"):
        jpeg_decode.decode_batch([b"\xff\xd8\xff\xd9"], device="cpu")
    with pytest.raises(_lib.ScgError, match="ROCm GPU"):
        jpeg_decode.decode_batch([], device="cpu")


def test_the_staging_layout():
    rng = np.random.default_rng(5)
    own = dict(R.STD_TABLES)
    bits, vals = R.AC_LUMA
    own[(1, 0)] = (bits, list(vals[:40]) + list(vals[40:][::-1]))                             # another table: another header block
    files = [R.segment_of_length(1), R.segment_of_length(129), R.segment_of_length(257),
             R.write_file(8, 64, R.random_blocks(rng, 8), tables=own), R.segment_of_length(127)]
    infos = [jpeg_decode.parse(f) for f in files]
    assert all(i is not None for i in infos)
    stage = jpeg_decode.BatchStage(infos, files).plan()
    n = len(files)
    assert stage.table_bytes == -(-4 * (n * W + 3 * (n + 1)) // 16) * 16
    assert len(stage.headers) == 2 and len(set(stage.header_offsets)) == 2                     # de-duplicated by content
    assert sorted(set(stage.header_offsets)) == [stage.table_bytes, stage.table_bytes + 4096]
    view = np.full(stage.nbytes, 0xAA, dtype=np.uint8)
    stage.fill(view)
    assert np.array_equal(view[:4 * stage.table.size].view(np.uint32), stage.table)            # tables first
    end = stage.table_bytes + 4096 * 2
    for i, (info, data) in enumerate(zip(infos, files)):
        at, nb = stage.segment_offsets[i], stage.segment_bytes[i]
        assert at % 16 == 0 and at >= end
        end = at + nb
        assert view[at:at + nb].tobytes() == data[info.segment_start:info.segment_end]
        h = stage.header_offsets[i]
        assert np.array_equal(view[h:h + 4096], jpeg_decode.header_block(info))
        rec = stage.table[i * W:(i + 1) * W]
        assert int(rec[16]) == nb and int(rec[18]) == h and int(rec[20]) == at
    assert stage.nbytes == -(-end // 16) * 16
    # nothing of a file but its segment is staged: the staged bytes are fewer than the files'
    assert stage.nbytes - stage.table_bytes - 8192 < sum(len(f) for f in files)

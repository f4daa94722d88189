"""JPEG files decoded on the GPU, host side (libscg_jpegdec.so; include/jpegdec/scg_jpegdec.h states the rule and the call).

    u8 = jpeg_decode.decode(path_or_bytes)        device uint8 (H, W, 3) or (H, W) == np.asarray(Image.open(path)), ONE host read
    info = jpeg_decode.parse(data)                host only: the frame, the tables, the bounds of the entropy-coded segment, or None
    plan = jpeg_decode.plan_of(info.frame, dev)   the workspace of one frame shape, kept between calls
    u8s = jpeg_decode.decode_batch(sources)       [decode(s) for s in sources] with ONE upload, ONE launch chain and ONE host read

The reference opens every camera image with Image.open (scene/dataset_readers.py) and loadCam packs and resizes it on one host
core; here the file's bytes (about a tenth of the pixels) are uploaded and the pixels appear where images.resize_u8 reads them.
The header block (quantisation and Huffman tables) and the file are staged in ONE pinned buffer and uploaded with one copy; the
launches follow; the status word is the call's one host read.  What parse refuses — progressive, arithmetic, 12-bit, CMYK / Adobe
transforms, other samplings, several scans, 16-bit DQT — and any file whose status is not 0 (truncated, damaged) goes to
np.asarray(Image.open(...)) and one upload: such a file raises or returns exactly what Pillow does, and both routes give the same
tensor.  A missing library raises: there is no CPU stand-in for a kernel.
"""
from __future__ import annotations

import ctypes as C
import io
import os
from collections import namedtuple
from typing import Dict, Optional, Tuple

import numpy as np
import torch

from . import _lib, _lib_jpegdec
from ._lib_jpegdec import check

SUBSEQ = _lib_jpegdec.JPEGDEC_SUBSEQ
HEADER_BYTES = _lib_jpegdec.JPEGDEC_HEADER_BYTES
FIRST_ROUNDS = 3            # sync launches enqueued at once: guess, hand over, see that nothing changed
MORE_ROUNDS = 4             # ... and per further batch
ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35,
                   42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62,
                   63], dtype=np.int64)

# frame: the SCG_JPEGDEC_FRAME_WORDS int32 of the C call; quant: {id: uint16[64], natural order}; huffman: {(class, id): (bits[16],
# vals)}; the entropy-coded segment is data[segment_start:segment_end]
JpegInfo = namedtuple("JpegInfo", "H W components h v restart_interval frame quant huffman segment_start segment_end")

# what the last decode() did: route "device" / "host", the status words, the sync launches run, host reads made
LAST: Dict[str, object] = {}


def _err(msg: str) -> _lib.ScgError:
    return _lib.ScgError("jpeg_decode: " + msg)


def _u16(data, at: int) -> int:
    return (data[at] << 8) | data[at + 1]


def huffman_table(bits, vals) -> Optional[np.ndarray]:
    """The 896 bytes of one table of the header block (scg_jpegdec.h), or None for counts that are no prefix code with the
    all-ones code word left over."""
    bits = [int(b) for b in bits]
    vals = [int(v) for v in vals]
    if len(bits) != 16 or len(vals) != sum(bits) or len(vals) > 256:
        return None
    look = np.zeros(256, dtype=np.uint16)
    maxcode = np.full(16, -1, dtype=np.int32)
    valoff = np.zeros(16, dtype=np.int32)
    code = k = 0
    for ln in range(1, 17):
        n = bits[ln - 1]
        if n and code + n > (1 << ln) - 1:          # the codes of this length must leave all ones free
            return None
        if n:
            valoff[ln - 1] = k - code
            maxcode[ln - 1] = code + n - 1
            if ln <= 8:
                for j in range(n):
                    first = (code + j) << (8 - ln)
                    look[first:first + (1 << (8 - ln))] = (ln << 8) | vals[k + j]
        code = (code + n) << 1
        k += n
    out = np.zeros(896, dtype=np.uint8)
    out[:512] = look.view(np.uint8)
    out[512:576] = maxcode.view(np.uint8)
    out[576:640] = valoff.view(np.uint8)
    out[640:640 + len(vals)] = vals
    return out


def parse(data) -> Optional[JpegInfo]:
    """Walk the markers of a JPEG file (bytes-like).  None for anything the kernels do not take (scg_jpegdec.h WHAT IS ACCEPTED)
    and for a file whose entropy-coded segment has no end."""
    data = bytes(data)
    n = len(data)
    if n < 4 or data[0] != 0xFF or data[1] != 0xD8:
        return None
    at = 2
    quant: Dict[int, np.ndarray] = {}
    huffman: Dict[Tuple[int, int], Tuple[list, list]] = {}
    frame = None
    ri = 0
    jfif = False
    while True:
        if at + 4 > n or data[at] != 0xFF:
            return None
        while at < n and data[at] == 0xFF:          # fill bytes
            at += 1
        if at >= n:
            return None
        marker = data[at]
        at += 1
        if marker == 0xD8 or marker == 0x01 or 0xD0 <= marker <= 0xD7:
            continue
        if marker == 0xD9 or at + 2 > n:
            return None
        length = _u16(data, at)
        if length < 2 or at + length > n:
            return None
        body = data[at + 2:at + length]
        if marker == 0xC0:
            if frame is not None or len(body) < 6 or body[0] != 8:
                return None
            H, W, nf = _u16(body, 1), _u16(body, 3), body[5]
            if nf not in (1, 3) or len(body) != 6 + 3 * nf or H < 1 or W < 1:
                return None
            frame = (H, W, [(body[6 + 3 * i], body[7 + 3 * i] >> 4, body[7 + 3 * i] & 15, body[8 + 3 * i]) for i in range(nf)])
        elif 0xC1 <= marker <= 0xCF and marker not in (0xC4, 0xC8):
            return None                             # extended, progressive, lossless, arithmetic (and DAC)
        elif marker == 0xC4:
            p = 0
            while p < len(body):
                if p + 17 > len(body):
                    return None
                tc, th = body[p] >> 4, body[p] & 15
                bits = list(body[p + 1:p + 17])
                cnt = sum(bits)
                if tc > 1 or th > 1 or p + 17 + cnt > len(body):
                    return None
                huffman[(tc, th)] = (bits, list(body[p + 17:p + 17 + cnt]))
                p += 17 + cnt
        elif marker == 0xDB:
            p = 0
            while p < len(body):
                pq, tq = body[p] >> 4, body[p] & 15
                if pq != 0 or tq > 3 or p + 65 > len(body):
                    return None
                table = np.zeros(64, dtype=np.uint16)
                table[ZIGZAG] = np.frombuffer(body[p + 1:p + 65], dtype=np.uint8)
                quant[tq] = table
                p += 65
        elif marker == 0xDD:
            if len(body) != 2:
                return None
            ri = _u16(body, 0)
        elif marker == 0xE0:
            jfif = jfif or body[:5] == b"JFIF\0"
        elif marker == 0xEE and body[:5] == b"Adobe":
            return None                             # a colour transform flag: Pillow's business
        elif marker == 0xDA:
            break
        at += length
    if frame is None:
        return None
    H, W, comps = frame
    nf = len(comps)
    if len(body) != 4 + 2 * nf or body[0] != nf or tuple(body[1 + 2 * nf:]) != (0, 63, 0):
        return None                                 # not every component, or a spectral / successive-approximation scan
    td, ta = [0, 0, 0], [0, 0, 0]
    for i, (cid, _h, _v, _tq) in enumerate(comps):
        if body[1 + 2 * i] != cid:
            return None
        td[i], ta[i] = body[2 + 2 * i] >> 4, body[2 + 2 * i] & 15
        if (0, td[i]) not in huffman or (1, ta[i]) not in huffman or comps[i][3] not in quant:
            return None
    h, v = comps[0][1], comps[0][2]
    if nf == 1:
        h = v = 1                                   # one component: its factors only scale the MCU, which is one block
    else:
        if (h, v) not in ((1, 1), (2, 1), (2, 2)) or any((c[1], c[2]) != (1, 1) for c in comps[1:]):
            return None
        if not jfif and tuple(c[0] for c in comps) != (1, 2, 3):
            return None                             # without JFIF libjpeg guesses the colour space from the ids
    for key in set([(0, t) for t in td[:nf]] + [(1, t) for t in ta[:nf]]):
        if huffman_table(*huffman[key]) is None:
            return None
    start = at + length
    # the segment ends at the first FF that is followed by neither 00 nor RSTn
    arr = np.frombuffer(data, dtype=np.uint8, offset=start)
    ff = np.flatnonzero(arr[:-1] == 0xFF) if arr.size > 1 else np.zeros(0, dtype=np.int64)
    nxt = arr[ff + 1]
    ends = ff[(nxt != 0) & ((nxt & 0xF8) != 0xD0)]
    if ends.size == 0 or ends[0] == 0:
        return None                                 # no end (a truncated file), or no entropy-coded byte at all
    end = start + int(ends[0])
    if data[end + 1] != 0xD9:
        return None                                 # another scan, DNL, ...
    if end - start > _lib_jpegdec.JPEGDEC_MAX_SEGMENT or max(H, W) > _lib_jpegdec.JPEGDEC_MAX_DIM:
        return None
    tq = [c[3] for c in comps] + [0] * (3 - nf)
    words = np.array([H, W, nf, h, v, ri] + tq + td + ta + [0], dtype=np.int32)
    words.setflags(write=False)
    return JpegInfo(H, W, nf, h, v, ri, words, quant, huffman, start, end)


def header_block(info: JpegInfo) -> np.ndarray:
    """The SCG_JPEGDEC_HEADER_BYTES of the device header block: quant[4][64] uint16, then the tables DC 0, DC 1, AC 0, AC 1."""
    out = np.zeros(HEADER_BYTES, dtype=np.uint8)
    for tq, table in info.quant.items():
        out[128 * tq:128 * tq + 128] = table.astype("<u2").view(np.uint8)
    for (tc, th), (bits, vals) in info.huffman.items():
        table = huffman_table(bits, vals)
        if table is not None:
            off = 512 + 896 * (2 * tc + th)
            out[off:off + 896] = table
    return out


def sizes(frame: np.ndarray, segment_bytes: int) -> Tuple[int, int, int]:
    """(workspace bytes, output bytes, sync launches that settle every stream) of scg_jpegdec_sizes; host only."""
    ws, ob, mr = C.c_uint64(), C.c_uint64(), C.c_int32()
    words = np.ascontiguousarray(frame, dtype=np.int32)
    check(_lib_jpegdec.load().scg_jpegdec_sizes(words.ctypes.data_as(C.POINTER(C.c_int32)), int(segment_bytes), C.byref(ws), C.byref(ob),
                                                C.byref(mr)), "scg_jpegdec_sizes")
    return int(ws.value), int(ob.value), int(mr.value)


class JpegDecodePlan:
    """The workspace of one frame shape on one device, like images.ResizePlan the tables: allocated for the largest segment seen
    (with a quarter to spare) and reused, so a scene's images of one size share it."""

    def __init__(self, frame: np.ndarray, device):
        self.frame = np.ascontiguousarray(frame, dtype=np.int32)
        if self.frame.shape != (_lib_jpegdec.JPEGDEC_FRAME_WORDS,):
            raise _err(f"a frame is {_lib_jpegdec.JPEGDEC_FRAME_WORDS} int32, not {self.frame.shape}")
        self.device = torch.device(device)
        self.shape = (int(frame[0]), int(frame[1])) + ((3,) if int(frame[2]) == 3 else ())
        self._workspace: Optional[torch.Tensor] = None
        self._for_bytes = 0
        self._staging: Optional[torch.Tensor] = None

    def staging(self, nbytes: int) -> torch.Tensor:
        """nbytes of the plan's pinned staging buffer (grown with a quarter to spare, then reused: a scene's files of one shape
        cost one pinned allocation).  decode() reads the status words, which waits for the upload, before the next call fills it."""
        if self._staging is None or self._staging.numel() < nbytes:
            self._staging = torch.empty(nbytes * 5 // 4, dtype=torch.uint8, pin_memory=True)
        return self._staging[:nbytes]

    def workspace(self, segment_bytes: int) -> torch.Tensor:
        need = sizes(self.frame, segment_bytes)[0]
        if self._workspace is None or self._workspace.numel() < need:
            self._for_bytes = max(int(segment_bytes), min(int(segment_bytes) * 5 // 4, _lib_jpegdec.JPEGDEC_MAX_SEGMENT))
            self._workspace = torch.empty(max(need, sizes(self.frame, self._for_bytes)[0]), dtype=torch.uint8, device=self.device)
        return self._workspace

    def launch(self, header_ptr: int, segment_ptr: int, segment_bytes: int, out: torch.Tensor, rounds_done: int, rounds: int) -> torch.Tensor:
        """One scg_jpegdec_decode on the current stream of the plan's device; returns the workspace (its first 16 bytes: the status)."""
        ws = self.workspace(segment_bytes)
        with torch.cuda.device(self.device):
            check(_lib_jpegdec.load().scg_jpegdec_decode(
                self.frame.ctypes.data_as(C.POINTER(C.c_int32)), header_ptr, segment_ptr, int(segment_bytes), out.data_ptr(), out.numel(),
                ws.data_ptr(), ws.numel(), int(rounds_done), int(rounds), _lib.stream_of(self.device, "jpeg_decode.decode")),
                "scg_jpegdec_decode")
        return ws


_PLANS: Dict[tuple, JpegDecodePlan] = {}


def plan_of(frame: np.ndarray, device) -> JpegDecodePlan:
    key = (tuple(int(x) for x in frame), str(device))
    plan = _PLANS.get(key)
    if plan is None:
        if len(_PLANS) >= 16:
            _PLANS.pop(next(iter(_PLANS)))
        plan = _PLANS[key] = JpegDecodePlan(frame, device)
    return plan


def _device(device) -> torch.device:
    dev = torch.device(device)
    if dev.type != "cuda":
        raise _err("the decoder runs on the ROCm GPU ('cuda'); there is no CPU path (Pillow decodes on the host)")
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    return dev


def _read_status(ws: torch.Tensor) -> np.ndarray:
    """The call's host read: the four status words."""
    LAST["host_reads"] = int(LAST.get("host_reads", 0)) + 1
    return ws[:16].view(torch.int32).cpu().numpy().astype(np.int64) & 0xFFFFFFFF


def _host_route(source, dev: torch.device, out: Optional[torch.Tensor]) -> torch.Tensor:
    from PIL import Image
    with Image.open(source if isinstance(source, (str, os.PathLike)) else io.BytesIO(source)) as im:
        arr = np.array(im)
    LAST["route"] = "host"
    t = torch.from_numpy(arr)
    if out is not None:
        if tuple(out.shape) != tuple(t.shape) or out.dtype != t.dtype:
            raise _err(f"out is {out.dtype} {tuple(out.shape)}, the image {t.dtype} {tuple(t.shape)}")
        return out.copy_(t)
    return t.to(dev)


@torch.no_grad()
def decode(data_or_path, device="cuda", out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The pixels of a JPEG file — a path or the file's bytes — as a device uint8 tensor (H, W, 3) or (H, W): what
    torch.from_numpy(np.asarray(Image.open(path))).to(device) gives.  `out`: a contiguous uint8 tensor of that shape on the device
    to decode into.  One pinned staging buffer, one upload, the launches, one host read of the status words (one more per further
    batch of sync rounds, which no file seen so far has needed)."""
    dev = _device(device)
    LAST.clear()
    LAST["host_reads"] = 0
    if isinstance(data_or_path, (str, os.PathLike)):
        with open(data_or_path, "rb") as fh:
            data = fh.read()
    else:
        data = bytes(data_or_path)
        data_or_path = data                                                      # what the host route opens
    info = parse(data)
    if info is None:
        return _host_route(data_or_path, dev, out)
    upload = stage(info, data, plan_of(info.frame, dev)).to(dev, non_blocking=True)      # the ONE upload
    res, status = decode_staged(info, upload, out)
    if int(status[0]) != 0:
        # truncated or damaged: Pillow decides what such a file is
        return _host_route(data_or_path, dev, out)
    return res


def stage(info: JpegInfo, data: bytes, plan: Optional[JpegDecodePlan] = None) -> torch.Tensor:
    """The pinned staging buffer of a file: [header block | the file's bytes]; the plan's own buffer when one is given."""
    nbytes = HEADER_BYTES + len(data)
    staged = torch.empty(nbytes, dtype=torch.uint8, pin_memory=True) if plan is None else plan.staging(nbytes)
    view = staged.numpy()
    view[:HEADER_BYTES] = header_block(info)
    view[HEADER_BYTES:] = np.frombuffer(data, dtype=np.uint8)
    return staged


@torch.no_grad()
def decode_staged(info: JpegInfo, upload: torch.Tensor, out: Optional[torch.Tensor] = None):
    """The launches and the host read for a staged buffer (stage()) that lies on the device: (pixels, the four status words).  The
    pixels are right only when status[0] == 0; decode() sends every other file to Pillow."""
    dev = upload.device
    plan = plan_of(info.frame, dev)
    if out is None:
        out = torch.empty(plan.shape, dtype=torch.uint8, device=dev)
    elif tuple(out.shape) != plan.shape or out.dtype != torch.uint8 or out.device != dev or not out.is_contiguous():
        raise _err(f"out must be a contiguous uint8 tensor of shape {plan.shape} on {dev}, not {out.dtype} {tuple(out.shape)} on {out.device}")
    if upload.dtype != torch.uint8 or not upload.is_contiguous() or upload.numel() < HEADER_BYTES + info.segment_end:
        raise _err("the staged buffer is [header block | file] as contiguous uint8")
    seg_bytes = info.segment_end - info.segment_start
    seg_ptr = upload.data_ptr() + HEADER_BYTES + info.segment_start
    max_rounds = sizes(info.frame, seg_bytes)[2]
    done, rounds = 0, min(FIRST_ROUNDS, max_rounds)
    while True:
        ws = plan.launch(upload.data_ptr(), seg_ptr, seg_bytes, out, done, rounds)
        status = _read_status(ws)
        done += rounds
        if not int(status[0]) & _lib_jpegdec.JPEGDEC_BAD_SYNC or done >= max_rounds:      # (unsettled states set other bits too)
            break
        rounds = min(MORE_ROUNDS, max_rounds - done)
    LAST.update(status=int(status[0]), rounds=int(status[1]), launched=done, blocks=int(status[2]), segment_bytes=seg_bytes,
                route="device" if int(status[0]) == 0 else "refused")
    return out, status


# --------------------------------------------------------------------------------------------------------------------------------
# a batch: a scene's images in one upload, one call, one read
# --------------------------------------------------------------------------------------------------------------------------------
IMAGE_WORDS = _lib_jpegdec.JPEGDEC_IMAGE_WORDS
_ALIGN = 16


def _round_up(v: int, to: int) -> int:
    return (v + to - 1) // to * to


def table_words(n: int) -> int:
    """uint32 words of the table block of n images: the records, then three prefix tables of n + 1 (scg_jpegdec.h)."""
    return n * IMAGE_WORDS + 3 * (n + 1)


class BatchStage:
    """Where everything lies in the ONE staging buffer of a batch: [table block | distinct header blocks | segments], every part
    at a 16-byte offset.  Host only.  Header blocks are de-duplicated by content (a video's frames, files written with the
    standard tables); of a file only its entropy-coded segment is staged."""

    def __init__(self, infos, datas):
        self.infos, self.datas = list(infos), list(datas)
        self.n = len(self.infos)
        self.table_bytes = _round_up(4 * table_words(self.n), _ALIGN)
        self.headers = []                                        # the distinct blocks, in order of first use
        seen: Dict[bytes, int] = {}
        at = self.table_bytes
        self.header_offsets = []
        for info in self.infos:
            block = header_block(info)
            key = block.tobytes()
            if key not in seen:
                seen[key] = self.table_bytes + HEADER_BYTES * len(self.headers)
                self.headers.append(block)
            self.header_offsets.append(seen[key])
        at += HEADER_BYTES * len(self.headers)
        self.segment_offsets, self.segment_bytes = [], []
        for info in self.infos:
            self.segment_offsets.append(at)
            self.segment_bytes.append(info.segment_end - info.segment_start)
            at = _round_up(at + self.segment_bytes[-1], _ALIGN)
        self.nbytes = at
        self.frames = np.ascontiguousarray(np.stack([np.asarray(i.frame, dtype=np.int32) for i in self.infos])) if self.n else \
            np.zeros((0, _lib_jpegdec.JPEGDEC_FRAME_WORDS), dtype=np.int32)
        self.table = np.zeros(table_words(self.n), dtype=np.uint32)
        self.out_offsets = np.zeros(self.n, dtype=np.uint64)
        self.workspace_bytes = self.out_bytes = self.max_rounds = 0

    def plan(self) -> "BatchStage":
        """scg_jpegdec_batch_plan: the table block, each image's place in the output, the totals."""
        u64 = lambda values: np.ascontiguousarray(values, dtype=np.uint64)                        # noqa: E731
        seg, hdr, sat = u64(self.segment_bytes), u64(self.header_offsets), u64(self.segment_offsets)
        ws, ob, mr = C.c_uint64(), C.c_uint64(), C.c_int32()
        p64 = C.POINTER(C.c_uint64)
        check(_lib_jpegdec.load().scg_jpegdec_batch_plan(
            self.n, self.frames.ctypes.data_as(C.POINTER(C.c_int32)), seg.ctypes.data_as(p64), hdr.ctypes.data_as(p64), sat.ctypes.data_as(p64),
            self.nbytes, self.table.ctypes.data_as(C.POINTER(C.c_uint32)), self.table.size, self.out_offsets.ctypes.data_as(p64),
            C.byref(ws), C.byref(ob), C.byref(mr)), "scg_jpegdec_batch_plan")
        self.workspace_bytes, self.out_bytes, self.max_rounds = int(ws.value), int(ob.value), int(mr.value)
        return self

    def fill(self, view: np.ndarray) -> None:
        """Write the staged bytes into view[0, nbytes) (uint8): what the ONE upload carries."""
        view[:4 * self.table.size] = self.table.view(np.uint8)
        for k, block in enumerate(self.headers):
            at = self.table_bytes + HEADER_BYTES * k
            view[at:at + HEADER_BYTES] = block
        for info, data, at, nb in zip(self.infos, self.datas, self.segment_offsets, self.segment_bytes):
            view[at:at + nb] = np.frombuffer(data, dtype=np.uint8, count=nb, offset=info.segment_start)

    def shape(self, i: int) -> tuple:
        info = self.infos[i]
        return (info.H, info.W) + ((3,) if info.components == 3 else ())


_BATCH_BUFFERS: Dict[str, object] = {}


def _batch_staging(nbytes: int) -> torch.Tensor:
    """nbytes of the module's pinned staging buffer (grown with a quarter to spare, then reused; decode_batch reads the status
    words, which waits for the upload, before the next chunk fills it)."""
    buf = _BATCH_BUFFERS.get("staging")
    if buf is None or buf.numel() < nbytes:
        buf = _BATCH_BUFFERS["staging"] = torch.empty(nbytes * 5 // 4, dtype=torch.uint8, pin_memory=True)
    return buf[:nbytes]


def _batch_workspace(nbytes: int, dev: torch.device) -> torch.Tensor:
    key = ("workspace", str(dev))
    buf = _BATCH_BUFFERS.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = _BATCH_BUFFERS[key] = torch.empty(max(nbytes * 5 // 4, _ALIGN), dtype=torch.uint8, device=dev)
    return buf


def launch_batch(stage: BatchStage, upload: torch.Tensor, out: torch.Tensor, workspace: torch.Tensor, rounds: int) -> None:
    """One scg_jpegdec_decode_batch on the current stream of the upload's device; the table block lies at the upload's front."""
    dev = upload.device
    with torch.cuda.device(dev):
        check(_lib_jpegdec.load().scg_jpegdec_decode_batch(
            stage.n, stage.frames.ctypes.data_as(C.POINTER(C.c_int32)), stage.table.ctypes.data_as(C.POINTER(C.c_uint32)), upload.data_ptr(),
            upload.data_ptr(), upload.numel(), out.data_ptr(), out.numel(), workspace.data_ptr(), workspace.numel(), int(rounds),
            _lib.stream_of(dev, "jpeg_decode.decode_batch")), "scg_jpegdec_decode_batch")


def _read(source):
    if isinstance(source, (str, os.PathLike)):
        with open(source, "rb") as fh:
            return fh.read(), source
    data = bytes(source)
    return data, data


@torch.no_grad()
def decode_batch(sources, device="cuda", max_workspace_bytes: int = 4 << 30):
    """What [decode(s) for s in sources] returns or raises (the exception of the first failing source in order), with every file
    parse() accepts staged into ONE pinned buffer — table block, distinct header blocks, entropy-coded segments — for ONE upload,
    ONE scg_jpegdec_decode_batch with min(FIRST_ROUNDS, max_rounds) sync launches and ONE host read of the 4 n status words.  A
    file parse() refuses, and one whose status is not 0 (unsettled, truncated, damaged), goes through decode() afterwards.  A list
    whose workspace would exceed max_workspace_bytes is split into consecutive chunks, each with its own upload and read.  The
    outputs of a chunk are views of ONE buffer in input order, 16-byte aligned: images of one shape lie at a constant stride.
    LAST: uploads, host_reads, headers (distinct header blocks), chunks, and per image status, rounds and route."""
    dev = _device(device)
    sources = list(sources)
    n = len(sources)
    report = dict(uploads=0, host_reads=0, headers=0, chunks=0, status=[None] * n, rounds=[None] * n, route=[None] * n)
    LAST.clear()
    LAST.update(report)
    if n == 0:
        return []
    read = [_read(s) for s in sources]
    infos = [parse(data) for data, _src in read]
    results = [None] * n
    accepted = [i for i in range(n) if infos[i] is not None]
    at = 0
    while at < len(accepted):
        # the longest run of consecutive accepted files whose workspace fits (one file always goes)
        k = len(accepted) - at
        while True:
            members = accepted[at:at + k]
            stage = BatchStage([infos[i] for i in members], [read[i][0] for i in members]).plan()
            if stage.workspace_bytes <= max_workspace_bytes or k == 1:
                break
            k = max(1, min(k - 1, k * int(max_workspace_bytes) // stage.workspace_bytes))
        at += k
        staged = _batch_staging(stage.nbytes)
        stage.fill(staged.numpy())
        upload = staged.to(dev, non_blocking=True)                                         # the chunk's ONE upload
        out = torch.empty(max(stage.out_bytes, _ALIGN), dtype=torch.uint8, device=dev)
        ws = _batch_workspace(stage.workspace_bytes, dev)
        launch_batch(stage, upload, out, ws, min(FIRST_ROUNDS, stage.max_rounds))
        status = ws[:16 * stage.n].view(torch.int32).cpu().numpy().astype(np.int64).reshape(stage.n, 4) & 0xFFFFFFFF      # the ONE read
        report["uploads"] += 1
        report["host_reads"] += 1
        report["chunks"] += 1
        report["headers"] += len(stage.headers)
        for j, i in enumerate(members):
            report["status"][i], report["rounds"][i] = int(status[j, 0]), int(status[j, 1])
            if int(status[j, 0]) == 0:
                first = int(stage.out_offsets[j])
                shape = stage.shape(j)
                results[i] = out[first:first + int(np.prod(shape))].view(shape)
                report["route"][i] = "device"
    for i in range(n):                                                                     # in order: the first failure raises
        if results[i] is None:
            results[i] = decode(read[i][1], dev)
            report["host_reads"] += int(LAST.get("host_reads", 0))
            report["uploads"] += 1
            report["route"][i] = "single " + str(LAST.get("route"))
    LAST.clear()
    LAST.update(report)
    return results

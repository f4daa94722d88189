// jpegunpack.hip — libscg_jpegdec.so: baseline JPEG files decoded on the GPU (include/jpegdec/scg_jpegdec.h states the rule and the call; it
// is the contract, and tests/jpegdec_refs.py restates it in numpy).
//
// The entropy-coded segment is one serial bit stream.  It is decoded in parallel and exactly by the self-synchronising scheme: a
// thread per subsequence of SCG_JPEGDEC_SUBSEQ bytes decodes from a guessed state, then from its predecessor's exit state until
// no exit state changes; subsequence 0 starts from the truth.  Kernels, in launch order:
//
//   jpegdec_sync_kernel    a workgroup per 256 subsequences; the four Huffman tables in LDS (3.5 KiB); the rounds inside the
//                          workgroup in LDS behind barriers, the rounds across workgroups one launch each
//   jpegdec_count_kernel   blocks that end in a subsequence, DC sums behind its last restart marker, the restart flag
//   jpegdec_scan_kernel    ONE workgroup: first block and DC predictors of every subsequence, the status words
//   jpegdec_write_kernel   int16 coefficients, natural order, into the (cleared) coefficient buffer
//   jpegdec_idct_kernel    eight threads a block: dequantise, columns, rows (jidctint islow), bytes of the component planes
//   jpegdec_colour_kernel  crop, upsample, convert; a lane owns 4 output bytes of a row
//
// Each kernel is a body over an image view (View) with two fronts: the single-image kernel fills the view from its arguments, the
// jpegdec_batch_* kernel from the image table of scg_jpegdec_decode_batch, where a workgroup finds its image from blockIdx.x alone.
// One decode function (run<kMode>) serves sync, count and write, so the three cannot disagree about a state.  No workgroup waits
// for another, nothing is allocated, no float atomics; the same input gives the same bytes.
#include "../../include/jpegdec/scg_jpegdec.h"

#include <string.h>

#include "compact.h"
#include "host_align.h"
#include "host_error.h"

namespace scg {
namespace {

constexpr int kT = SCG_JPEGDEC_THREADS;
constexpr uint32_t kSubBits = 8u * SCG_JPEGDEC_SUBSEQ;
constexpr int kCtlWords = 4;                       // the status words in front of the per-launch change counters
constexpr int kIdctBlocks = kT / 8;                // blocks of a workgroup of the idct kernel
constexpr int kIdctStride = 73;                    // dwords of a block in LDS: 8 rows of 9, one more to spread the blocks over the banks
static_assert(kT == kBlock, "compact.h's scans are instantiated for this workgroup");

thread_local ErrorText g_err = {};

__constant__ uint8_t d_natural[64] = {0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20,
                                      13, 6, 7, 14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45,
                                      38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

struct HuffDev {
    uint16_t look[256];
    int32_t maxcode[16];
    int32_t valoff[16];
    uint8_t vals[256];
};
struct HeaderDev {
    uint16_t quant[4][64];
    HuffDev huff[4];
};
static_assert(sizeof(HuffDev) == 896 && sizeof(HeaderDev) == SCG_JPEGDEC_HEADER_BYTES, "the header block of scg_jpegdec.h");

struct Frame {
    int H, W, comps, hs, vs, ri;
    int tq[3], td[3], ta[3];
    int bpm, ybl;                  // blocks of an MCU, of them Y's
    int mcux, mcuy;
    uint32_t nblocks, nbytes, nsub, nwg;
    int pw[2], ph[2];              // the padded planes: Y, chroma
};

struct Layout {
    uint64_t ctl, entry, exit_, bnd, cnt, dcs, coef, coef_bytes, planes, plane1, plane2, total;
};

// One image as the kernel bodies see it: its frame (passed beside the view: scg_jpegdec_decode's kernels have it among their
// arguments, scg_jpegdec_decode_batch's put it into LDS, so that neither indexes its table ids in scratch) and where its buffers
// lie.  The single-image kernels fill the view from their arguments, the batched ones from the image table; the bodies below are
// the same for both.
struct View {
    const HeaderDev* hdr;
    const uint8_t* s;
    uint64_t *entry, *exit_, *bnd;
    uint32_t *status, *chg, *cnt;  // the four status words; the change counter of every sync launch
    int4* dcs;
    int16_t* coef;
    uint8_t *p0, *p1, *p2, *out;
};

// The frame of SCG_JPEGDEC_FRAME_WORDS words and a segment's bytes: 0, or which rule of the header it breaks first (the host turns
// that into its message, a kernel leaves such a record alone).  The one place where the derived sizes are computed.
enum { kFrameDim = 1, kFrameComps, kFrameSampling, kFrameRestart, kFrameTables, kFrameLast, kFrameSegment, kFrameBlocks };
__host__ __device__ inline int frame_from(const int32_t* w, uint64_t segment_bytes, Frame* f) {
    f->H = w[0]; f->W = w[1]; f->comps = w[2]; f->hs = w[3]; f->vs = w[4]; f->ri = w[5];
    if (f->H < 1 || f->H > SCG_JPEGDEC_MAX_DIM || f->W < 1 || f->W > SCG_JPEGDEC_MAX_DIM) return kFrameDim;
    if (f->comps != 1 && f->comps != 3) return kFrameComps;
    const bool sampling_ok = f->comps == 1 ? (f->hs == 1 && f->vs == 1) : ((f->hs == 1 || f->hs == 2) && (f->vs == 1 || f->vs == 2) && f->vs <= f->hs);
    if (!sampling_ok) return kFrameSampling;
    if (f->ri < 0 || f->ri > 65535) return kFrameRestart;
    for (int c = 0; c < 3; ++c) {
        f->tq[c] = w[6 + c]; f->td[c] = w[9 + c]; f->ta[c] = w[12 + c];
    }
    for (int c = 0; c < 3; ++c)
        if (f->tq[c] < 0 || f->tq[c] > 3 || f->td[c] < 0 || f->td[c] > 1 || f->ta[c] < 0 || f->ta[c] > 1) return kFrameTables + (c << 8);
    if (w[15] != 0) return kFrameLast;
    if (segment_bytes < 1 || segment_bytes > SCG_JPEGDEC_MAX_SEGMENT) return kFrameSegment;
    f->ybl = f->hs * f->vs;
    f->bpm = f->ybl + (f->comps == 3 ? 2 : 0);
    f->mcux = (f->W + 8 * f->hs - 1) / (8 * f->hs);
    f->mcuy = (f->H + 8 * f->vs - 1) / (8 * f->vs);
    const uint64_t nblocks = (uint64_t)f->mcux * f->mcuy * f->bpm;
    f->nblocks = (uint32_t)nblocks;
    if (nblocks > 0x03FFFFFFull) return kFrameBlocks;
    f->nbytes = (uint32_t)segment_bytes;
    f->nsub = (uint32_t)((segment_bytes + SCG_JPEGDEC_SUBSEQ - 1) / SCG_JPEGDEC_SUBSEQ);
    f->nwg = (f->nsub + kT - 1) / kT;
    f->pw[0] = f->mcux * f->hs * 8; f->ph[0] = f->mcuy * f->vs * 8;
    f->pw[1] = f->mcux * 8; f->ph[1] = f->mcuy * 8;
    return 0;
}
__host__ __device__ inline uint32_t idct_groups(const Frame& f) { return (f.nblocks + kIdctBlocks - 1) / kIdctBlocks; }
__host__ __device__ inline uint32_t colour_chunks(const Frame& f) { return (uint32_t)((f.W * f.comps + 4 * kT - 1) / (4 * kT)); }

// ---- the stream ------------------------------------------------------------------------------------------------------------------
// Bits MSB first in `buf`, `nbits` of them; `sbuf` moves with it and holds, at the lowest bit of every FF data byte, the flag of
// the stuffed 00 behind it, so that the position of the next bit in the STUFFED stream is (pos - popcount(sbuf)) * 8 - nbits.
struct Reader {
    const uint8_t* s;
    uint32_t n, pos;
    uint64_t buf, sbuf;
    int nbits, stop;               // stop: 1 = RSTn at pos, 2 = the segment's end (or any other marker) at pos

    __device__ __forceinline__ void fill() {
        while (nbits <= 56 && !stop) {
            if (pos >= n) {
                stop = 2;
                break;
            }
            const uint32_t b = s[pos];
            if (b != 0xFFu) {
                buf |= (uint64_t)b << (56 - nbits);
                nbits += 8;
                pos += 1;
            } else {
                const uint32_t m = pos + 1 < n ? s[pos + 1] : 0xD9u;
                if (m == 0u) {
                    buf |= 0xFFull << (56 - nbits);
                    sbuf |= 1ull << (56 - nbits);
                    nbits += 8;
                    pos += 2;
                } else {
                    stop = (m & 0xF8u) == 0xD0u ? 1 : 2;
                }
            }
        }
    }
    __device__ __forceinline__ void drop(int k) {
        buf <<= k;
        sbuf <<= k;
        nbits -= k;
    }
    __device__ __forceinline__ void start(uint32_t bitpos) {
        pos = bitpos >> 3;
        buf = sbuf = 0;
        nbits = stop = 0;
        fill();
        const int k = (int)(bitpos & 7u);
        if (k <= nbits) drop(k);
    }
    __device__ __forceinline__ uint32_t position() const { return (pos - (uint32_t)__popcll(sbuf)) * 8u - (uint32_t)nbits; }
};

__device__ __forceinline__ uint64_t pack_state(uint32_t p, int blk, int zz) { return (uint64_t)p | ((uint64_t)((blk << 8) | zz) << 32); }

struct Acc {
    uint32_t blocks = 0, reset = 0, err = 0;
    int32_t dc[3] = {0, 0, 0};     // count: sums behind the last marker; write: the predictors
    uint32_t B = 0;                // write: the block being filled
    int16_t* coef = nullptr;
};

// kMode 0: the exit state alone; 1: count; 2: write.  Decodes the symbols that BEGIN in [state, end) and returns the state at the
// first one that does not.
template <int kMode>
__device__ uint64_t run(const Frame& f, const HuffDev* huff, const uint8_t* s, uint64_t state, uint32_t end, Acc& acc) {
    uint32_t p = (uint32_t)state;
    const uint32_t total = f.nbytes * 8u;
    if (p >= end || p >= total) return state;
    int blk = (int)((state >> 40) & 0xFFu), zz = (int)((state >> 32) & 63u);
    blk = blk < f.bpm ? blk : 0;
    Reader r;
    r.s = s;
    r.n = f.nbytes;
    r.start(p);
    const int per_interval = f.ri * f.bpm;
    // write: is the byte pair in front of the next symbol a restart marker?  (FF in the data is always followed by 00.)
    bool behind_marker = kMode == 2 && (p & 7u) == 0u && p >= 16u && s[(p >> 3) - 2u] == 0xFFu && (s[(p >> 3) - 1u] & 0xF8u) == 0xD0u;
    for (;;) {
        p = r.position();
        if (p >= end || p >= total) break;
        const int comp = blk < f.ybl ? 0 : blk - f.ybl + 1;
        const bool is_dc = zz == 0;
        const HuffDev& h = huff[is_dc ? (f.td[comp] & 1) : 2 + (f.ta[comp] & 1)];
        const uint32_t peek = (uint32_t)(r.buf >> 48);
        const uint32_t look = h.look[peek >> 8];
        int len = (int)((look >> 8) & 15u), sym = (int)(look & 255u);
        if (len == 0) {
            for (int l = 9; l <= 16; ++l) {
                const int c = (int)(peek >> (16 - l));
                if (c <= h.maxcode[l - 1]) {
                    sym = h.vals[(c + h.valoff[l - 1]) & 255];
                    len = l;
                    break;
                }
            }
        }
        const int size = sym & 15;
        const int need = (len ? len : 16) + size;
        if (r.stop && (need > r.nbits || (len == 0 && r.nbits < 16))) {
            if (r.stop == 2) {                      // the end: what is left are pad bits
                p = total;
                break;
            }
            // RSTn: whatever the state, the stream goes on behind the marker in the known one
            const uint32_t at = r.pos;
            if (kMode == 2) {
                const uint32_t m = s[at + 1] & 7u;
                // (in front of the first block no marker is due: B == 0 is refused outright, its index would wrap to 7)
                if (blk != 0 || zz != 0 || per_interval == 0 || acc.B == 0u || acc.B % (uint32_t)per_interval != 0u ||
                    ((acc.B / (uint32_t)per_interval - 1u) & 7u) != m)
                    acc.err |= SCG_JPEGDEC_BAD_RESTART;
            }
            if (kMode != 0) {
                acc.dc[0] = acc.dc[1] = acc.dc[2] = 0;
                acc.reset = 1;
            }
            blk = zz = 0;
            r.start((at + 2u) * 8u);
            behind_marker = true;
            continue;
        }
        if (len == 0) {                             // no table holds it: pass one bit over, so that every state moves on
            acc.err |= SCG_JPEGDEC_BAD_CODE;
            r.drop(1);
            r.fill();
            continue;
        }
        // an interval is full: only a marker may follow
        if (kMode == 2 && is_dc && blk == 0 && per_interval != 0 && acc.B != 0u && acc.B % (uint32_t)per_interval == 0u && !behind_marker)
            acc.err |= SCG_JPEGDEC_BAD_RESTART;
        behind_marker = false;
        int v = 0;
        if (size) {
            v = (int)((r.buf << len) >> (64 - size));
            if (v < (1 << (size - 1))) v -= (1 << size) - 1;
        }
        r.drop(need);
        r.fill();
        bool ends = false;
        if (is_dc) {
            if (sym > 11) acc.err |= SCG_JPEGDEC_BAD_CODE;
            if (kMode != 0) acc.dc[comp] += v;
            if (kMode == 2 && acc.B < f.nblocks) acc.coef[(size_t)acc.B * 64] = (int16_t)acc.dc[comp];
            zz = 1;
        } else if (size == 0) {
            if ((sym >> 4) == 15) {
                zz += 16;
                if (zz > 64) acc.err |= SCG_JPEGDEC_BAD_ZIGZAG;
                ends = zz >= 64;
            } else {
                ends = true;                        // EOB
            }
        } else {
            if (size > 10) acc.err |= SCG_JPEGDEC_BAD_CODE;
            zz += sym >> 4;
            if (zz > 63) {
                acc.err |= SCG_JPEGDEC_BAD_ZIGZAG;
                zz = 63;
            }
            if (kMode == 2 && acc.B < f.nblocks) acc.coef[(size_t)acc.B * 64 + d_natural[zz]] = (int16_t)v;
            zz += 1;
            ends = zz >= 64;
        }
        if (ends) {
            if (kMode == 1) acc.blocks += 1;
            if (kMode == 2) acc.B += 1;
            zz = 0;
            blk = blk + 1 < f.bpm ? blk + 1 : 0;
        }
    }
    return pack_state(p, blk, zz);
}

__device__ __forceinline__ void load_tables(HuffDev* dst, const HeaderDev* hdr) {
    const uint32_t* from = reinterpret_cast<const uint32_t*>(hdr->huff);
    uint32_t* to = reinterpret_cast<uint32_t*>(dst);
    for (int i = threadIdx.x; i < (int)(4 * sizeof(HuffDev) / 4); i += kT) to[i] = from[i];
    __syncthreads();
}

// ---- sync ------------------------------------------------------------------------------------------------------------------------
// Workgroup g of the image's own grid: thread t owns subsequence g * kT + t of THIS image, and nothing but the view says where its
// states, its hand-over words and its change counters lie.
__device__ __forceinline__ void sync_body(const Frame& f, const View& v, uint32_t g, int round) {
    __shared__ HuffDev s_huff[4];
    __shared__ uint64_t s_exit[kT];
    const uint8_t* s = v.s;
    uint64_t *entry = v.entry, *exit_ = v.exit_;
    load_tables(s_huff, v.hdr);
    const uint32_t t = threadIdx.x, i = g * kT + t;
    const bool live = i < f.nsub;
    const uint32_t end = (i + 1u) * kSubBits;
    const uint64_t* bin = v.bnd + (size_t)(round & 1) * f.nwg;
    uint64_t* bout = v.bnd + (size_t)((round + 1) & 1) * f.nwg;
    Acc none;
    uint64_t used = 0, mine = 0;
    if (live) {
        if (round == 0) {
            used = pack_state(i * kSubBits, 0, 0);
            mine = run<0>(f, s_huff, s, used, end, none);
        } else {
            used = entry[i];
            mine = exit_[i];
        }
    }
    // the state in front of the workgroup: the truth for the first one, else what the launch before left
    const uint64_t head = g == 0 ? 0ull : (round == 0 ? used : bin[g - 1]);
    s_exit[t] = mine;
    int head_changed = 0;
    for (int it = 0; it < kT; ++it) {
        __syncthreads();
        const uint64_t pred = t == 0 ? head : s_exit[t - 1];
        const bool ch = live && pred != used;
        __syncthreads();
        if (ch) {
            used = pred;
            mine = run<0>(f, s_huff, s, used, end, none);
            s_exit[t] = mine;
            if (t == 0) head_changed = 1;
        }
        if (!__syncthreads_or(ch ? 1 : 0)) break;
    }
    if (live) {
        entry[i] = used;
        exit_[i] = mine;
        if (t == kT - 1 || i == f.nsub - 1u) bout[g] = mine;
    }
    if (t == 0 && (head_changed || (round == 0 && g > 0))) atomicAdd(&v.chg[round], 1u);
}

__global__ void __launch_bounds__(kT) jpegdec_sync_kernel(Frame f, const HeaderDev* hdr, const uint8_t* s, uint64_t* entry, uint64_t* exit_,
                                                          uint64_t* bnd, uint32_t* ctl, int round) {
    View v = {};
    v.hdr = hdr; v.s = s; v.entry = entry; v.exit_ = exit_; v.bnd = bnd; v.status = ctl; v.chg = ctl + kCtlWords;
    sync_body(f, v, blockIdx.x, round);
}

// ---- count, scan, write ----------------------------------------------------------------------------------------------------------
template <int kMode>
__device__ __forceinline__ void pass_body(const Frame& f, const View& v, uint32_t g) {
    __shared__ HuffDev s_huff[4];
    load_tables(s_huff, v.hdr);
    const uint32_t i = g * kT + threadIdx.x;
    if (i >= f.nsub) return;
    Acc acc;
    if (kMode == 2) {
        const int4 d = v.dcs[i];
        acc.B = v.cnt[i];
        acc.dc[0] = d.y; acc.dc[1] = d.z; acc.dc[2] = d.w;
        acc.coef = v.coef;
    }
    run<kMode>(f, s_huff, v.s, i == 0 ? 0ull : v.exit_[i - 1], (i + 1u) * kSubBits, acc);
    if (kMode == 1) {
        v.cnt[i] = acc.blocks;
        v.dcs[i] = make_int4((int)acc.reset, acc.dc[0], acc.dc[1], acc.dc[2]);
    }
    if (acc.err) atomicOr(&v.status[0], acc.err);
}

template <int kMode>
__global__ void __launch_bounds__(kT) jpegdec_pass_kernel(Frame f, const HeaderDev* hdr, const uint8_t* s, uint64_t* exit_, uint32_t* cnt,
                                                          int4* dcs, int16_t* coef, uint32_t* ctl) {
    View v = {};
    v.hdr = hdr; v.s = s; v.exit_ = exit_; v.cnt = cnt; v.dcs = dcs; v.coef = coef; v.status = ctl;
    pass_body<kMode>(f, v, blockIdx.x);
}

// (reset flag, sums): b behind a
__device__ __forceinline__ int4 behind(const int4 a, const int4 b) {
    return b.x ? b : make_int4(a.x, a.y + b.y, a.z + b.z, a.w + b.w);
}
__device__ __forceinline__ int4 shfl_up4(const int4 v, int off) {
    return make_int4(__shfl_up(v.x, off, kWave), __shfl_up(v.y, off, kWave), __shfl_up(v.z, off, kWave), __shfl_up(v.w, off, kWave));
}

// compact.h's carry scan under the operator above: v becomes its exclusive prefix in place, in subsequence order
__device__ __forceinline__ void carry_scan_reset(int4* v, int n) {
    constexpr int kWaves = kT / kWave;
    __shared__ int4 s_w[kWaves];
    const int lane = lane_id(), w = wave_id();
    int4 carry = make_int4(0, 0, 0, 0);
    for (int base = 0; base < n; base += kT) {
        const int g = base + (int)threadIdx.x;
        int4 x = g < n ? v[g] : make_int4(0, 0, 0, 0);
        for (int off = 1; off < kWave; off <<= 1) {
            const int4 y = shfl_up4(x, off);
            if (lane >= off) x = behind(y, x);
        }
        if (lane == kWave - 1) s_w[w] = x;
        int4 ex = shfl_up4(x, 1);
        if (lane == 0) ex = make_int4(0, 0, 0, 0);
        __syncthreads();
        int4 before = carry, all = carry;
        for (int j = 0; j < kWaves; ++j) {
            if (j < w) before = behind(before, s_w[j]);
            all = behind(all, s_w[j]);
        }
        if (g < n) v[g] = behind(before, ex);
        carry = all;
        __syncthreads();
    }
}

__device__ __forceinline__ void scan_body(const Frame& f, const View& v, int rounds_run) {
    uint32_t total[1];
    carry_scan<1, kT>(v.cnt, (int)f.nsub, total);
    carry_scan_reset(v.dcs, (int)f.nsub);
    if (threadIdx.x == 0) {
        uint32_t bad = 0, settled = 0;
        for (int k = 0; k < rounds_run && !settled; ++k)
            if (v.chg[k] == 0u) settled = (uint32_t)k + 1u;
        if (v.chg[rounds_run - 1] != 0u) bad |= SCG_JPEGDEC_BAD_SYNC;
        if (total[0] != f.nblocks) bad |= SCG_JPEGDEC_BAD_COUNT;
        if (bad) atomicOr(&v.status[0], bad);
        v.status[1] = settled;
        v.status[2] = total[0];
        v.status[3] = 0u;
    }
}

__global__ void __launch_bounds__(kT) jpegdec_scan_kernel(Frame f, uint32_t* cnt, int4* dcs, uint32_t* ctl, int rounds_run) {
    View v = {};
    v.cnt = cnt; v.dcs = dcs; v.status = ctl; v.chg = ctl + kCtlWords;
    scan_body(f, v, rounds_run);
}

// ---- idct: libjpeg's jidctint.c, islow -------------------------------------------------------------------------------------------
template <int kShift>
__device__ __forceinline__ void idct_1d(int* d) {
    int z2 = d[2], z3 = d[6];
    int z1 = (z2 + z3) * 4433;
    int tmp2 = z1 + z3 * -15137, tmp3 = z1 + z2 * 6270;
    int tmp0 = (d[0] + d[4]) * 8192, tmp1 = (d[0] - d[4]) * 8192;
    const int tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    tmp0 = d[7]; tmp1 = d[5]; tmp2 = d[3]; tmp3 = d[1];
    z1 = tmp0 + tmp3; z2 = tmp1 + tmp2; z3 = tmp0 + tmp2;
    int z4 = tmp1 + tmp3;
    const int z5 = (z3 + z4) * 9633;
    tmp0 *= 2446; tmp1 *= 16819; tmp2 *= 25172; tmp3 *= 12299;
    z1 *= -7373; z2 *= -20995; z3 *= -16069; z4 *= -3196;
    z3 += z5; z4 += z5;
    tmp0 += z1 + z3; tmp1 += z2 + z4; tmp2 += z2 + z3; tmp3 += z1 + z4;
    constexpr int half = 1 << (kShift - 1);
    d[0] = (tmp10 + tmp3 + half) >> kShift; d[7] = (tmp10 - tmp3 + half) >> kShift;
    d[1] = (tmp11 + tmp2 + half) >> kShift; d[6] = (tmp11 - tmp2 + half) >> kShift;
    d[2] = (tmp12 + tmp1 + half) >> kShift; d[5] = (tmp12 - tmp1 + half) >> kShift;
    d[3] = (tmp13 + tmp0 + half) >> kShift; d[4] = (tmp13 - tmp0 + half) >> kShift;
}

__device__ __forceinline__ uint32_t to_byte(int v) { return (uint32_t)(v < 0 ? 0 : (v > 255 ? 255 : v)); }

// Workgroup g of the image's own grid: its blocks g * kIdctBlocks ...
__device__ __forceinline__ void idct_body(const Frame& f, const View& v, uint32_t g) {
    __shared__ int s_ws[kIdctBlocks * kIdctStride];
    __shared__ uint16_t s_q[4 * 64];
    const int16_t* coef = v.coef;
    uint8_t *y_plane = v.p0, *cb_plane = v.p1, *cr_plane = v.p2;
    const int t = threadIdx.x, lb = t >> 3, r = t & 7;
    s_q[t] = v.hdr->quant[t >> 6][t & 63];
    const uint32_t B = g * (uint32_t)kIdctBlocks + (uint32_t)lb;
    const bool live = B < f.nblocks;
    int* ws = s_ws + lb * kIdctStride;
    const uint32_t mcu = B / (uint32_t)f.bpm;
    const int k = (int)(B - mcu * (uint32_t)f.bpm);
    const int comp = k < f.ybl ? 0 : k - f.ybl + 1;
    __syncthreads();
    int d[8];
    if (live) {
        const int4 raw = *reinterpret_cast<const int4*>(coef + (size_t)B * 64 + r * 8);
        const uint16_t* q = s_q + (f.tq[comp] & 3) * 64 + r * 8;
        const int w[4] = {raw.x, raw.y, raw.z, raw.w};
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            ws[r * 9 + 2 * c] = (int)(int16_t)(w[c] & 0xFFFF) * (int)q[2 * c];
            ws[r * 9 + 2 * c + 1] = (w[c] >> 16) * (int)q[2 * c + 1];
        }
    }
    __syncthreads();
    if (live) {                                     // this thread's column
#pragma unroll
        for (int j = 0; j < 8; ++j) d[j] = ws[j * 9 + r];
        idct_1d<13 - 2>(d);
#pragma unroll
        for (int j = 0; j < 8; ++j) ws[j * 9 + r] = d[j];
    }
    __syncthreads();
    if (live) {                                     // this thread's row
#pragma unroll
        for (int j = 0; j < 8; ++j) d[j] = ws[r * 9 + j];
        idct_1d<13 + 2 + 3>(d);
        uint32_t lo = 0, hi = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            lo |= to_byte(d[j] + 128) << (8 * j);
            hi |= to_byte(d[j + 4] + 128) << (8 * j);
        }
        const int mx = (int)(mcu % (uint32_t)f.mcux), my = (int)(mcu / (uint32_t)f.mcux);
        uint8_t* plane = comp == 0 ? y_plane : (comp == 1 ? cb_plane : cr_plane);
        const int pw = f.pw[comp ? 1 : 0];
        const int bx = comp == 0 ? mx * f.hs + k % f.hs : mx, by = comp == 0 ? my * f.vs + k / f.hs : my;
        *reinterpret_cast<uint2*>(plane + ((size_t)by * 8 + r) * pw + (size_t)bx * 8) = make_uint2(lo, hi);
    }
}

__global__ void __launch_bounds__(kT) jpegdec_idct_kernel(Frame f, const HeaderDev* hdr, int16_t* coef, uint8_t* y_plane, uint8_t* cb_plane,
                                                          uint8_t* cr_plane) {
    View v = {};
    v.hdr = hdr; v.coef = coef; v.p0 = y_plane; v.p1 = cb_plane; v.p2 = cr_plane;
    idct_body(f, v, blockIdx.x);
}

// ---- colour ----------------------------------------------------------------------------------------------------------------------
struct Chroma {
    const uint8_t* c;
    int pw, cw, ch, hs, vs;
    __device__ __forceinline__ int at(int y, int x) const {
        if (hs == 1) return c[(size_t)y * pw + x];
        const int i = x >> 1;
        if (vs == 1) {
            const uint8_t* row = c + (size_t)y * pw;
            const int v = row[i];
            if (x == 0 || x == 2 * cw - 1) return v;
            return (x & 1) ? (3 * v + row[i + 1] + 2) >> 2 : (3 * v + row[i - 1] + 1) >> 2;
        }
        const int near = y >> 1;
        const int far = (y & 1) ? (near + 1 < ch ? near + 1 : ch - 1) : (near > 0 ? near - 1 : 0);
        const uint8_t* rn = c + (size_t)near * pw;
        const uint8_t* rf = c + (size_t)far * pw;
        const int sv = 3 * rn[i] + rf[i];
        if (x & 1) {
            const int o = i + 1 < cw ? 3 * rn[i + 1] + rf[i + 1] : sv;
            return (3 * sv + o + 7) >> 4;
        }
        const int o = i > 0 ? 3 * rn[i - 1] + rf[i - 1] : sv;
        return (3 * sv + o + 8) >> 4;
    }
};

// Row y of the image, chunk `chunk` of 4 * kT bytes of it.
__device__ __forceinline__ void colour_body(const Frame& f, const View& v, int y, uint32_t chunk) {
    const uint8_t *y_plane = v.p0, *cb_plane = v.p1, *cr_plane = v.p2;
    uint8_t* out = v.out;
    const int RB = f.W * f.comps;
    const int b0 = (int)(chunk * kT + threadIdx.x) * 4;
    if (b0 >= RB) return;
    uint32_t o[4] = {0, 0, 0, 0};
    if (f.comps == 1) {
        for (int i = 0; i < 4; ++i)
            if (b0 + i < RB) o[i] = y_plane[(size_t)y * f.pw[0] + b0 + i];
    } else {
        Chroma cb{cb_plane, f.pw[1], (f.W + f.hs - 1) / f.hs, (f.H + f.vs - 1) / f.vs, f.hs, f.vs};
        Chroma cr = cb;
        cr.c = cr_plane;
        const int x0 = b0 / 3;
        uint32_t px[6] = {0, 0, 0, 0, 0, 0};
        for (int j = 0; j < 2; ++j) {
            const int x = x0 + j;
            if (x >= f.W) break;
            const int Y = y_plane[(size_t)y * f.pw[0] + x], u = cb.at(y, x) - 128, v = cr.at(y, x) - 128;
            px[3 * j] = to_byte(Y + ((91881 * v + 32768) >> 16));
            px[3 * j + 1] = to_byte(Y + ((-22554 * u - 46802 * v + 32768) >> 16));
            px[3 * j + 2] = to_byte(Y + ((116130 * u + 32768) >> 16));
        }
        const int first = b0 - 3 * x0;
        for (int i = 0; i < 4; ++i) o[i] = px[first + i];
    }
    uint8_t* q = out + (size_t)y * RB + b0;
    if ((reinterpret_cast<uintptr_t>(q) & 3) == 0 && b0 + 4 <= RB) {
        *reinterpret_cast<uint32_t*>(q) = o[0] | (o[1] << 8) | (o[2] << 16) | (o[3] << 24);
    } else {
        for (int i = 0; i < 4; ++i)
            if (b0 + i < RB) q[i] = (uint8_t)o[i];
    }
}

__global__ void __launch_bounds__(kT) jpegdec_colour_kernel(Frame f, uint8_t* y_plane, uint8_t* cb_plane, uint8_t* cr_plane, uint8_t* out) {
    View v = {};
    v.p0 = y_plane; v.p1 = cb_plane; v.p2 = cr_plane; v.out = out;
    colour_body(f, v, (int)blockIdx.y, blockIdx.x);
}

// ---- the batch -------------------------------------------------------------------------------------------------------------------
// The image table as uploaded (scg_jpegdec.h): n records of SCG_JPEGDEC_IMAGE_WORDS, then the three prefix tables of n + 1 words.
constexpr int kRecSegment = 16, kRecHeaderAt = 18, kRecSegmentAt = 20, kRecOutAt = 22, kRecRegions = 24, kRegions = 10;
enum { kGridEntropy = 0, kGridIdct = 1, kGridColour = 2 };
enum { kRegCtl = 0, kRegEntry, kRegExit, kRegBnd, kRegCnt, kRegDcs, kRegCoef, kRegP0, kRegP1, kRegP2 };

struct Batch {
    const uint32_t* __restrict__ table;
    int n, rounds;                 // rounds: the sync launches of the call, one change counter each per image
    const uint8_t* upload;
    uint64_t upload_bytes;
    uint8_t* out;
    uint64_t out_bytes;
    char* ws;
    uint64_t ws_bytes;
};

// the bytes of the ten workspace regions of an image, in the order of the record (host: the plan; device: the bounds)
__host__ __device__ inline void region_bytes(const Frame& f, int rounds, uint64_t b[kRegions]) {
    b[kRegCtl] = 4ull * (uint64_t)rounds;
    b[kRegEntry] = b[kRegExit] = 8ull * f.nsub;
    b[kRegBnd] = 16ull * f.nwg;
    b[kRegCnt] = 4ull * f.nsub;
    b[kRegDcs] = 16ull * f.nsub;
    b[kRegCoef] = 128ull * f.nblocks;
    b[kRegP0] = (uint64_t)f.pw[0] * f.ph[0];
    b[kRegP1] = b[kRegP2] = f.comps == 3 ? (uint64_t)f.pw[1] * f.ph[1] : 0ull;
}

__host__ __device__ inline uint32_t groups_of(const Frame& f, int grid) {
    return grid == kGridEntropy ? f.nwg : (grid == kGridIdct ? idct_groups(f) : colour_chunks(f) * (uint32_t)f.H);
}

__device__ __forceinline__ uint64_t word64(const uint32_t* rec, int at) { return (uint64_t)rec[at] | ((uint64_t)rec[at + 1] << 32); }
__device__ __forceinline__ bool inside(uint64_t at, uint64_t bytes, uint64_t of) { return at <= of && bytes <= of - at; }

// The view of image `img` from the DEVICE table, every offset held to the sizes the kernel was passed: false for a record that
// names a byte outside a buffer (the host validated its own copy; a device copy that differs must not be followed).
__device__ __forceinline__ bool view_of_image(const Batch& a, int img, Frame* f, View* v) {
    const uint32_t* rec = a.table + (size_t)img * SCG_JPEGDEC_IMAGE_WORDS;
    if (frame_from(reinterpret_cast<const int32_t*>(rec), rec[kRecSegment], f) != 0) return false;
    const uint64_t hdr = word64(rec, kRecHeaderAt), seg = word64(rec, kRecSegmentAt), out = word64(rec, kRecOutAt);
    if ((hdr & 15u) || !inside(hdr, SCG_JPEGDEC_HEADER_BYTES, a.upload_bytes) || !inside(seg, f->nbytes, a.upload_bytes)) return false;
    if (!inside(out, (uint64_t)f->H * f->W * f->comps, a.out_bytes) || !inside(16ull * img, 16, a.ws_bytes)) return false;
    uint64_t need[kRegions], at[kRegions];
    region_bytes(*f, a.rounds, need);
    bool ok = true;
#pragma unroll
    for (int k = 0; k < kRegions; ++k) {
        at[k] = word64(rec, kRecRegions + 2 * k);
        ok = ok && (at[k] & 15u) == 0u && inside(at[k], need[k], a.ws_bytes);
    }
    if (!ok) return false;
    v->hdr = reinterpret_cast<const HeaderDev*>(a.upload + hdr);
    v->s = a.upload + seg;
    v->out = a.out + out;
    v->status = reinterpret_cast<uint32_t*>(a.ws) + 4 * (size_t)img;
    v->chg = reinterpret_cast<uint32_t*>(a.ws + at[kRegCtl]);
    v->entry = reinterpret_cast<uint64_t*>(a.ws + at[kRegEntry]);
    v->exit_ = reinterpret_cast<uint64_t*>(a.ws + at[kRegExit]);
    v->bnd = reinterpret_cast<uint64_t*>(a.ws + at[kRegBnd]);
    v->cnt = reinterpret_cast<uint32_t*>(a.ws + at[kRegCnt]);
    v->dcs = reinterpret_cast<int4*>(a.ws + at[kRegDcs]);
    v->coef = reinterpret_cast<int16_t*>(a.ws + at[kRegCoef]);
    v->p0 = reinterpret_cast<uint8_t*>(a.ws + at[kRegP0]);
    v->p1 = reinterpret_cast<uint8_t*>(a.ws + at[kRegP1]);
    v->p2 = reinterpret_cast<uint8_t*>(a.ws + at[kRegP2]);
    return true;
}

// A workgroup lies inside one image and finds it from blockIdx.x alone: the last image whose first workgroup in this grid is not
// behind g.  Uniform, so the table and the record come through scalar loads.  *local: the workgroup within the image's own grid.
// The frame goes to LDS (*shared, behind a barrier): the bodies index its table ids by component.
template <int kGrid>
__device__ __forceinline__ bool view_of_group(const Batch& a, uint32_t g, Frame* shared, View* v, uint32_t* local) {
    Frame f;
    const uint32_t* first = a.table + (size_t)a.n * SCG_JPEGDEC_IMAGE_WORDS + (size_t)kGrid * (a.n + 1);
    int lo = 0, hi = a.n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (first[mid] <= g) lo = mid; else hi = mid - 1;
    }
    if (g < first[lo] || !view_of_image(a, lo, &f, v)) return false;
    *local = g - first[lo];
    if (*local >= groups_of(f, kGrid)) return false;
    if (threadIdx.x == 0) *shared = f;
    __syncthreads();
    return true;
}

__global__ void __launch_bounds__(kT) jpegdec_batch_sync_kernel(Batch a, int round) {
    __shared__ Frame s_frame;
    View v;
    uint32_t g;
    if (!view_of_group<kGridEntropy>(a, blockIdx.x, &s_frame, &v, &g)) return;      // uniform: before any barrier
    sync_body(s_frame, v, g, round);
}

template <int kMode>
__global__ void __launch_bounds__(kT) jpegdec_batch_pass_kernel(Batch a) {
    __shared__ Frame s_frame;
    View v;
    uint32_t g;
    if (!view_of_group<kGridEntropy>(a, blockIdx.x, &s_frame, &v, &g)) return;
    pass_body<kMode>(s_frame, v, g);
}

// a workgroup per image; an image whose record cannot be followed reports that its states were never settled
__global__ void __launch_bounds__(kT) jpegdec_batch_scan_kernel(Batch a) {
    Frame f;
    View v;
    const int img = blockIdx.x;
    if (!view_of_image(a, img, &f, &v)) {
        if (threadIdx.x == 0 && inside(16ull * img, 16, a.ws_bytes))
            atomicOr(reinterpret_cast<uint32_t*>(a.ws) + 4 * (size_t)img, (uint32_t)(SCG_JPEGDEC_BAD_SYNC | SCG_JPEGDEC_BAD_COUNT));
        return;
    }
    scan_body(f, v, a.rounds);
}

__global__ void __launch_bounds__(kT) jpegdec_batch_idct_kernel(Batch a) {
    __shared__ Frame s_frame;
    View v;
    uint32_t g;
    if (!view_of_group<kGridIdct>(a, blockIdx.x, &s_frame, &v, &g)) return;
    idct_body(s_frame, v, g);
}

__global__ void __launch_bounds__(kT) jpegdec_batch_colour_kernel(Batch a) {
    __shared__ Frame s_frame;
    View v;
    uint32_t g;
    if (!view_of_group<kGridColour>(a, blockIdx.x, &s_frame, &v, &g)) return;
    const uint32_t chunks = colour_chunks(s_frame);
    colour_body(s_frame, v, (int)(g / chunks), g % chunks);
}

// ---- host ------------------------------------------------------------------------------------------------------------------------
// The sync launches after which every stream's states are right AND seen to be: workgroup g is right after launch g, one more
// launch shows that nothing changed; a single workgroup settles inside its first launch.  The one limit of sizes and decode.
inline uint32_t settle_rounds(uint32_t nwg) { return nwg == 1u ? 1u : nwg + 1u; }

int frame_of(const char* who, const int32_t* w, uint64_t segment_bytes, Frame* f, Layout* l) {
    if (!w) return g_err.fail(SCG_E_NULL, "%s: frame is NULL", who);
    const int why = frame_from(w, segment_bytes, f);
    const int c = why >> 8;
    switch (why & 255) {
        case 0: break;
        case kFrameDim: return g_err.fail(SCG_E_RANGE, "%s: a frame of %d x %d pixels (1..%d)", who, f->W, f->H, SCG_JPEGDEC_MAX_DIM);
        case kFrameComps: return g_err.fail(SCG_E_RANGE, "%s: %d components (1 or 3)", who, f->comps);
        case kFrameSampling:
            return g_err.fail(SCG_E_RANGE, "%s: sampling %d x %d (1x1; with three components also 2x1, 2x2)", who, f->hs, f->vs);
        case kFrameRestart: return g_err.fail(SCG_E_RANGE, "%s: restart interval %d (0..65535)", who, f->ri);
        case kFrameTables:
            return g_err.fail(SCG_E_RANGE, "%s: component %d names tables (%d, %d, %d): quant 0..3, Huffman 0..1", who, c, f->tq[c], f->td[c], f->ta[c]);
        case kFrameLast: return g_err.fail(SCG_E_RANGE, "%s: frame word 15 is %d, not 0", who, w[15]);
        case kFrameSegment:
            return g_err.fail(SCG_E_RANGE, "%s: a segment of %llu bytes (1..%d)", who, (unsigned long long)segment_bytes, SCG_JPEGDEC_MAX_SEGMENT);
        default:
            return g_err.fail(SCG_E_RANGE, "%s: %llu blocks are more than 2^26 - 1", who,
                              (unsigned long long)f->mcux * (unsigned long long)f->mcuy * (unsigned long long)f->bpm);
    }
    const uint64_t nblocks = f->nblocks;
    uint64_t at = 0;
    auto take = [&](uint64_t bytes) { const uint64_t o = at; at = align_to<256>(at + bytes); return o; };
    l->ctl = take(4ull * (kCtlWords + f->nwg + 1));
    l->entry = take(8ull * f->nsub);
    l->exit_ = take(8ull * f->nsub);
    l->bnd = take(16ull * f->nwg);
    l->cnt = take(4ull * f->nsub);
    l->dcs = take(16ull * f->nsub);
    l->coef_bytes = 128ull * nblocks;
    l->coef = take(l->coef_bytes);
    l->planes = take((uint64_t)f->pw[0] * f->ph[0]);
    l->plane1 = l->plane2 = l->planes;
    if (f->comps == 3) {
        l->plane1 = take((uint64_t)f->pw[1] * f->ph[1]);
        l->plane2 = take((uint64_t)f->pw[1] * f->ph[1]);
    }
    l->total = at;
    return 0;
}

// ---- the batch's plan ------------------------------------------------------------------------------------------------------------
// Workspace of a batch: [4 n status words | the change counters of every image] (ONE clear), then per image entry, exit, bnd, cnt,
// dcs and the planes, then every coefficient buffer (ONE clear).  Totals first, then the records in input order through `each`,
// so that scg_jpegdec_batch_plan (which writes them) and scg_jpegdec_decode_batch (which compares them) cannot disagree.
struct BatchTotals {
    uint64_t workspace, out, clear_bytes, coef_at, coef_bytes;
    uint32_t groups[3];
    int32_t max_rounds;
};

// inputs(i, v): v[0] the segment's bytes, v[1] the offset of the header block, v[2] of the segment in the upload.
template <class Inputs, class Each>
int batch_walk(const char* who, int32_t n, const int32_t* frames, Inputs&& inputs, uint64_t upload_bytes, BatchTotals* tot, Each&& each) {
    uint64_t in[3];
    Frame f;
    Layout l;
    uint64_t need[kRegions];
    uint32_t rounds = 1;
    for (int32_t i = 0; i < n; ++i) {
        inputs(i, in);
        const uint64_t header_at = in[1], segment_at = in[2];
        if (int rc = frame_of(who, frames + (size_t)i * SCG_JPEGDEC_FRAME_WORDS, in[0], &f, &l)) {
            char first[400];
            snprintf(first, sizeof(first), "%s", g_err.text);
            return g_err.fail(rc, "image %d: %s", i, first);
        }
        if (header_at % 16 || segment_at % 16)
            return g_err.fail(SCG_E_ALIGN, "%s: image %d: header block or segment not at a 16-byte offset of the upload", who, i);
        if (header_at > upload_bytes || SCG_JPEGDEC_HEADER_BYTES > upload_bytes - header_at)
            return g_err.fail(SCG_E_RANGE, "%s: image %d: the header block at %llu leaves the upload of %llu bytes", who, i,
                              (unsigned long long)header_at, (unsigned long long)upload_bytes);
        if (segment_at > upload_bytes || in[0] > upload_bytes - segment_at)
            return g_err.fail(SCG_E_RANGE, "%s: image %d: the segment at %llu leaves the upload of %llu bytes", who, i,
                              (unsigned long long)segment_at, (unsigned long long)upload_bytes);
        rounds = settle_rounds(f.nwg) > rounds ? settle_rounds(f.nwg) : rounds;
    }
    tot->max_rounds = (int32_t)rounds;
    const uint64_t counters = align_to<16>(4ull * rounds);
    tot->clear_bytes = 16ull * n + counters * n;
    uint64_t at = align_to<256>(tot->clear_bytes), coef = 0, out = 0, groups[3] = {0, 0, 0};
    auto take = [](uint64_t* cursor, uint64_t bytes) { const uint64_t o = *cursor; *cursor = align_to<256>(o + bytes); return o; };
    // (the coefficient buffers lie behind everything else: where they start is known only after this pass)
    for (int32_t i = 0; i < n; ++i) {
        inputs(i, in);
        frame_from(frames + (size_t)i * SCG_JPEGDEC_FRAME_WORDS, in[0], &f);
        region_bytes(f, (int)rounds, need);
        for (int k = kRegEntry; k < kRegions; ++k)
            if (k != kRegCoef) take(&at, need[k]);
    }
    tot->coef_at = at;
    uint64_t other = align_to<256>(tot->clear_bytes);
    for (int32_t i = 0; i < n; ++i) {
        inputs(i, in);
        frame_from(frames + (size_t)i * SCG_JPEGDEC_FRAME_WORDS, in[0], &f);
        region_bytes(f, (int)rounds, need);
        uint32_t rec[SCG_JPEGDEC_IMAGE_WORDS] = {};
        for (int k = 0; k < SCG_JPEGDEC_FRAME_WORDS; ++k) rec[k] = (uint32_t)frames[(size_t)i * SCG_JPEGDEC_FRAME_WORDS + k];
        rec[kRecSegment] = (uint32_t)in[0];
        auto put = [&](int word, uint64_t v) { rec[word] = (uint32_t)v; rec[word + 1] = (uint32_t)(v >> 32); };
        put(kRecHeaderAt, in[1]);
        put(kRecSegmentAt, in[2]);
        put(kRecOutAt, out);
        uint64_t where[kRegions];
        where[kRegCtl] = 16ull * n + counters * i;
        for (int k = kRegEntry; k <= kRegDcs; ++k) where[k] = take(&other, need[k]);
        where[kRegCoef] = tot->coef_at + take(&coef, need[kRegCoef]);
        where[kRegP0] = take(&other, need[kRegP0]);
        where[kRegP1] = where[kRegP2] = where[kRegP0];
        if (f.comps == 3) {
            where[kRegP1] = take(&other, need[kRegP1]);
            where[kRegP2] = take(&other, need[kRegP2]);
        }
        for (int k = 0; k < kRegions; ++k) put(kRecRegions + 2 * k, where[k]);
        uint32_t first[3];
        for (int k = 0; k < 3; ++k) {
            first[k] = (uint32_t)groups[k];
            groups[k] += groups_of(f, k);
            if (groups[k] > 0x7FFFFFFFull) return g_err.fail(SCG_E_RANGE, "%s: more than 2^31 - 1 workgroups in one grid at image %d", who, i);
        }
        if (int rc = each(i, rec, first, out)) return rc;
        out = align_to<16>(out + (uint64_t)f.H * f.W * f.comps);
    }
    tot->coef_bytes = coef;
    tot->workspace = tot->coef_at + coef;
    tot->out = out;
    for (int k = 0; k < 3; ++k) tot->groups[k] = (uint32_t)groups[k];
    return 0;
}

}  // namespace
}  // namespace scg

using namespace scg;

extern "C" {

const char* scg_jpegdec_last_error(void) { return g_err.text; }
int32_t scg_jpegdec_abi_version(void) { return SCG_JPEGDEC_ABI_VERSION; }

int scg_jpegdec_sizes(const int32_t* frame, uint64_t segment_bytes, uint64_t* workspace_bytes, uint64_t* out_bytes, int32_t* max_rounds) {
    const char* who = "scg_jpegdec_sizes";
    Frame f;
    Layout l;
    if (int rc = frame_of(who, frame, segment_bytes, &f, &l)) return rc;
    if (!workspace_bytes || !out_bytes || !max_rounds) return g_err.fail(SCG_E_NULL, "%s: an output is NULL", who);
    *workspace_bytes = l.total;
    *out_bytes = (uint64_t)f.H * f.W * f.comps;
    *max_rounds = (int32_t)settle_rounds(f.nwg);
    return 0;
}

int scg_jpegdec_decode(const int32_t* frame, const void* header_dev, const uint8_t* segment_dev, uint64_t segment_bytes, void* out,
                       size_t out_bytes, void* workspace, size_t workspace_bytes, int32_t rounds_done, int32_t rounds, void* stream) {
    const char* who = "scg_jpegdec_decode";
    Frame f;
    Layout l;
    if (int rc = frame_of(who, frame, segment_bytes, &f, &l)) return rc;
    if (int rc = g_err.check_ptr(who, header_dev, "header_dev", 16)) return rc;
    if (!segment_dev) return g_err.fail(SCG_E_NULL, "%s: segment_dev is NULL", who);
    if (int rc = g_err.check_ptr(who, out, "out", 16)) return rc;
    const uint64_t need = (uint64_t)f.H * f.W * f.comps;
    if (out_bytes < need) return g_err.fail(SCG_E_SCRATCH, "%s: out of %zu bytes < %llu", who, out_bytes, (unsigned long long)need);
    if (int rc = g_err.check_ptr(who, workspace, "workspace", 16)) return rc;
    if (workspace_bytes < l.total)
        return g_err.fail(SCG_E_SCRATCH, "%s: workspace of %zu bytes < %llu", who, workspace_bytes, (unsigned long long)l.total);
    if (rounds < 1) return g_err.fail(SCG_E_RANGE, "%s: rounds = %d (>= 1)", who, rounds);
    if (rounds_done < 0 || (uint64_t)rounds_done + (uint64_t)rounds > (uint64_t)settle_rounds(f.nwg))
        return g_err.fail(SCG_E_RANGE, "%s: rounds_done + rounds = %lld launches, more than the %u that settle every stream", who,
                          (long long)rounds_done + rounds, settle_rounds(f.nwg));

    hipStream_t st = static_cast<hipStream_t>(stream);
    char* ws = static_cast<char*>(workspace);
    uint32_t* ctl = reinterpret_cast<uint32_t*>(ws + l.ctl);
    uint64_t* entry = reinterpret_cast<uint64_t*>(ws + l.entry);
    uint64_t* exit_ = reinterpret_cast<uint64_t*>(ws + l.exit_);
    uint64_t* bnd = reinterpret_cast<uint64_t*>(ws + l.bnd);
    uint32_t* cnt = reinterpret_cast<uint32_t*>(ws + l.cnt);
    int4* dcs = reinterpret_cast<int4*>(ws + l.dcs);
    int16_t* coef = reinterpret_cast<int16_t*>(ws + l.coef);
    uint8_t* p0 = reinterpret_cast<uint8_t*>(ws + l.planes);
    uint8_t* p1 = reinterpret_cast<uint8_t*>(ws + l.plane1);
    uint8_t* p2 = reinterpret_cast<uint8_t*>(ws + l.plane2);
    const HeaderDev* hdr = static_cast<const HeaderDev*>(header_dev);

    // the status words always; the change counters only when a decode starts (a continued one keeps those of its earlier launches)
    const size_t ctl_bytes = rounds_done == 0 ? 4ull * (kCtlWords + f.nwg + 1) : 4ull * kCtlWords;
    if (int rc = g_err.check_hip(hipMemsetAsync(ctl, 0, ctl_bytes, st), "jpegdec clear status")) return rc;
    if (int rc = g_err.check_hip(hipMemsetAsync(coef, 0, l.coef_bytes, st), "jpegdec clear coefficients")) return rc;
    for (int k = rounds_done; k < rounds_done + rounds; ++k) {
        hipLaunchKernelGGL(jpegdec_sync_kernel, dim3(f.nwg), dim3(kT), 0, st, f, hdr, segment_dev, entry, exit_, bnd, ctl, k);
        if (int rc = g_err.check_hip(hipGetLastError(), "jpegdec_sync")) return rc;
    }
    hipLaunchKernelGGL(jpegdec_pass_kernel<1>, dim3(f.nwg), dim3(kT), 0, st, f, hdr, segment_dev, exit_, cnt, dcs, coef, ctl);
    if (int rc = g_err.check_hip(hipGetLastError(), "jpegdec_count")) return rc;
    hipLaunchKernelGGL(jpegdec_scan_kernel, dim3(1), dim3(kT), 0, st, f, cnt, dcs, ctl, rounds_done + rounds);
    if (int rc = g_err.check_hip(hipGetLastError(), "jpegdec_scan")) return rc;
    hipLaunchKernelGGL(jpegdec_pass_kernel<2>, dim3(f.nwg), dim3(kT), 0, st, f, hdr, segment_dev, exit_, cnt, dcs, coef, ctl);
    if (int rc = g_err.check_hip(hipGetLastError(), "jpegdec_write")) return rc;
    hipLaunchKernelGGL(jpegdec_idct_kernel, dim3((f.nblocks + kIdctBlocks - 1) / kIdctBlocks), dim3(kT), 0, st, f, hdr, coef, p0, p1, p2);
    if (int rc = g_err.check_hip(hipGetLastError(), "jpegdec_idct")) return rc;
    hipLaunchKernelGGL(jpegdec_colour_kernel, dim3((unsigned)((f.W * f.comps + 4 * kT - 1) / (4 * kT)), (unsigned)f.H), dim3(kT), 0, st, f, p0,
                       p1, p2, static_cast<uint8_t*>(out));
    return g_err.check_hip(hipGetLastError(), "jpegdec_colour");
}

int scg_jpegdec_batch_plan(int32_t n, const int32_t* frames, const uint64_t* segment_bytes, const uint64_t* header_offsets,
                           const uint64_t* segment_offsets, uint64_t upload_bytes, uint32_t* table, uint64_t table_words,
                           uint64_t* out_offsets, uint64_t* workspace_bytes, uint64_t* out_bytes, int32_t* max_rounds) {
    const char* who = "scg_jpegdec_batch_plan";
    if (n < 1 || n > SCG_JPEGDEC_MAX_BATCH) return g_err.fail(SCG_E_RANGE, "%s: n = %d images (1..%d)", who, n, SCG_JPEGDEC_MAX_BATCH);
    if (!frames || !segment_bytes || !header_offsets || !segment_offsets) return g_err.fail(SCG_E_NULL, "%s: an input table is NULL", who);
    if (!table || !out_offsets || !workspace_bytes || !out_bytes || !max_rounds) return g_err.fail(SCG_E_NULL, "%s: an output is NULL", who);
    if (table_words < (uint64_t)n * SCG_JPEGDEC_IMAGE_WORDS + 3ull * (n + 1))
        return g_err.fail(SCG_E_SCRATCH, "%s: a table of %llu words < %llu", who, (unsigned long long)table_words,
                          (unsigned long long)n * SCG_JPEGDEC_IMAGE_WORDS + 3ull * (n + 1));
    BatchTotals tot;
    uint32_t* prefix = table + (size_t)n * SCG_JPEGDEC_IMAGE_WORDS;
    if (int rc = batch_walk(who, n, frames,
                            [&](int32_t i, uint64_t v[3]) { v[0] = segment_bytes[i]; v[1] = header_offsets[i]; v[2] = segment_offsets[i]; },
                            upload_bytes, &tot,
                            [&](int32_t i, const uint32_t* rec, const uint32_t* first, uint64_t out_at) {
                                memcpy(table + (size_t)i * SCG_JPEGDEC_IMAGE_WORDS, rec, 4 * SCG_JPEGDEC_IMAGE_WORDS);
                                for (int k = 0; k < 3; ++k) prefix[(size_t)k * (n + 1) + i] = first[k];
                                out_offsets[i] = out_at;
                                return 0;
                            }))
        return rc;
    for (int k = 0; k < 3; ++k) prefix[(size_t)k * (n + 1) + n] = tot.groups[k];
    *workspace_bytes = tot.workspace;
    *out_bytes = tot.out;
    *max_rounds = tot.max_rounds;
    return 0;
}

int scg_jpegdec_decode_batch(int32_t n, const int32_t* frames, const uint32_t* table, const void* table_dev, const void* upload_dev,
                             uint64_t upload_bytes, void* out, size_t out_bytes, void* workspace, size_t workspace_bytes, int32_t rounds,
                             void* stream) {
    const char* who = "scg_jpegdec_decode_batch";
    if (n < 1 || n > SCG_JPEGDEC_MAX_BATCH) return g_err.fail(SCG_E_RANGE, "%s: n = %d images (1..%d)", who, n, SCG_JPEGDEC_MAX_BATCH);
    if (!frames || !table) return g_err.fail(SCG_E_NULL, "%s: frames or table is NULL", who);
    // what the plan was given, read back from the host table; the walk then produces every record again and compares
    BatchTotals tot = {};
    const uint32_t* prefix = table + (size_t)n * SCG_JPEGDEC_IMAGE_WORDS;
    auto same = [&](int32_t i, const uint32_t* rec, const uint32_t* first, uint64_t) {
        bool eq = memcmp(table + (size_t)i * SCG_JPEGDEC_IMAGE_WORDS, rec, 4 * SCG_JPEGDEC_IMAGE_WORDS) == 0;
        for (int k = 0; k < 3; ++k) eq = eq && prefix[(size_t)k * (n + 1) + i] == first[k];
        return eq ? 0 : g_err.fail(SCG_E_RANGE, "%s: the record or a prefix entry of image %d is not what scg_jpegdec_batch_plan gives", who, i);
    };
    auto from_table = [&](int32_t i, uint64_t v[3]) {
        const uint32_t* rec = table + (size_t)i * SCG_JPEGDEC_IMAGE_WORDS;
        v[0] = rec[kRecSegment];
        v[1] = (uint64_t)rec[kRecHeaderAt] | ((uint64_t)rec[kRecHeaderAt + 1] << 32);
        v[2] = (uint64_t)rec[kRecSegmentAt] | ((uint64_t)rec[kRecSegmentAt + 1] << 32);
    };
    if (int rc = batch_walk(who, n, frames, from_table, upload_bytes, &tot, same)) return rc;
    for (int k = 0; k < 3; ++k)
        if (prefix[(size_t)k * (n + 1) + n] != tot.groups[k])
            return g_err.fail(SCG_E_RANGE, "%s: the last entry of prefix table %d is not what scg_jpegdec_batch_plan gives", who, k);
    if (int e = g_err.check_ptr(who, table_dev, "table_dev", 16)) return e;
    if (int e = g_err.check_ptr(who, upload_dev, "upload_dev", 16)) return e;
    if (int e = g_err.check_ptr(who, out, "out", 16)) return e;
    if (out_bytes < tot.out) return g_err.fail(SCG_E_SCRATCH, "%s: out of %zu bytes < %llu", who, out_bytes, (unsigned long long)tot.out);
    if (int e = g_err.check_ptr(who, workspace, "workspace", 16)) return e;
    if (workspace_bytes < tot.workspace)
        return g_err.fail(SCG_E_SCRATCH, "%s: workspace of %zu bytes < %llu", who, workspace_bytes, (unsigned long long)tot.workspace);
    if (rounds < 1 || rounds > tot.max_rounds)
        return g_err.fail(SCG_E_RANGE, "%s: rounds = %d (1..%d, the launches that settle every stream of the batch)", who, rounds, tot.max_rounds);

    hipStream_t st = static_cast<hipStream_t>(stream);
    Batch a;
    a.table = static_cast<const uint32_t*>(table_dev);
    a.n = n;
    a.rounds = rounds;
    a.upload = static_cast<const uint8_t*>(upload_dev);
    a.upload_bytes = upload_bytes;
    a.out = static_cast<uint8_t*>(out);
    a.out_bytes = out_bytes;
    a.ws = static_cast<char*>(workspace);
    a.ws_bytes = workspace_bytes;
    if (int e = g_err.check_hip(hipMemsetAsync(a.ws, 0, tot.clear_bytes, st), "jpegdec batch clear status")) return e;
    if (int e = g_err.check_hip(hipMemsetAsync(a.ws + tot.coef_at, 0, tot.coef_bytes, st), "jpegdec batch clear coefficients")) return e;
    for (int k = 0; k < rounds; ++k) {
        hipLaunchKernelGGL(jpegdec_batch_sync_kernel, dim3(tot.groups[kGridEntropy]), dim3(kT), 0, st, a, k);
        if (int e = g_err.check_hip(hipGetLastError(), "jpegdec_batch_sync")) return e;
    }
    hipLaunchKernelGGL(jpegdec_batch_pass_kernel<1>, dim3(tot.groups[kGridEntropy]), dim3(kT), 0, st, a);
    if (int e = g_err.check_hip(hipGetLastError(), "jpegdec_batch_count")) return e;
    hipLaunchKernelGGL(jpegdec_batch_scan_kernel, dim3((unsigned)n), dim3(kT), 0, st, a);
    if (int e = g_err.check_hip(hipGetLastError(), "jpegdec_batch_scan")) return e;
    hipLaunchKernelGGL(jpegdec_batch_pass_kernel<2>, dim3(tot.groups[kGridEntropy]), dim3(kT), 0, st, a);
    if (int e = g_err.check_hip(hipGetLastError(), "jpegdec_batch_write")) return e;
    hipLaunchKernelGGL(jpegdec_batch_idct_kernel, dim3(tot.groups[kGridIdct]), dim3(kT), 0, st, a);
    if (int e = g_err.check_hip(hipGetLastError(), "jpegdec_batch_idct")) return e;
    hipLaunchKernelGGL(jpegdec_batch_colour_kernel, dim3(tot.groups[kGridColour]), dim3(kT), 0, st, a);
    return g_err.check_hip(hipGetLastError(), "jpegdec_batch_colour");
}

}  // extern "C"

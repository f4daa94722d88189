// pngpack.hip — libscg_png.so: the zlib streams of PNG files packed on the GPU (include/png/scg_png.h states the stream; it is the
// contract, and tests/png_refs.py restates it in numpy).
//
// A PNG is a re-layout (the filter), a histogram and a bit pack; except for a chunk's code table every byte is decided from a few
// neighbours.  A batch of any number of images of unequal sizes is three launches over the FLAT list of all images' 32 KiB chunks:
//
//   png_count_kernel   a workgroup per chunk.  The filtered bytes go to LDS (a row of 33 dwords per thread's 32: the odd stride
//                      puts the lanes' own segments on distinct banks).  A thread owns 128 consecutive bytes: the run starts of
//                      its segment are a 128-bit mask, the nearest start before and after the segment come from a workgroup max /
//                      min scan, so every token follows from its position, its run's start and its run's length
//                      (for_each_token).  Histogram and Adler sums through LDS atomics; the code in the same workgroup: a bitonic
//                      sort of 512 (frequency, symbol) keys, the two-queue merge by one lane, the depth counts, miniz's repair.
//   png_scan_kernel    ONE workgroup: the blocks' byte offsets (compact.h carry_scan), the images' streams back to back at
//                      multiples of 16, the zlib header and the Adler-32 of every image, the table.
//   png_encode_kernel  a workgroup per chunk: the same bytes and tokens by the same functions, canonical codes, an exclusive scan of
//                      the threads' bit counts, the bits ORed into a zeroed LDS window of the block (16 KiB at a time, so that
//                      LDS stays under 64 KiB and two workgroups fit a compute unit), the window written out: whole dwords where
//                      all four bytes are this block's, single bytes at the edges.
//
// No workgroup waits for another, nothing is allocated, nothing is read back; the same input gives the same bytes.
#include "../../include/png/scg_png.h"
#include "bitwindow.h"
#include "compact.h"
#include "host_align.h"
#include "host_error.h"

namespace scg {
namespace {

constexpr int kT = SCG_PNG_THREADS;
constexpr int kChunk = SCG_PNG_CHUNK;
constexpr int kSeg = kChunk / kT;                  // 128 bytes of the chunk per thread
constexpr int kSegWords = kSeg / 4;                // 32
constexpr int kRowWords = kSegWords + 1;           // 33: the odd stride
constexpr int kDataWords = kT * kRowWords;         // 33 792 bytes
constexpr int kSyms = SCG_PNG_SYMBOLS;
constexpr int kLens = SCG_PNG_LENGTHS;
constexpr int kKeys = 512;
constexpr int kMaxBits = SCG_PNG_MAX_CODE_BITS;
constexpr int kEob = 256;
constexpr uint32_t kMod = 65521u;
constexpr int kWinWords = 4096;                    // the encode kernel's LDS window of the block: 16 KiB
static_assert(kT == kBlock && kSeg == 128 && kKeys == 2 * kT && kKeys >= kSyms, "a 128-bit start mask per thread, a key pair per thread");

thread_local ErrorText g_err = {};

struct PngArgs {
    int images, chunks, filter, gray_as_rgb;
    const ScgPngImage* img;
    const ScgPngChunk* chunk;
    uint8_t* lengths;
    ScgPngChunkInfo* info;
    uint32_t* base;
    uint32_t* ioff;
    uint32_t* table;
    uint8_t* out;
    uint64_t capacity;
};

// ---- the filtered bytes ----------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int daddr(int p) { return p + ((p >> 7) << 2); }       // byte p of the chunk in the padded LDS rows
__device__ __forceinline__ uint32_t dbyte(const uint32_t* s_data, int p) {
    return reinterpret_cast<const uint8_t*>(s_data)[daddr(p)];
}

struct Source {
    const uint8_t* src;
    int W, bpp, row;            // row: bytes of a stream row, the filter byte included
    bool expand;                // one channel written as three
    __device__ __forceinline__ uint32_t at(int y, int xb) const {                  // byte xb of pixel row y; 0 outside
        if (y < 0 || xb < 0) return 0u;
        return expand ? src[(int64_t)y * W + xb / 3] : src[(int64_t)y * (row - 1) + xb];
    }
};

__device__ __forceinline__ uint32_t paeth(uint32_t a, uint32_t b, uint32_t c) {
    const int p = (int)a + (int)b - (int)c;
    const int pa = abs(p - (int)a), pb = abs(p - (int)b), pc = abs(p - (int)c);
    return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}

__device__ __forceinline__ uint32_t filtered(const Source& s, int filter, int y, int x) {       // x: byte of the stream row
    if (x == 0) return (uint32_t)filter;
    const int xb = x - 1;
    const uint32_t cur = s.at(y, xb);
    switch (filter) {
        case SCG_PNG_FILTER_SUB: return (cur - s.at(y, xb - s.bpp)) & 255u;
        case SCG_PNG_FILTER_UP: return (cur - s.at(y - 1, xb)) & 255u;
        case SCG_PNG_FILTER_PAETH: return (cur - paeth(s.at(y, xb - s.bpp), s.at(y - 1, xb), s.at(y - 1, xb - s.bpp))) & 255u;
        default: return cur;
    }
}

// The chunk's n filtered bytes into s_data; returns n.  A thread forms four consecutive bytes and stores one dword.
__device__ int load_filtered(uint32_t* s_data, const ScgPngImage& im, int index, int filter, int gray_as_rgb) {
    Source s;
    s.src = reinterpret_cast<const uint8_t*>(im.src);
    s.W = im.W;
    s.bpp = (im.channels == 3 || gray_as_rgb) ? 3 : 1;
    s.row = 1 + im.W * s.bpp;
    s.expand = im.channels == 1 && s.bpp == 3;
    const int64_t begin = (int64_t)index * kChunk;
    const int64_t left = (int64_t)im.stream_bytes - begin;
    const int n = left < kChunk ? (int)left : kChunk;
    for (int p0 = 4 * (int)threadIdx.x; p0 < n; p0 += 4 * kT) {
        const int64_t g = begin + p0;
        int y = (int)g / s.row, x = (int)g - y * s.row;                         // S < 2^31
        uint32_t word = 0u;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (p0 + k < n) word |= filtered(s, filter, y, x) << (8 * k);
            if (++x == s.row) { x = 0; ++y; }
        }
        s_data[daddr(p0) >> 2] = word;
    }
    return n;
}

// ---- runs and tokens -------------------------------------------------------------------------------------------------------------
struct Segment {
    int lo, hi;                 // this thread's bytes of the chunk
    int prev_start;             // the nearest run start before lo
    int next_start;             // the nearest run start at or behind hi (n when there is none)
    uint64_t m0, m1;            // bit i: byte lo + i starts a run
};

// Every thread of the workgroup calls it, after a barrier behind load_filtered.  s_scan: 8 ints of LDS.
__device__ Segment analyse_runs(const uint32_t* s_data, int n, int* s_scan) {
    Segment g;
    const int t = threadIdx.x, lane = lane_id(), w = wave_id();
    g.lo = t * kSeg < n ? t * kSeg : n;
    g.hi = g.lo + kSeg < n ? g.lo + kSeg : n;
    g.m0 = g.m1 = 0ull;
    uint32_t pb = g.lo > 0 && g.lo < n ? dbyte(s_data, g.lo - 1) : 256u;        // 256: equal to no byte, so byte 0 starts a run
    for (int k = 0; k < kSegWords && g.lo + 4 * k < g.hi; ++k) {
        const uint32_t word = s_data[t * kRowWords + k];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int i = 4 * k + j;
            const uint32_t b = (word >> (8 * j)) & 255u;
            if (g.lo + i < g.hi && b != pb) {
                if (i < 64) g.m0 |= 1ull << i; else g.m1 |= 1ull << (i - 64);
            }
            pb = b;
        }
    }
    const bool any = (g.m0 | g.m1) != 0ull;
    int last = -1, first = n;
    if (any) {
        first = g.lo + (g.m0 ? __ffsll((unsigned long long)g.m0) - 1 : 64 + __ffsll((unsigned long long)g.m1) - 1);
        last = g.lo + (g.m1 ? 127 - __clzll((long long)g.m1) : 63 - __clzll((long long)g.m0));
    }
    int mx = last, mn = first;                                                   // inclusive scans inside the wave
    for (int off = 1; off < kWave; off <<= 1) {
        const int a = __shfl_up(mx, off, kWave), b = __shfl_down(mn, off, kWave);
        if (lane >= off) mx = max(mx, a);
        if (lane + off < kWave) mn = min(mn, b);
    }
    if (lane == kWave - 1) s_scan[w] = mx;
    if (lane == 0) s_scan[4 + w] = mn;
    int ex_mx = __shfl_up(mx, 1, kWave), ex_mn = __shfl_down(mn, 1, kWave);
    if (lane == 0) ex_mx = -1;
    if (lane == kWave - 1) ex_mn = n;
    __syncthreads();
    for (int j = 0; j < kT / kWave; ++j) {
        if (j < w) ex_mx = max(ex_mx, s_scan[j]);
        if (j > w) ex_mn = min(ex_mn, s_scan[4 + j]);
    }
    g.prev_start = ex_mx;
    g.next_start = ex_mn;
    return g;
}

// Length 3..258 -> its symbol, the number of extra bits and their value (RFC 1951 3.2.5).
__device__ __forceinline__ int length_symbol(int len, int& ebits, int& eval) {
    ebits = eval = 0;
    if (len == 258) return 285;
    const int l = len - 3;
    if (l < 8) return 257 + l;
    const int e = 29 - __clz(l);                     // floor(log2 l) - 2
    ebits = e;
    eval = l & ((1 << e) - 1);
    return 261 + 4 * e + ((l >> e) & 3);
}
__device__ __forceinline__ int symbol_extra_bits(int sym) { return (sym < 265 || sym == 285) ? 0 : (sym - 261) >> 2; }

// The tokens whose FIRST byte lies in [a, b) of the run [s, e) of value v, in stream order.
template <class F>
__device__ __forceinline__ void run_tokens(int s, int e, int a, int b, uint32_t v, F& f) {
    const int len = e - s;
    if (len < 4) {
        for (int p = a; p < b; ++p) f.lit(v);
        return;
    }
    if (a == s) f.lit(v);
    const int m = len - 1, full = m / 258, r = m - full * 258;
    for (int k = a > s + 1 ? (a - s - 1 + 257) / 258 : 0; k < full && s + 1 + 258 * k < b; ++k) f.match(258);
    const int pr = s + 1 + 258 * full;
    if (r >= 3) {
        if (pr >= a && pr < b) f.match(r);
    } else {
        for (int p = max(pr, a); p < min(pr + r, b); ++p) f.lit(v);
    }
}

// Every token that begins in the thread's segment, in stream order.
template <class F>
__device__ __forceinline__ void for_each_token(const Segment& g, const uint32_t* s_data, F& f) {
    if (g.lo >= g.hi) return;
    uint64_t m0 = g.m0, m1 = g.m1;
    int s = g.prev_start;
    if (m0 & 1ull) {
        s = g.lo;
        m0 &= ~1ull;
    }
    for (;;) {
        int e = g.next_start;
        if (m0) {
            e = g.lo + __ffsll((unsigned long long)m0) - 1;
            m0 &= m0 - 1ull;
        } else if (m1) {
            e = g.lo + 64 + __ffsll((unsigned long long)m1) - 1;
            m1 &= m1 - 1ull;
        }
        const int a = s > g.lo ? s : g.lo, b = e < g.hi ? e : g.hi;
        run_tokens(s, e, a, b, dbyte(s_data, a), f);
        if (e >= g.hi) break;
        s = e;
    }
}

struct HistTokens {
    uint32_t* hist;
    __device__ __forceinline__ void lit(uint32_t v) { atomicAdd(&hist[v], 1u); }
    __device__ __forceinline__ void match(int len) {
        int eb, ev;
        atomicAdd(&hist[length_symbol(len, eb, ev)], 1u);
    }
};

// ---- launch 1: count -------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kT) void png_count_kernel(PngArgs a) {
    __shared__ uint32_t s_data[kDataWords];
    __shared__ uint32_t s_hist[kLens];
    __shared__ uint32_t s_keys[kKeys];
    __shared__ uint32_t s_wt[2 * kSyms];              // the tree: leaves in sorted order, then the merged nodes in creation order
    __shared__ uint16_t s_par[2 * kSyms], s_dep[2 * kSyms];
    __shared__ uint32_t s_cnt[kMaxBits + 2], s_cum[kMaxBits + 2];
    __shared__ uint8_t s_len[kLens];
    __shared__ unsigned long long s_sum[2];
    __shared__ uint32_t s_used, s_bits;
    __shared__ int s_scan[8];

    const int c = blockIdx.x, t = threadIdx.x;
    if (c >= a.chunks) return;
    const ScgPngChunk ck = a.chunk[c];
    if (ck.image < 0 || ck.image >= a.images) return;
    const ScgPngImage im = a.img[ck.image];
    if (ck.index < 0 || ck.index >= im.chunks) return;

    for (int i = t; i < kLens; i += kT) {
        s_hist[i] = i == kEob ? 1u : 0u;
        s_len[i] = i >= kSyms ? 1 : 0;                // the two distance codes
    }
    if (t < kMaxBits + 2) s_cnt[t] = 0u;
    if (t == 0) {
        s_sum[0] = s_sum[1] = 0ull;
        s_used = s_bits = 0u;
    }
    const int n = load_filtered(s_data, im, ck.index, a.filter, a.gray_as_rgb);
    __syncthreads();
    const Segment g = analyse_runs(s_data, n, s_scan);

    HistTokens h{s_hist};
    for_each_token(g, s_data, h);
    unsigned long long sa = 0ull, sb = 0ull;          // Adler: sum d[i] and sum (n - i) d[i]; the second exceeds 32 bits
    for (int p = g.lo; p < g.hi; ++p) {
        const uint32_t d = dbyte(s_data, p);
        sa += d;
        sb += (unsigned long long)(n - p) * d;
    }
    if (sa) {
        atomicAdd(&s_sum[0], sa);
        atomicAdd(&s_sum[1], sb);
    }
    __syncthreads();

    // 1. the used symbols by (frequency, symbol): a bitonic sort of 512 keys, the unused ones behind
    for (int i = t; i < kKeys; i += kT) {
        const uint32_t f = i < kSyms ? s_hist[i] : 0u;
        s_keys[i] = f ? (f << 9) | (uint32_t)i : 0xFFFFFFFFu;
        if (f) atomicAdd(&s_used, 1u);
    }
    __syncthreads();
    for (int k = 2; k <= kKeys; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            const int lo = ((t & ~(j - 1)) << 1) | (t & (j - 1)), hi = lo | j;
            const uint32_t x = s_keys[lo], y = s_keys[hi];
            if ((x > y) == ((lo & k) == 0)) {
                s_keys[lo] = y;
                s_keys[hi] = x;
            }
            __syncthreads();
        }
    const int used = (int)s_used;                     // >= 2: end-of-block and at least one literal

    // 2. the two-queue merge, one lane: leaves 0 .. used-1, merged nodes used .. 2 used - 2; the leaf on a tie
    for (int i = t; i < used; i += kT) s_wt[i] = s_keys[i] >> 9;
    __syncthreads();
    if (t == 0) {
        int li = 0, ni = used, next = used;
        for (int k = 0; k < used - 1; ++k) {
            int pick[2];
#pragma unroll
            for (int q = 0; q < 2; ++q) pick[q] = (li < used && (ni >= next || s_wt[li] <= s_wt[ni])) ? li++ : ni++;
            s_wt[next] = s_wt[pick[0]] + s_wt[pick[1]];
            s_par[pick[0]] = s_par[pick[1]] = (uint16_t)next;
            ++next;
        }
        s_dep[2 * used - 2] = 0;
        for (int k = 2 * used - 3; k >= used; --k) s_dep[k] = (uint16_t)(s_dep[s_par[k]] + 1);
    }
    __syncthreads();
    // 3. leaves per depth, 4. those beyond 15 counted at 15
    for (int i = t; i < used; i += kT) {
        const int d = s_dep[s_par[i]] + 1;
        atomicAdd(&s_cnt[d < kMaxBits ? d : kMaxBits], 1u);
    }
    __syncthreads();
    if (t == 0) {
        uint32_t total = 0u;
        for (int l = kMaxBits; l > 0; --l) total += s_cnt[l] << (kMaxBits - l);
        while (total != (1u << kMaxBits)) {           // miniz's repair: each round lowers the Kraft sum by one unit of 2^-15
            s_cnt[kMaxBits]--;
            for (int l = kMaxBits - 1; l > 0; --l)
                if (s_cnt[l]) {
                    s_cnt[l]--;
                    s_cnt[l + 1] += 2u;
                    break;
                }
            total--;
        }
        uint32_t cum = 0u;
        s_cum[0] = 0u;
        for (int l = 1; l <= kMaxBits; ++l) s_cum[l] = (cum += s_cnt[l]);
    }
    __syncthreads();
    // 5. the r-th most frequent symbol gets the first length whose cumulated count exceeds r
    for (int i = t; i < used; i += kT) {
        const uint32_t r = (uint32_t)(used - 1 - i);
        int l = 1;
        while (l < kMaxBits && s_cum[l] <= r) ++l;
        s_len[s_keys[i] & 511u] = (uint8_t)l;
    }
    __syncthreads();
    for (int i = t; i < kSyms; i += kT)
        if (s_hist[i]) atomicAdd(&s_bits, s_hist[i] * ((uint32_t)s_len[i] + (uint32_t)symbol_extra_bits(i) + (i > kEob ? 1u : 0u)));
    __syncthreads();

    for (int i = t; i < kLens; i += kT) a.lengths[(int64_t)c * kLens + i] = s_len[i];
    if (t == 0) {
        const bool final = ck.index == im.chunks - 1;
        const uint32_t bits = SCG_PNG_HEADER_BITS + s_bits;
        const uint32_t dyn = final ? (bits + 7u) >> 3 : ((bits + 3u + 7u) >> 3) + 4u;
        ScgPngChunkInfo o;
        o.kind = dyn >= (uint32_t)n + 5u ? SCG_PNG_KIND_STORED : SCG_PNG_KIND_DYNAMIC;
        o.bytes = o.kind == SCG_PNG_KIND_STORED ? (uint32_t)n + 5u : dyn;
        o.sum_a = (uint32_t)(s_sum[0] % kMod);
        o.sum_b = (uint32_t)(s_sum[1] % kMod);
        a.info[c] = o;
    }
}

// ---- launch 2: scan --------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kT) void png_scan_kernel(PngArgs a) {
    const int t = threadIdx.x;
    uint32_t total[1];
    for (int c = t; c < a.chunks; c += kT) a.base[c] = a.info[c].bytes;
    __syncthreads();
    carry_scan<1, kT>(a.base, a.chunks, total);
    if (t == 0) a.base[a.chunks] = total[0];
    __syncthreads();
    for (int i = t; i < a.images; i += kT) {
        const ScgPngImage im = a.img[i];
        const uint32_t raw = a.base[im.first_chunk + im.chunks] - a.base[im.first_chunk];
        a.table[2 * i + 1] = raw + 6u;
        a.ioff[i] = (raw + 6u + (SCG_PNG_ALIGN - 1u)) & ~(uint32_t)(SCG_PNG_ALIGN - 1u);
    }
    __syncthreads();
    carry_scan<1, kT>(a.ioff, a.images, total);
    if (t == 0) {
        a.table[2 * a.images] = total[0];
        a.table[2 * a.images + 1] = (uint32_t)a.images;
    }
    for (int i = t; i < a.images; i += kT) {
        const ScgPngImage im = a.img[i];
        const uint32_t off = a.ioff[i], bytes = a.table[2 * i + 1];
        a.table[2 * i] = off;
        if ((uint64_t)off + bytes > a.capacity) continue;            // cannot happen with the validated tables
        uint64_t s1 = 1u, s2 = 0u;                                   // Adler-32 from the chunks' partial sums, exact modulo 65521
        for (int k = 0; k < im.chunks; ++k) {
            const ScgPngChunkInfo o = a.info[im.first_chunk + k];
            const int64_t left = (int64_t)im.stream_bytes - (int64_t)k * kChunk;
            const uint64_t n = left < kChunk ? (uint64_t)left : (uint64_t)kChunk;
            s2 = (s2 + (n % kMod) * s1 + o.sum_b) % kMod;
            s1 = (s1 + o.sum_a) % kMod;
        }
        uint8_t* p = a.out + off;
        p[0] = 0x78;
        p[1] = 0x01;
        p += bytes - 4u;
        p[0] = (uint8_t)(s2 >> 8);
        p[1] = (uint8_t)s2;
        p[2] = (uint8_t)(s1 >> 8);
        p[3] = (uint8_t)s1;
    }
}

// ---- launch 3: encode ------------------------------------------------------------------------------------------------------------
struct Window {
    uint32_t* img;
    uint32_t wlo, whi;          // the words of the block that the LDS image holds
    __device__ __forceinline__ void put(uint32_t bitpos, uint32_t val) const {         // val: at most 21 bits, the first one lowest
        const uint64_t v = (uint64_t)val << (bitpos & 31u);
        window_or(img, wlo, whi, bitpos >> 5, (uint32_t)v, (uint32_t)(v >> 32));
    }
};

struct BitTokens {                                  // the bits of a thread's tokens
    const uint32_t* code;       // per symbol: the bit-reversed code, its length << 16
    uint32_t bits;
    __device__ __forceinline__ void lit(uint32_t v) { bits += code[v] >> 16; }
    __device__ __forceinline__ void match(int len) {
        int eb, ev;
        bits += (code[length_symbol(len, eb, ev)] >> 16) + (uint32_t)eb + 1u;
    }
};

struct PutTokens {
    const uint32_t* code;
    Window win;
    uint32_t at;
    __device__ __forceinline__ void lit(uint32_t v) {
        const uint32_t cd = code[v];
        win.put(at, cd & 0xFFFFu);
        at += cd >> 16;
    }
    __device__ __forceinline__ void match(int len) {
        int eb, ev;
        const uint32_t cd = code[length_symbol(len, eb, ev)];
        const int cl = (int)(cd >> 16);
        win.put(at, (cd & 0xFFFFu) | ((uint32_t)ev << cl));         // the distance code is the single bit 0
        at += (uint32_t)(cl + eb + 1);
    }
};

// Bytes [b0, b1) of the block that starts at byte `off` of out: dwords where all four bytes are the block's, else single bytes.
template <class G>
__device__ __forceinline__ void write_bytes(uint8_t* out, uint64_t off, uint32_t b0, uint32_t b1, const G& get) {
    const uint64_t g0 = off + b0, g1 = off + b1;
    for (uint64_t g = (g0 & ~(uint64_t)3u) + 4u * threadIdx.x; g < g1; g += 4u * kT) {
        if (g >= g0 && g + 4u <= g1) {
            const uint32_t k = (uint32_t)(g - off);
            *reinterpret_cast<uint32_t*>(out + g) = get(k) | (get(k + 1u) << 8) | (get(k + 2u) << 16) | (get(k + 3u) << 24);
        } else {
            for (uint64_t q = g; q < g + 4u; ++q)
                if (q >= g0 && q < g1) out[q] = (uint8_t)get((uint32_t)(q - off));
        }
    }
}

__global__ __launch_bounds__(kT) void png_encode_kernel(PngArgs a) {
    __shared__ uint32_t s_data[kDataWords];
    __shared__ uint32_t s_img[kWinWords];
    __shared__ uint32_t s_code[kLens];
    __shared__ uint8_t s_len[kLens];
    __shared__ uint32_t s_cnt[kMaxBits + 2], s_next[kMaxBits + 2];
    __shared__ uint32_t s_wave[kT / kWave];
    __shared__ int s_scan[8];

    const int c = blockIdx.x, t = threadIdx.x;
    if (c >= a.chunks) return;
    const ScgPngChunk ck = a.chunk[c];
    if (ck.image < 0 || ck.image >= a.images) return;
    const ScgPngImage im = a.img[ck.image];
    if (ck.index < 0 || ck.index >= im.chunks) return;
    const ScgPngChunkInfo info = a.info[c];
    const uint64_t off = (uint64_t)a.table[2 * ck.image] + 2u + (a.base[c] - a.base[im.first_chunk]);
    if (off + info.bytes > a.capacity) return;                       // cannot happen with the validated tables
    const bool final = ck.index == im.chunks - 1;

    if (t < kMaxBits + 2) s_cnt[t] = 0u;
    for (int i = t; i < kLens; i += kT) s_len[i] = a.lengths[(int64_t)c * kLens + i];
    const int n = load_filtered(s_data, im, ck.index, a.filter, a.gray_as_rgb);
    __syncthreads();

    if (info.kind == SCG_PNG_KIND_STORED) {
        const uint32_t un = (uint32_t)n;
        write_bytes(a.out, off, 0u, un + 5u, [&](uint32_t k) -> uint32_t {
            switch (k) {
                case 0: return final ? 1u : 0u;
                case 1: return un & 255u;
                case 2: return un >> 8;
                case 3: return ~un & 255u;
                case 4: return (~un >> 8) & 255u;
                default: return dbyte(s_data, (int)k - 5);
            }
        });
        return;
    }

    const Segment g = analyse_runs(s_data, n, s_scan);
    // canonical codes (RFC 1951 3.2.2): per length the first code, per symbol its rank among the earlier symbols of its length
    for (int i = t; i < kSyms; i += kT)
        if (s_len[i]) atomicAdd(&s_cnt[s_len[i]], 1u);
    __syncthreads();
    if (t == 0) {
        uint32_t code = 0u;
        s_cnt[0] = 0u;
        for (int l = 1; l <= kMaxBits; ++l) s_next[l] = code = (code + s_cnt[l - 1]) << 1;
    }
    __syncthreads();
    for (int i = t; i < kSyms; i += kT) {
        const uint32_t l = s_len[i];
        uint32_t cd = 0u;
        if (l) {
            uint32_t rank = 0u;
            for (int j = 0; j < i; ++j) rank += s_len[j] == l;
            cd = (__brev(s_next[l] + rank) >> (32u - l)) | (l << 16);
        }
        s_code[i] = cd;
    }
    __syncthreads();

    BitTokens bt{s_code, 0u};
    for_each_token(g, s_data, bt);
    uint32_t before, all;                                            // the threads' bit counts in front of this one, and all of them
    block_exclusive_sum<kT>(bt.bits, s_wave, before, all);
    const uint32_t my_lo = SCG_PNG_HEADER_BITS + before, my_hi = my_lo + bt.bits;
    const uint32_t eob_at = SCG_PNG_HEADER_BITS + all;
    const uint32_t end_bits = eob_at + (s_code[kEob] >> 16);
    const uint32_t tail = (end_bits + 3u + 7u) >> 3;                 // non-final: the empty stored block's LEN begins here
    const uint32_t bytes = final ? (end_bits + 7u) >> 3 : tail + 4u; // == info.bytes
    if (bytes != info.bytes) return;                                 // the count kernel's size is this one's, or nothing is written
    const uint32_t words = (bytes + 3u) >> 2;

    for (uint32_t wlo = 0u; wlo < words; wlo += kWinWords) {
        Window win{s_img, wlo, wlo + kWinWords};
        for (int i = t; i < kWinWords; i += kT) s_img[i] = 0u;
        __syncthreads();
        if (wlo == 0u) {                                             // the header lies in the first window: 1226 bits
            if (t == 0) {
                // BFINAL, BTYPE = 10 (the bits 0, 1), HLIT = 29, HDIST = 1, HCLEN = 15
                win.put(0u, (final ? 1u : 0u) | (2u << 1) | (29u << 3) | (1u << 8) | (15u << 13));
            }
            if (t < 19) win.put(17u + 3u * t, t < 3 ? 0u : 4u);   // RFC order 16 17 18 0 8 7 ...: the first three are unused
            for (int i = t; i < kLens; i += kT)                      // a length L has the 4-bit code L, sent from its top bit
                win.put(74u + 4u * i, __brev((uint32_t)s_len[i]) >> 28);
        }
        if (my_hi > 32u * win.wlo && my_lo < 32u * win.whi) {
            PutTokens pt{s_code, win, my_lo};
            for_each_token(g, s_data, pt);
        }
        if (t == 0) {
            win.put(eob_at, s_code[kEob] & 0xFFFFu);
            if (!final) win.put(8u * (tail + 2u), 0xFFFFu);
        }
        __syncthreads();
        const uint32_t b0 = 4u * wlo, b1 = min(bytes, 4u * (wlo + kWinWords));
        write_bytes(a.out, off, b0, b1, [&](uint32_t k) -> uint32_t { return reinterpret_cast<const uint8_t*>(s_img)[k - b0]; });
        __syncthreads();
    }
}

// ---- host ------------------------------------------------------------------------------------------------------------------------
bool filter_ok(int f) { return f == SCG_PNG_FILTER_NONE || f == SCG_PNG_FILTER_SUB || f == SCG_PNG_FILTER_UP || f == SCG_PNG_FILTER_PAETH; }

// The workspace's regions from images and chunks.
void place(ScgPngLayout* l) {
    l->lengths_offset = 0u;
    l->info_offset = align_to<16>(l->lengths_offset + l->chunks * kLens);
    l->base_offset = align_to<16>(l->info_offset + l->chunks * sizeof(ScgPngChunkInfo));
    l->scan_offset = align_to<16>(l->base_offset + 4u * (l->chunks + 1u));
    l->table_offset = align_to<16>(l->scan_offset + 4u * l->images);
    l->table_bytes = 8u * (l->images + 1u);
    l->workspace_bytes = align_to<16>(l->table_offset + l->table_bytes);
}

// The layout and the two tables from the sizes; who == nullptr: no message.
int layout_of(const char* who, int64_t n, const int32_t* hwc, int gray_as_rgb, ScgPngLayout* l, ScgPngImage* images, ScgPngChunk* chunks) {
    if (n < 0 || n > SCG_PNG_MAX_IMAGES) return who ? g_err.fail(SCG_E_RANGE, "%s: %lld images (0..%d)", who, (long long)n, SCG_PNG_MAX_IMAGES) : SCG_E_RANGE;
    if (n > 0 && !hwc) return who ? g_err.fail(SCG_E_NULL, "%s: hwc is NULL", who) : SCG_E_NULL;
    if (gray_as_rgb != 0 && gray_as_rgb != 1) return who ? g_err.fail(SCG_E_RANGE, "%s: gray_as_rgb = %d (0 or 1)", who, gray_as_rgb) : SCG_E_RANGE;
    uint64_t nchunks = 0, capacity = 0;
    for (int64_t i = 0; i < n; ++i) {
        const int32_t H = hwc[3 * i], W = hwc[3 * i + 1], C = hwc[3 * i + 2];
        if (H < 1 || W < 1 || H > SCG_PNG_MAX_DIM || W > SCG_PNG_MAX_DIM)
            return who ? g_err.fail(SCG_E_RANGE, "%s: image %lld of %d x %d pixels (H, W must be 1..%d)", who, (long long)i, W, H, SCG_PNG_MAX_DIM) : SCG_E_RANGE;
        if (C != 1 && C != 3) return who ? g_err.fail(SCG_E_RANGE, "%s: image %lld has %d channels (1 or 3)", who, (long long)i, C) : SCG_E_RANGE;
        const uint64_t bpp = (C == 3 || gray_as_rgb) ? 3u : 1u;
        const uint64_t S = (uint64_t)H * (1u + (uint64_t)W * bpp);
        if (S > SCG_PNG_MAX_STREAM)
            return who ? g_err.fail(SCG_E_RANGE, "%s: image %lld has a filtered stream of %llu bytes (< 2^31)", who, (long long)i, (unsigned long long)S) : SCG_E_RANGE;
        const uint64_t k = (S + SCG_PNG_CHUNK - 1u) / SCG_PNG_CHUNK;
        if (images) {
            ScgPngImage& im = images[i];
            im.src = 0u;
            im.H = H; im.W = W; im.channels = C;
            im.first_chunk = (int32_t)nchunks; im.chunks = (int32_t)k; im.stream_bytes = (int32_t)S;
        }
        if (chunks)
            for (uint64_t j = 0; j < k; ++j) {
                chunks[nchunks + j].image = (int32_t)i;
                chunks[nchunks + j].index = (int32_t)j;
            }
        nchunks += k;
        capacity += SCG_PNG_ALIGN + S + 5u * k + 6u;
        if (capacity > 0xFFFFFFFFull || nchunks > 0x7FFFFFFFull)
            return who ? g_err.fail(SCG_E_RANGE, "%s: the batch needs more than 2^32 - 1 bytes of output", who) : SCG_E_RANGE;
    }
    l->images = (uint64_t)n;
    l->chunks = nchunks;
    l->capacity = capacity;
    place(l);
    return 0;
}

}  // namespace
}  // namespace scg

using namespace scg;

extern "C" {

const char* scg_png_last_error(void) { return g_err.text; }
int32_t scg_png_abi_version(void) { return SCG_PNG_ABI_VERSION; }

size_t scg_png_struct_bytes(int32_t which) {
    switch (which) {
        case 0: return sizeof(ScgPngLayout);
        case 1: return sizeof(ScgPngImage);
        case 2: return sizeof(ScgPngChunk);
        case 3: return sizeof(ScgPngChunkInfo);
        case 4: return sizeof(ScgPngEncode);
        default: return 0;
    }
}

int scg_png_layout(int32_t n, const int32_t* hwc, int32_t gray_as_rgb, ScgPngLayout* out, ScgPngImage* images_out, ScgPngChunk* chunks_out) {
    if (!out) return g_err.fail(SCG_E_NULL, "scg_png_layout: out is NULL");
    ScgPngLayout l;
    if (int rc = layout_of("scg_png_layout", n, hwc, gray_as_rgb, &l, images_out, chunks_out)) return rc;
    *out = l;
    return 0;
}

int scg_png_encode(const ScgPngEncode* p, void* out, size_t out_bytes, void* workspace, size_t workspace_bytes, void* stream) {
    const char* who = "scg_png_encode";
    if (!p) return g_err.fail(SCG_E_NULL, "%s: args is NULL", who);
    if (p->struct_bytes != (int32_t)sizeof(ScgPngEncode))
        return g_err.fail(SCG_E_RANGE, "%s: struct_bytes = %d, the library's ScgPngEncode has %zu", who, p->struct_bytes, sizeof(ScgPngEncode));
    if (p->images < 1 || p->images > SCG_PNG_MAX_IMAGES) return g_err.fail(SCG_E_RANGE, "%s: images = %d is outside 1..%d", who, p->images, SCG_PNG_MAX_IMAGES);
    if (!filter_ok(p->filter)) return g_err.fail(SCG_E_RANGE, "%s: filter = %d (0 None, 1 Sub, 2 Up, 4 Paeth)", who, p->filter);
    if (p->gray_as_rgb != 0 && p->gray_as_rgb != 1) return g_err.fail(SCG_E_RANGE, "%s: gray_as_rgb = %d (0 or 1)", who, p->gray_as_rgb);
    if (!p->images_host || !p->images_dev) return g_err.fail(SCG_E_NULL, "%s: an image table is NULL", who);
    if (!p->chunks_dev) return g_err.fail(SCG_E_NULL, "%s: the chunk table is NULL", who);
    // the image table: the one the layout gives for its own sizes, record by record
    ScgPngLayout l;
    {
        uint64_t first = 0;
        int32_t hwc[3];
        ScgPngLayout one;
        ScgPngImage want;
        for (int i = 0; i < p->images; ++i) {
            const ScgPngImage& x = p->images_host[i];
            hwc[0] = x.H; hwc[1] = x.W; hwc[2] = x.channels;
            if (layout_of(nullptr, 1, hwc, p->gray_as_rgb, &one, &want, nullptr))
                return g_err.fail(SCG_E_RANGE, "%s: image %d of %d x %d pixels and %d channels is outside the limits", who, i, x.W, x.H, x.channels);
            if ((uint64_t)x.first_chunk != first || x.chunks != want.chunks || x.stream_bytes != want.stream_bytes)
                return g_err.fail(SCG_E_RANGE, "%s: image %d is (first chunk %d, chunks %d, stream %d), the layout gives (%llu, %d, %d)", who, i,
                                x.first_chunk, x.chunks, x.stream_bytes, (unsigned long long)first, want.chunks, want.stream_bytes);
            if (!x.src) return g_err.fail(SCG_E_NULL, "%s: image %d has no pixels (src is 0)", who, i);
            first += (uint64_t)want.chunks;
        }
        // the sums: the same arithmetic over all images
        uint64_t capacity = 0;
        for (int i = 0; i < p->images; ++i)
            capacity += SCG_PNG_ALIGN + (uint64_t)p->images_host[i].stream_bytes + 5u * (uint64_t)p->images_host[i].chunks + 6u;
        if (capacity > 0xFFFFFFFFull || first > 0x7FFFFFFFull)
            return g_err.fail(SCG_E_RANGE, "%s: the batch needs more than 2^32 - 1 bytes of output", who);
        l.images = (uint64_t)p->images;
        l.chunks = first;
        l.capacity = capacity;
        place(&l);
    }
    if (int rc = g_err.check_batch_buffers(who, out, out_bytes, l.capacity, workspace, workspace_bytes, l.workspace_bytes, p->images_dev, 8,
                                           p->chunks_dev, 4))
        return rc;

    PngArgs a;
    a.images = p->images;
    a.chunks = (int)l.chunks;
    a.filter = p->filter;
    a.gray_as_rgb = p->gray_as_rgb;
    a.img = p->images_dev;
    a.chunk = p->chunks_dev;
    char* ws = static_cast<char*>(workspace);
    a.lengths = reinterpret_cast<uint8_t*>(ws + l.lengths_offset);
    a.info = reinterpret_cast<ScgPngChunkInfo*>(ws + l.info_offset);
    a.base = reinterpret_cast<uint32_t*>(ws + l.base_offset);
    a.ioff = reinterpret_cast<uint32_t*>(ws + l.scan_offset);
    a.table = reinterpret_cast<uint32_t*>(ws + l.table_offset);
    a.out = static_cast<uint8_t*>(out);
    a.capacity = l.capacity;
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(png_count_kernel, dim3((unsigned)l.chunks), dim3(kT), 0, st, a);
    if (int rc = g_err.check_hip(hipGetLastError(), "png_count")) return rc;
    hipLaunchKernelGGL(png_scan_kernel, dim3(1), dim3(kT), 0, st, a);
    if (int rc = g_err.check_hip(hipGetLastError(), "png_scan")) return rc;
    hipLaunchKernelGGL(png_encode_kernel, dim3((unsigned)l.chunks), dim3(kT), 0, st, a);
    return g_err.check_hip(hipGetLastError(), "png_encode");
}

}  // extern "C"

// jpegpack.hip — libscg_jpg.so: baseline JPEG files packed on the GPU (include/jpg/scg_jpeg.h states the stream; it is the contract,
// and tests/jpeg_refs.py restates it in numpy).
//
// A JPEG is a per-block transform, a bit count, a scan and a bit pack; with one restart interval per MCU row nothing but the byte
// offset crosses a row.  A batch of any number of images of unequal sizes is three launches over the FLAT list of all images'
// MCU rows (segments):
//
//   jpeg_count_kernel   a workgroup per segment, rounds of 256 blocks, a block per thread: the 64 samples from the pixels (colour
//                       conversion and the 2 x 2 average on the way), libjpeg's integer DCT in registers, the exact quantiser, the
//                       quantised coefficients as int16 in LDS (a row of 33 dwords per thread: the odd stride keeps the lanes on
//                       distinct banks), the DC chain of the dummy blocks and the predictors through LDS, the code sizes, a
//                       workgroup scan of the bit offsets.  The bits are ORed, MSB first, into a 16 KiB LDS window that walks along
//                       the segment; a code word that straddles two windows is put into both.  A full window is only counted: its
//                       bytes and its FF bytes.
//   jpeg_scan_kernel    ONE workgroup: the segments' byte offsets (compact.h carry_scan), what every image needs, the images that
//                       fit back to back at multiples of 16, the table.
//   jpeg_encode_kernel  a workgroup per segment: the same device functions; a full window is written out, every thread 64 bytes of
//                       it behind a scan of the FF counts, then the marker; the first segment of an image copies its header.
//
// No workgroup waits for another, nothing is allocated, nothing is read back; the same input gives the same bytes.
#include "../../include/jpg/scg_jpeg.h"
#include "bitwindow.h"
#include "compact.h"
#include "host_align.h"
#include "host_error.h"

#include <map>
#include <tuple>

namespace scg {
namespace {

constexpr int kT = SCG_JPEG_THREADS;
constexpr int kRow = 66;                           // int16 per thread's block in LDS: 33 dwords
constexpr int kWinBytes = SCG_JPEG_WINDOW;
constexpr int kWinWords = kWinBytes / 4;
constexpr uint32_t kWinBits = 8u * kWinBytes;
constexpr int kMine = kWinBytes / kT;              // 64 bytes of a window per thread
constexpr int kHist = 8;                           // DC values of the round before that a block may refer to (at most 6 back)
static_assert(kT == kBlock && kMine == 64 && kWinWords % kT == 0, "a block per thread, 64 window bytes per thread");

thread_local ErrorText g_err = {};

// ---- the tables: data (T.81 Annex K) ---------------------------------------------------------------------------------------------
#define SCG_JPEG_ZIGZAG {0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, \
    28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63}
#define SCG_JPEG_BITS {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125}, \
    {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}, {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119}}
#define SCG_JPEG_DC_VALS {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11}
#define SCG_JPEG_AC_LUMA_VALS {1, 2, 3, 0, 4, 17, 5, 18, 33, 49, 65, 6, 19, 81, 97, 7, 34, 113, 20, 50, 129, 145, 161, 8, 35, 66, 177, 193, \
    21, 82, 209, 240, 36, 51, 98, 114, 130, 9, 10, 22, 23, 24, 25, 26, 37, 38, 39, 40, 41, 42, 52, 53, 54, 55, 56, 57, 58, 67, 68, 69, 70, \
    71, 72, 73, 74, 83, 84, 85, 86, 87, 88, 89, 90, 99, 100, 101, 102, 103, 104, 105, 106, 115, 116, 117, 118, 119, 120, 121, 122, 131, \
    132, 133, 134, 135, 136, 137, 138, 146, 147, 148, 149, 150, 151, 152, 153, 154, 162, 163, 164, 165, 166, 167, 168, 169, 170, 178, \
    179, 180, 181, 182, 183, 184, 185, 186, 194, 195, 196, 197, 198, 199, 200, 201, 202, 210, 211, 212, 213, 214, 215, 216, 217, 218, \
    225, 226, 227, 228, 229, 230, 231, 232, 233, 234, 241, 242, 243, 244, 245, 246, 247, 248, 249, 250}
#define SCG_JPEG_AC_CHROMA_VALS {0, 1, 2, 3, 17, 4, 5, 33, 49, 6, 18, 65, 81, 7, 97, 113, 19, 34, 50, 129, 8, 20, 66, 145, 161, 177, 193, 9, \
    35, 51, 82, 240, 21, 98, 114, 209, 10, 22, 36, 52, 225, 37, 241, 23, 24, 25, 26, 38, 39, 40, 41, 42, 53, 54, 55, 56, 57, 58, 67, 68, \
    69, 70, 71, 72, 73, 74, 83, 84, 85, 86, 87, 88, 89, 90, 99, 100, 101, 102, 103, 104, 105, 106, 115, 116, 117, 118, 119, 120, 121, \
    122, 130, 131, 132, 133, 134, 135, 136, 137, 138, 146, 147, 148, 149, 150, 151, 152, 153, 154, 162, 163, 164, 165, 166, 167, 168, \
    169, 170, 178, 179, 180, 181, 182, 183, 184, 185, 186, 194, 195, 196, 197, 198, 199, 200, 201, 202, 210, 211, 212, 213, 214, 215, \
    216, 217, 218, 226, 227, 228, 229, 230, 231, 232, 233, 234, 242, 243, 244, 245, 246, 247, 248, 249, 250}

// host copies (the header templates) and device copies (the code tables); table order DC0, AC0, DC1, AC1
const uint8_t h_zigzag[64] = SCG_JPEG_ZIGZAG;
const uint8_t h_bits[4][16] = SCG_JPEG_BITS;
const uint8_t h_dc_vals[12] = SCG_JPEG_DC_VALS;
const uint8_t h_ac_luma[162] = SCG_JPEG_AC_LUMA_VALS;
const uint8_t h_ac_chroma[162] = SCG_JPEG_AC_CHROMA_VALS;
// zigzag position of the natural index
__constant__ uint8_t d_unzigzag[64] = {0, 1, 5, 6, 14, 15, 27, 28, 2, 4, 7, 13, 16, 26, 29, 42, 3, 8, 12, 17, 25, 30, 41, 43, 9, 11, 18, 24, 31,
                                       40, 44, 53, 10, 19, 23, 32, 39, 45, 52, 54, 20, 22, 33, 38, 46, 51, 55, 60, 21, 34, 37, 47, 50, 56, 59,
                                       61, 35, 36, 48, 49, 57, 58, 62, 63};
__constant__ uint8_t d_bits[4][16] = SCG_JPEG_BITS;
__constant__ uint8_t d_dc_vals[12] = SCG_JPEG_DC_VALS;
__constant__ uint8_t d_ac_luma[162] = SCG_JPEG_AC_LUMA_VALS;
__constant__ uint8_t d_ac_chroma[162] = SCG_JPEG_AC_CHROMA_VALS;
// Annex K.1, natural order
const uint8_t h_base[2][64] = {
    {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
     18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99},
    {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};

struct JpegArgs {
    int images, segments, sub420, bgr;
    const ScgJpegImage* img;
    const ScgJpegSegment* seg;
    const uint8_t* headers;
    uint32_t* base;             // segments + 1: sizes, then exclusive offsets and their sum
    uint32_t* ioff;
    uint32_t* table;
    uint8_t* out;
    uint8_t q[2][64];           // natural order
};

// ---- samples ---------------------------------------------------------------------------------------------------------------------
struct Pixels {
    const uint8_t* src;
    int H, W, C, bgr;
    // component `comp` of the pixel (y, x), indices clamped to the image
    __device__ __forceinline__ int at(int comp, int y, int x) const {
        y = y < H ? y : H - 1;
        x = x < W ? x : W - 1;
        if (C == 1) return src[(int64_t)y * W + x];
        const uint8_t* p = src + ((int64_t)y * W + x) * 3;
        const int r = p[bgr ? 2 : 0], g = p[1], b = p[bgr ? 0 : 2];
        if (comp == 0) return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16;
        if (comp == 1) return (-11059 * r - 21709 * g + 32768 * b + 8388608 + 32767) >> 16;
        return (32768 * r - 27439 * g - 5329 * b + 8388608 + 32767) >> 16;
    }
    // the 2 x 2 average: columns padded then averaged, rows averaged then the last averaged row repeated
    __device__ __forceinline__ int chroma(int comp, int cy, int cx) const {
        const int last = (H + 1) / 2 - 1;
        cy = cy < last ? cy : last;
        return (at(comp, 2 * cy, 2 * cx) + at(comp, 2 * cy, 2 * cx + 1) + at(comp, 2 * cy + 1, 2 * cx) + at(comp, 2 * cy + 1, 2 * cx + 1) +
                1 + (cx & 1)) >> 2;
    }
};

// ---- libjpeg's jfdctint.c --------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }

template <int kStride, bool kFirst>
__device__ __forceinline__ void dct_pass(int* d) {
    constexpr int n = kFirst ? 13 - 2 : 13 + 2;
    const int t0 = d[0] + d[7 * kStride], t7 = d[0] - d[7 * kStride], t1 = d[kStride] + d[6 * kStride], t6 = d[kStride] - d[6 * kStride];
    const int t2 = d[2 * kStride] + d[5 * kStride], t5 = d[2 * kStride] - d[5 * kStride];
    const int t3 = d[3 * kStride] + d[4 * kStride], t4 = d[3 * kStride] - d[4 * kStride];
    const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    if (kFirst) {
        d[0] = (t10 + t11) << 2;
        d[4 * kStride] = (t10 - t11) << 2;
    } else {
        d[0] = descale(t10 + t11, 2);
        d[4 * kStride] = descale(t10 - t11, 2);
    }
    int z1 = (t12 + t13) * 4433;
    d[2 * kStride] = descale(z1 + t13 * 6270, n);
    d[6 * kStride] = descale(z1 - t12 * 15137, n);
    z1 = t4 + t7;
    int z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
    const int z5 = (z3 + z4) * 9633;
    const int a4 = t4 * 2446, a5 = t5 * 16819, a6 = t6 * 25172, a7 = t7 * 12299;
    z1 *= -7373;
    z2 *= -20995;
    z3 = z3 * -16069 + z5;
    z4 = z4 * -3196 + z5;
    d[7 * kStride] = descale(a4 + z1 + z3, n);
    d[5 * kStride] = descale(a5 + z2 + z4, n);
    d[3 * kStride] = descale(a6 + z2 + z3, n);
    d[kStride] = descale(a7 + z1 + z4, n);
}

// ---- the blocks of a segment -----------------------------------------------------------------------------------------------------
struct Geometry {
    Pixels px;
    int row, mcus, per, blocks;         // the MCU row, MCUs per row, blocks per MCU, blocks of the segment
    int wb, hb;                         // the real luminance blocks
    bool sub420;
};

struct Block {
    int comp;                           // 0 Y, 1 Cb, 2 Cr; -1: no block (behind the segment's end)
    int dummy_src;                      // > 0: a dummy, its DC is that of the block this many places before it
    int pred;                           // the block of the same component this many places before it predicts the DC (0: none)
};

__device__ __forceinline__ Block classify(const Geometry& g, int b, int& y0, int& x0) {
    Block k;
    k.comp = -1;
    k.dummy_src = k.pred = 0;
    y0 = x0 = 0;
    if (b >= g.blocks) return k;
    const int mx = b / g.per, p = b - mx * g.per;
    if (!g.sub420) {
        k.comp = p;
        k.pred = b >= g.per ? g.per : 0;
        y0 = 8 * g.row;
        x0 = 8 * mx;
        return k;
    }
    if (p >= 4) {
        k.comp = p - 3;
        k.pred = b >= 6 ? 6 : 0;
        y0 = 8 * g.row;                 // of the averaged plane
        x0 = 8 * mx;
        return k;
    }
    k.comp = 0;
    k.pred = p ? 1 : (b ? 3 : 0);       // Y00 follows the Y11 of the MCU before it
    const int by = 2 * g.row + (p >> 1), bx = 2 * mx + (p & 1);
    y0 = 8 * by;
    x0 = 8 * bx;
    const bool bottom = by >= g.hb, right = bx >= g.wb;
    if (bottom || right) {
        const bool y01_real = 2 * mx + 1 < g.wb;            // Y00 is always real
        if (p == 1) k.dummy_src = 1;
        else if (p == 2) k.dummy_src = y01_real ? 1 : 2;
        else k.dummy_src = bottom ? (y01_real ? 2 : 3) : 1;
    }
    return k;
}

// The thread's block: samples, DCT, quantiser; the 64 quantised coefficients in zigzag order into `coef` (its LDS row).
__device__ __forceinline__ void transform(const Geometry& g, const Block& k, int y0, int x0, const uint16_t* s_q, int16_t* coef) {
    const bool avg = g.sub420 && k.comp > 0;
#pragma nounroll
    for (int i = 0; i < 64; ++i)        // through the thread's own LDS row: a compact loop, and d[] below has constant indices only
        coef[i] = (int16_t)(avg ? g.px.chroma(k.comp, y0 + (i >> 3), x0 + (i & 7)) : g.px.at(k.comp, y0 + (i >> 3), x0 + (i & 7)));
    int d[64];
#pragma unroll
    for (int i = 0; i < 64; ++i) d[i] = coef[i] - 128;
#pragma unroll
    for (int r = 0; r < 8; ++r) dct_pass<1, true>(d + 8 * r);
#pragma unroll
    for (int c = 0; c < 8; ++c) dct_pass<8, false>(d + c);
    const uint16_t* q = s_q + (k.comp ? 64 : 0);
#pragma unroll
    for (int i = 0; i < 64; ++i) {
        const int v = d[i], qq = q[i], a = v < 0 ? -v : v;
        const int m = (a + 4 * qq) / (8 * qq);
        coef[d_unzigzag[i]] = (int16_t)(v < 0 ? -m : m);
    }
}

__device__ __forceinline__ int magnitude_bits(int v) {
    const int a = v < 0 ? -v : v;
    return a ? 32 - __clz(a) : 0;
}

// The code words of one block, in order: f.put(value, bits), at most 26 bits each.  code: (code | size << 16) per symbol.
template <class F>
__device__ __forceinline__ void for_each_code(const int16_t* coef, int diff, const uint32_t* dc, const uint32_t* ac, F& f) {
    int s = magnitude_bits(diff);
    uint32_t cd = dc[s];
    f.put(((cd & 0xFFFFu) << s) | ((uint32_t)(diff < 0 ? diff - 1 : diff) & ((1u << s) - 1u)), (int)(cd >> 16) + s);
    int run = 0;
    for (int z = 1; z < 64; ++z) {
        const int v = coef[z];
        if (v == 0) {
            ++run;
            continue;
        }
        while (run > 15) {
            f.put(ac[0xF0] & 0xFFFFu, (int)(ac[0xF0] >> 16));
            run -= 16;
        }
        s = magnitude_bits(v);
        cd = ac[(run << 4) | s];
        f.put(((cd & 0xFFFFu) << s) | ((uint32_t)(v < 0 ? v - 1 : v) & ((1u << s) - 1u)), (int)(cd >> 16) + s);
        run = 0;
    }
    if (run) f.put(ac[0] & 0xFFFFu, (int)(ac[0] >> 16));
}

struct CountBits {
    uint32_t bits;
    __device__ __forceinline__ void put(uint32_t, int n) { bits += (uint32_t)n; }
};

// The window: the words [wlo, wlo + kWinWords) of the segment's bit stream, big-endian words (bit 31 first).
struct PutBits {
    uint32_t* win;
    uint32_t wlo, at;
    __device__ __forceinline__ void put(uint32_t val, int n) {
        const uint64_t v = (uint64_t)val << (64 - (int)(at & 31u) - n);
        window_or(win, wlo, wlo + kWinWords, at >> 5, (uint32_t)(v >> 32), (uint32_t)v);
        at += (uint32_t)n;
    }
};

__device__ __forceinline__ uint32_t window_byte(const uint32_t* win, int k) { return (win[k >> 2] >> (24 - 8 * (k & 3))) & 255u; }

// The four code tables from BITS and HUFFVAL (T.81 Annex C): table order DC0, AC0, DC1, AC1, 256 entries each.
__device__ __forceinline__ void build_codes(uint32_t* s_code) {
    const int t = threadIdx.x;
    for (int i = t; i < 4 * 256; i += kT) s_code[i] = 0u;
    __syncthreads();
    if (t < 4) {
        const uint8_t* vals = (t & 1) ? (t == 1 ? d_ac_luma : d_ac_chroma) : d_dc_vals;
        uint32_t code = 0u;
        int k = 0;
        for (int size = 1; size <= 16; ++size) {
            for (int j = 0; j < d_bits[t][size - 1]; ++j) s_code[256 * t + vals[k++]] = code++ | ((uint32_t)size << 16);
            code <<= 1;
        }
    }
    __syncthreads();
}

// One segment.  kWrite: the encode kernel (bytes to `dst`, at most `limit` of them); else only the count.  Returns the stuffed
// size of the segment's entropy-coded bytes (without the marker), the same in every thread.
template <bool kWrite>
__device__ uint32_t walk_segment(const JpegArgs& a, const ScgJpegImage& im, int row, uint8_t* dst, uint32_t limit) {
    __shared__ int16_t s_coef[kT * kRow];
    __shared__ uint32_t s_win[kWinWords];
    __shared__ uint32_t s_code[4 * 256];
    __shared__ uint16_t s_q[128];
    __shared__ int s_dc[kHist + kT];
    __shared__ uint32_t s_wave[kT / kWave];
    __shared__ uint32_t s_ff[kT / kWave];

    const int t = threadIdx.x;
    Geometry g;
    g.px.src = reinterpret_cast<const uint8_t*>(im.src);
    g.px.H = im.H;
    g.px.W = im.W;
    g.px.C = im.channels;
    g.px.bgr = a.bgr;
    g.sub420 = im.channels == 3 && a.sub420;
    g.row = row;
    g.mcus = im.mcus;
    g.per = im.channels == 1 ? 1 : (g.sub420 ? 6 : 3);
    g.blocks = g.mcus * g.per;
    g.wb = (im.W + 7) / 8;
    g.hb = (im.H + 7) / 8;

    if (t < 128) s_q[t] = a.q[t >> 6][t & 63];
    if (t < kHist) s_dc[t] = 0;
    for (int i = t; i < kWinWords; i += kT) s_win[i] = 0u;
    build_codes(s_code);                                             // holds the barriers

    uint32_t P = 0u;                    // bits of the rounds before this one
    uint32_t cur = 0u;                  // the window in LDS
    uint32_t stuffed = 0u;              // FF bytes of the windows before `cur`

    // window `cur` holds nb bytes: count them (and write them); every thread calls it, behind a barrier
    auto flush = [&](uint32_t nb) {
        const int k0 = t * kMine, k1 = min(k0 + kMine, (int)nb);
        uint32_t ff = 0u;
        for (int k = k0; k < k1; ++k) ff += window_byte(s_win, k) == 255u;
        uint32_t before, all;
        block_exclusive_sum<kT>(ff, s_ff, before, all);
        if (kWrite) {
            uint32_t pos = cur * (uint32_t)kWinBytes + (uint32_t)k0 + stuffed + before;
            for (int k = k0; k < k1; ++k) {
                const uint32_t b = window_byte(s_win, k);
                if (pos < limit) dst[pos] = (uint8_t)b;
                ++pos;
                if (b == 255u) {
                    if (pos < limit) dst[pos] = 0;
                    ++pos;
                }
            }
        }
        stuffed += all;
        __syncthreads();                                             // s_ff and the window are free again
    };

    for (int first = 0; first < g.blocks; first += kT) {
        int y0, x0;
        const Block k = classify(g, first + t, y0, x0);
        int16_t* coef = s_coef + t * kRow;
        if (k.comp >= 0) {
            if (k.dummy_src) {
                for (int z = 0; z < 64; ++z) coef[z] = 0;
            } else {
                transform(g, k, y0, x0, s_q, coef);
                s_dc[kHist + t] = coef[0];
            }
        }
        __syncthreads();
        if (k.comp >= 0 && k.dummy_src) {                            // a real block of the same MCU, so not another dummy's slot
            const int dc = s_dc[kHist + t - k.dummy_src];
            coef[0] = (int16_t)dc;
            s_dc[kHist + t] = dc;
        }
        __syncthreads();
        CountBits cb{0u};
        int diff = 0;
        const uint32_t* dc_code = s_code + (k.comp > 0 ? 512 : 0);
        const uint32_t* ac_code = dc_code + 256;
        if (k.comp >= 0) {
            diff = coef[0] - (k.pred ? s_dc[kHist + t - k.pred] : 0);
            for_each_code(coef, diff, dc_code, ac_code, cb);
        }
        uint32_t before, R;                                          // the blocks' bit counts in front of this one, and the round's
        block_exclusive_sum<kT>(cb.bits, s_wave, before, R);         // (s_wave, not s_ff: no barrier between this scan and a flush's)
        const uint32_t my_lo = P + before, my_hi = my_lo + cb.bits;
        // the windows this round's bits [P, P + R) touch, in order; R > 0: a block has at least four bits
        for (uint32_t j = P / kWinBits; j <= (P + R - 1u) / kWinBits; ++j) {
            if (j != cur) {                                          // `cur` is full
                flush((uint32_t)kWinBytes);
                for (int i = t; i < kWinWords; i += kT) s_win[i] = 0u;
                cur = j;
                __syncthreads();
            }
            if (cb.bits && my_hi > j * kWinBits && my_lo < (j + 1u) * kWinBits) {
                PutBits pb{s_win, j * (uint32_t)kWinWords, my_lo};
                for_each_code(coef, diff, dc_code, ac_code, pb);
            }
            __syncthreads();
        }
        P += R;
        if (t >= kT - kHist) s_dc[t - (kT - kHist)] = s_dc[kHist + t];     // the tail of this round for the next one
        __syncthreads();
    }
    // the pad: 1-bits to the byte; bit P lies in window `cur` unless P is a multiple of the window (then there is no pad)
    const uint32_t pad = (8u - (P & 7u)) & 7u;
    if (t == 0 && pad) {
        PutBits pb{s_win, cur * (uint32_t)kWinWords, P};
        pb.put((1u << pad) - 1u, (int)pad);
    }
    __syncthreads();
    const uint32_t bytes = (P + 7u) >> 3;
    flush(bytes - cur * (uint32_t)kWinBytes);
    return bytes + stuffed;
}

// the segment of a workgroup: false when the record names nothing of the batch
__device__ __forceinline__ bool segment_of(const JpegArgs& a, int s, ScgJpegSegment& sg, ScgJpegImage& im) {
    if (s >= a.segments) return false;
    sg = a.seg[s];
    if (sg.image < 0 || sg.image >= a.images) return false;
    im = a.img[sg.image];
    return sg.row >= 0 && sg.row < im.segments && im.first_segment + sg.row == s;
}

// ---- launch 1: count -------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kT) void jpeg_count_kernel(JpegArgs a) {
    const int s = blockIdx.x;
    ScgJpegSegment sg;
    ScgJpegImage im;
    if (!segment_of(a, s, sg, im)) {
        if (s < a.segments && threadIdx.x == 0) a.base[s] = 0u;
        return;
    }
    const uint32_t n = walk_segment<false>(a, im, sg.row, nullptr, 0u);
    if (threadIdx.x == 0) a.base[s] = n + 2u;                        // the restart marker or FFD9 behind it
}

// ---- launch 2: scan --------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kT) void jpeg_scan_kernel(JpegArgs a) {
    __shared__ uint32_t s_over;
    const int t = threadIdx.x;
    uint32_t total[1];
    if (t == 0) s_over = 0u;
    __syncthreads();
    carry_scan<1, kT>(a.base, a.segments, total);
    if (t == 0) a.base[a.segments] = total[0];
    __syncthreads();
    for (int i = t; i < a.images; i += kT) {
        const ScgJpegImage im = a.img[i];
        const uint32_t raw = a.base[im.first_segment + im.segments] - a.base[im.first_segment];
        const uint64_t need = (uint64_t)im.header_bytes + raw;
        const bool fits = need <= (uint64_t)im.capacity;
        a.table[4 * i + 1] = fits ? (uint32_t)need : 0u;
        a.table[4 * i + 2] = need > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)need;
        a.table[4 * i + 3] = fits ? 0u : 1u;
        if (!fits) atomicAdd(&s_over, 1u);
        a.ioff[i] = fits ? ((uint32_t)need + (SCG_JPEG_ALIGN - 1u)) & ~(uint32_t)(SCG_JPEG_ALIGN - 1u) : 0u;
    }
    __syncthreads();
    carry_scan<1, kT>(a.ioff, a.images, total);
    for (int i = t; i < a.images; i += kT) a.table[4 * i] = a.ioff[i];
    if (t == 0) {
        a.table[4 * a.images] = total[0];
        a.table[4 * a.images + 1] = (uint32_t)a.images;
        a.table[4 * a.images + 2] = s_over;
        a.table[4 * a.images + 3] = 0u;
    }
}

// ---- launch 3: encode ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kT) void jpeg_encode_kernel(JpegArgs a) {
    const int s = blockIdx.x, t = threadIdx.x;
    ScgJpegSegment sg;
    ScgJpegImage im;
    if (!segment_of(a, s, sg, im)) return;
    if (a.table[4 * sg.image + 3]) return;                           // the file does not fit: no byte of it
    uint8_t* file = a.out + a.table[4 * sg.image];                   // its [0, bytes) lie inside the capacity: the scan kernel's test
    const uint32_t size = a.base[s + 1] - a.base[s];                 // entropy-coded bytes + 2
    uint8_t* dst = file + (uint32_t)im.header_bytes + (a.base[s] - a.base[im.first_segment]);
    if (sg.row == 0)
        for (int k = t; k < im.header_bytes; k += kT) file[k] = a.headers[im.header_offset + k];
    const uint32_t n = walk_segment<true>(a, im, sg.row, dst, size - 2u);
    if (t == 0 && n + 2u == size) {                                  // the count kernel's size is this one's, or no marker
        dst[n] = 0xFF;
        dst[n + 1u] = sg.row == im.segments - 1 ? 0xD9 : (uint8_t)(0xD0 + (sg.row & 7));
    }
}

// ---- host ------------------------------------------------------------------------------------------------------------------------
int scale_of(int q) { return q < 50 ? 5000 / q : 200 - 2 * q; }

void quant_tables(int quality, uint8_t q[2][64]) {
    const int s = scale_of(quality);
    for (int k = 0; k < 2; ++k)
        for (int i = 0; i < 64; ++i) {
            const int v = (h_base[k][i] * s + 50) / 100;
            q[k][i] = (uint8_t)(v < 1 ? 1 : (v > 255 ? 255 : v));
        }
}

bool sub_ok(int s) { return s == SCG_JPEG_444 || s == SCG_JPEG_420; }

int header_size(int channels) { return channels == 3 ? 629 : 334; }

// the header template of one shape; returns its size
int write_header(uint8_t* p, int H, int W, int channels, int quality, int subsampling, int mcus) {
    uint8_t q[2][64];
    quant_tables(quality, q);
    uint8_t* const p0 = p;
    auto put = [&](std::initializer_list<int> b) { for (int v : b) *p++ = (uint8_t)v; };
    put({0xFF, 0xD8, 0xFF, 0xE0, 0x00, 0x10, 'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0});
    for (int k = 0; k < (channels == 3 ? 2 : 1); ++k) {
        put({0xFF, 0xDB, 0x00, 0x43, k});
        for (int z = 0; z < 64; ++z) *p++ = q[k][h_zigzag[z]];
    }
    put({0xFF, 0xC0, 0x00, 8 + 3 * channels, 8, H >> 8, H & 255, W >> 8, W & 255, channels});
    if (channels == 3) put({1, subsampling == SCG_JPEG_420 ? 0x22 : 0x11, 0, 2, 0x11, 1, 3, 0x11, 1});
    else put({1, 0x11, 0});
    for (int k = 0; k < (channels == 3 ? 4 : 2); ++k) {
        const bool ac = k & 1;
        const int n = ac ? 162 : 12;
        const uint8_t* vals = ac ? (k == 1 ? h_ac_luma : h_ac_chroma) : h_dc_vals;
        put({0xFF, 0xC4, (19 + n) >> 8, (19 + n) & 255, (ac ? 0x10 : 0x00) | (k >> 1)});
        for (int i = 0; i < 16; ++i) *p++ = h_bits[k][i];
        for (int i = 0; i < n; ++i) *p++ = vals[i];
    }
    put({0xFF, 0xDD, 0x00, 0x04, mcus >> 8, mcus & 255});
    if (channels == 3) put({0xFF, 0xDA, 0x00, 0x0C, 3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 0x3F, 0});
    else put({0xFF, 0xDA, 0x00, 0x08, 1, 1, 0x00, 0, 0x3F, 0});
    return (int)(p - p0);
}

// the workspace's regions from images and segments
void place(ScgJpegLayout* l) {
    l->base_offset = 0u;
    l->scan_offset = align_to<16>(l->base_offset + 4u * (l->segments + 1u));
    l->table_offset = align_to<16>(l->scan_offset + 4u * l->images);
    l->table_bytes = 16u * (l->images + 1u);
    l->workspace_bytes = align_to<16>(l->table_offset + l->table_bytes);
}

// what depends on one image's shape alone; false: outside the limits
bool shape_of(int H, int W, int C, int subsampling, int* segments, int* mcus) {
    if (H < 1 || W < 1 || H > SCG_JPEG_MAX_DIM || W > SCG_JPEG_MAX_DIM || (C != 1 && C != 3)) return false;
    const int m = (C == 3 && subsampling == SCG_JPEG_420) ? 16 : 8;
    *segments = (H + m - 1) / m;
    *mcus = (W + m - 1) / m;
    return true;
}

int layout_of(const char* who, int64_t n, const int32_t* hwc, int quality, int subsampling, const uint32_t* capacities, ScgJpegLayout* l,
              ScgJpegImage* images, ScgJpegSegment* segments, uint8_t* headers) {
    if (n < 0 || n > SCG_JPEG_MAX_IMAGES) return g_err.fail(SCG_E_RANGE, "%s: %lld images (0..%d)", who, (long long)n, SCG_JPEG_MAX_IMAGES);
    if (n > 0 && !hwc) return g_err.fail(SCG_E_NULL, "%s: hwc is NULL", who);
    if (quality < 1 || quality > 100) return g_err.fail(SCG_E_RANGE, "%s: quality = %d (1..100)", who, quality);
    if (!sub_ok(subsampling)) return g_err.fail(SCG_E_RANGE, "%s: subsampling = %d (0: 4:4:4, 2: 4:2:0)", who, subsampling);
    std::map<std::tuple<int, int, int>, int> seen;                  // shape -> its template's offset
    uint64_t nseg = 0, capacity = 0, hbytes = 0;
    for (int64_t i = 0; i < n; ++i) {
        const int32_t H = hwc[3 * i], W = hwc[3 * i + 1], C = hwc[3 * i + 2];
        int segs, mcus;
        if (!shape_of(H, W, C, subsampling, &segs, &mcus))
            return g_err.fail(SCG_E_RANGE, "%s: image %lld of %d x %d pixels and %d channels (H, W must be 1..%d, channels 1 or 3)", who,
                              (long long)i, W, H, C, SCG_JPEG_MAX_DIM);
        const int hs = header_size(C);
        auto it = seen.find(std::make_tuple(H, W, C));
        int hoff;
        if (it == seen.end()) {
            hoff = (int)hbytes;
            seen.emplace(std::make_tuple(H, W, C), hoff);
            if (headers) write_header(headers + hoff, H, W, C, quality, subsampling, mcus);
            hbytes += (uint64_t)hs;
            if (hbytes > 0x7FFFFFFFull) return g_err.fail(SCG_E_RANGE, "%s: the header templates need more than 2^31 - 1 bytes", who);
        } else {
            hoff = it->second;
        }
        const uint64_t cap = capacities ? (uint64_t)capacities[i] : (uint64_t)hs + 3ull * (uint64_t)H * (uint64_t)W;
        if (cap > 0xFFFFFFFFull)
            return g_err.fail(SCG_E_RANGE, "%s: image %lld has a default capacity of %llu bytes (< 2^32): pass capacities", who, (long long)i,
                              (unsigned long long)cap);
        if (images) {
            ScgJpegImage& im = images[i];
            im.src = 0u;
            im.H = H; im.W = W; im.channels = C;
            im.first_segment = (int32_t)nseg; im.segments = segs; im.mcus = mcus;
            im.header_offset = hoff; im.header_bytes = hs;
            im.capacity = (uint32_t)cap;
            im.reserved = 0;
        }
        if (segments)
            for (int j = 0; j < segs; ++j) {
                segments[nseg + j].image = (int32_t)i;
                segments[nseg + j].row = j;
            }
        nseg += (uint64_t)segs;
        capacity += align_to<16>(cap);
        if (capacity > 0xFFFFFFFFull || nseg > 0x7FFFFFFFull)
            return g_err.fail(SCG_E_RANGE, "%s: the batch needs more than 2^32 - 1 bytes of output or 2^31 - 1 segments", who);
    }
    l->images = (uint64_t)n;
    l->segments = nseg;
    l->headers_bytes = hbytes;
    l->capacity = capacity;
    place(l);
    return 0;
}

}  // namespace
}  // namespace scg

using namespace scg;

extern "C" {

const char* scg_jpg_last_error(void) { return g_err.text; }
int32_t scg_jpg_abi_version(void) { return SCG_JPG_ABI_VERSION; }

size_t scg_jpg_struct_bytes(int32_t which) {
    switch (which) {
        case 0: return sizeof(ScgJpegLayout);
        case 1: return sizeof(ScgJpegImage);
        case 2: return sizeof(ScgJpegSegment);
        case 3: return sizeof(ScgJpegEncode);
        default: return 0;
    }
}

int scg_jpeg_layout(int32_t n, const int32_t* hwc, int32_t quality, int32_t subsampling, const uint32_t* capacities, ScgJpegLayout* out,
                    ScgJpegImage* images_out, ScgJpegSegment* segments_out, uint8_t* headers_out) {
    if (!out) return g_err.fail(SCG_E_NULL, "scg_jpeg_layout: out is NULL");
    ScgJpegLayout l;
    if (int rc = layout_of("scg_jpeg_layout", n, hwc, quality, subsampling, capacities, &l, images_out, segments_out, headers_out)) return rc;
    *out = l;
    return 0;
}

int scg_jpeg_encode(const ScgJpegEncode* p, void* out, size_t out_bytes, void* workspace, size_t workspace_bytes, void* stream) {
    const char* who = "scg_jpeg_encode";
    if (!p) return g_err.fail(SCG_E_NULL, "%s: args is NULL", who);
    if (p->struct_bytes != (int32_t)sizeof(ScgJpegEncode))
        return g_err.fail(SCG_E_RANGE, "%s: struct_bytes = %d, the library's ScgJpegEncode has %zu", who, p->struct_bytes, sizeof(ScgJpegEncode));
    if (p->images < 1 || p->images > SCG_JPEG_MAX_IMAGES) return g_err.fail(SCG_E_RANGE, "%s: images = %d is outside 1..%d", who, p->images, SCG_JPEG_MAX_IMAGES);
    if (p->quality < 1 || p->quality > 100) return g_err.fail(SCG_E_RANGE, "%s: quality = %d (1..100)", who, p->quality);
    if (!sub_ok(p->subsampling)) return g_err.fail(SCG_E_RANGE, "%s: subsampling = %d (0: 4:4:4, 2: 4:2:0)", who, p->subsampling);
    if (p->bgr != 0 && p->bgr != 1) return g_err.fail(SCG_E_RANGE, "%s: bgr = %d (0 or 1)", who, p->bgr);
    if (!p->images_host || !p->images_dev) return g_err.fail(SCG_E_NULL, "%s: an image table is NULL", who);
    if (!p->segments_dev) return g_err.fail(SCG_E_NULL, "%s: the segment table is NULL", who);
    if (!p->headers_dev) return g_err.fail(SCG_E_NULL, "%s: the header templates are NULL", who);
    // the image table: the one the layout gives for its own sizes, record by record
    ScgJpegLayout l;
    uint64_t first = 0, capacity = 0;
    for (int i = 0; i < p->images; ++i) {
        const ScgJpegImage& x = p->images_host[i];
        int segs, mcus;
        if (!shape_of(x.H, x.W, x.channels, p->subsampling, &segs, &mcus))
            return g_err.fail(SCG_E_RANGE, "%s: image %d of %d x %d pixels and %d channels is outside the limits", who, i, x.W, x.H, x.channels);
        if ((uint64_t)x.first_segment != first || x.segments != segs || x.mcus != mcus)
            return g_err.fail(SCG_E_RANGE, "%s: image %d is (first segment %d, segments %d, MCUs %d), the layout gives (%llu, %d, %d)", who, i,
                              x.first_segment, x.segments, x.mcus, (unsigned long long)first, segs, mcus);
        if (x.header_bytes != header_size(x.channels) || x.header_offset < 0 ||
            (uint64_t)x.header_offset + (uint64_t)x.header_bytes > p->headers_bytes)
            return g_err.fail(SCG_E_RANGE, "%s: image %d has its header at [%d, +%d) of %llu template bytes", who, i, x.header_offset,
                              x.header_bytes, (unsigned long long)p->headers_bytes);
        if (!x.src) return g_err.fail(SCG_E_NULL, "%s: image %d has no pixels (src is 0)", who, i);
        first += (uint64_t)segs;
        capacity += align_to<16>((uint64_t)x.capacity);
    }
    if (capacity > 0xFFFFFFFFull || first > 0x7FFFFFFFull)
        return g_err.fail(SCG_E_RANGE, "%s: the batch needs more than 2^32 - 1 bytes of output or 2^31 - 1 segments", who);
    l.images = (uint64_t)p->images;
    l.segments = first;
    l.headers_bytes = p->headers_bytes;
    l.capacity = capacity;
    place(&l);
    if (int rc = g_err.check_batch_buffers(who, out, out_bytes, l.capacity, workspace, workspace_bytes, l.workspace_bytes, p->images_dev, 8,
                                           p->segments_dev, 4))
        return rc;

    JpegArgs a;
    a.images = p->images;
    a.segments = (int)l.segments;
    a.sub420 = p->subsampling == SCG_JPEG_420;
    a.bgr = p->bgr;
    a.img = p->images_dev;
    a.seg = p->segments_dev;
    a.headers = p->headers_dev;
    char* ws = static_cast<char*>(workspace);
    a.base = reinterpret_cast<uint32_t*>(ws + l.base_offset);
    a.ioff = reinterpret_cast<uint32_t*>(ws + l.scan_offset);
    a.table = reinterpret_cast<uint32_t*>(ws + l.table_offset);
    a.out = static_cast<uint8_t*>(out);
    quant_tables(p->quality, a.q);
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(jpeg_count_kernel, dim3((unsigned)l.segments), dim3(kT), 0, st, a);
    if (int rc = g_err.check_hip(hipGetLastError(), "jpeg_count")) return rc;
    hipLaunchKernelGGL(jpeg_scan_kernel, dim3(1), dim3(kT), 0, st, a);
    if (int rc = g_err.check_hip(hipGetLastError(), "jpeg_scan")) return rc;
    hipLaunchKernelGGL(jpeg_encode_kernel, dim3((unsigned)l.segments), dim3(kT), 0, st, a);
    return g_err.check_hip(hipGetLastError(), "jpeg_encode");
}

}  // extern "C"

// depthviz.hip — the reference's depth colour maps and video frames, per frame (include/scg_viz.h).
//
//   render.py:97-110, render_video.py:98-113   np.percentile(depth, 98), depth.min()       -> select_pass_kernel x 3, select_finish_kernel
//                                              Normalize, the turbo table, the byte cast   -> viz_frame_kernel
//   render_video.py:132,148                    (clamp(rendering) * 255.).astype(uint8)[..., ::-1]          -> viz_frame_kernel
//
// Selection: the values of rank lo and hi of x are found digit by digit on the order-preserving key of x, 11 + 11 + 10 bits.  A
// pass counts, per workgroup in LDS and then with integer atomics in a global histogram, the next digit of the values that carry
// the digits chosen so far — for rank lo and for rank hi, which may part ways at any digit (one histogram while they agree).  The
// workgroups of the next pass each scan the global histograms again to find those digits: nothing waits, nothing is read on the
// host, and integer sums are exact in any order.
//
// Normalised depths lie in [0, 1]: the first digit (sign, exponent, two mantissa bits) of most pixels falls in about a dozen
// bins, and a wave's adds to one LDS address serialise.  SCG_VIZ_HIST_MODE picks what is done about it, for
// tools/depthviz_timing.py to measure one against the other (README, round 15, says which is the default and why):
//   0  nothing: one LDS atomic per value
//   1  wave_hist_add merges equal digits within the wave first (a ballot per distinct digit, one add of the population count), for
//      at most kMergeRounds distinct digits; lanes left after that add on their own
//   2  every wave of the first pass has a histogram of its own (the later passes count only the few values under the chosen prefix)
//
// Compiled with -ffp-contract=off: x, the interpolation between the two order statistics and the normalisation are chains of
// separately rounded fp32 operations, as numpy and torch round them (the byte rules are pixel_rules.h's; its quantiser pins its own
// two roundings).  Divisions are the correctly rounded __fdiv_rn; the one of the normalisation is matplotlib's, in fp64
// (viz_frame_kernel).
#include <math.h>

#include "scg_common.h"
#include "reduce.h"
#include "pixel_rules.h"
#include "../../include/scg_viz.h"

namespace scg {

constexpr int kSelPerThread = 16;
constexpr int kSelBlock = kBlock * kSelPerThread;          // values of x a workgroup of a pass reads
constexpr int kBits0 = 11, kBits1 = 11, kBits2 = 10;
constexpr int kBins0 = 1 << kBits0, kBins1 = 1 << kBits1, kBins2 = 1 << kBits2;
constexpr int kMergeRounds = 8;
#ifndef SCG_VIZ_HIST_MODE
#define SCG_VIZ_HIST_MODE 0
#endif
constexpr int64_t kSelMaxN = 1ll << 24;                    // n - 1 exact in fp32
static_assert(kBits0 + kBits1 + kBits2 == 32, "the three digits are the key");

// scratch, in 32-bit words
constexpr int kOffHist0 = 0;                               // [kBins0]
constexpr int kOffHist1 = kOffHist0 + kBins0;              // [2][kBins1]: rank lo, rank hi (the second only where the prefixes differ)
constexpr int kOffHist2 = kOffHist1 + 2 * kBins1;          // [2][kBins2]
constexpr int kOffMaxInv = kOffHist2 + 2 * kBins2;         // max of ~key: the minimum, from a zeroed word
constexpr int kOffNan = kOffMaxInv + 1;
constexpr int kSelWords = kOffNan + 1;

// the plane being coloured (scg_viz.h): the one place that forms x
__device__ __forceinline__ float viz_x(float d, const float* __restrict__ range) {
    if (!range) return d;
    const float lo = range[0], hi = range[1];
    return __fdiv_rn(d - lo, hi - lo);
}

// ascending keys for ascending floats; -0.0 in front of +0.0; every NaN behind +inf
__device__ __forceinline__ uint32_t key_of(float x) {
    if (x != x) return 0xFFFFFFFFu;
    const uint32_t b = __float_as_uint(x);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float value_of(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k); }

// ++hist[bin] for the lanes with `valid`; called by whole waves
__device__ __forceinline__ void wave_hist_add(uint32_t* hist, uint32_t bin, bool valid) {
#if SCG_VIZ_HIST_MODE == 1
    unsigned long long todo = __ballot(valid);
    for (int round = 0; round < kMergeRounds && todo; ++round) {
        const int leader = __ffsll((long long)todo) - 1;
        const uint32_t b = (uint32_t)__shfl((int)bin, leader, kWave);
        const unsigned long long same = __ballot(valid && bin == b);
        if (lane_id() == leader) atomicAdd(&hist[b], (uint32_t)__popcll(same));
        todo &= ~same;
    }
    valid = (todo >> lane_id()) & 1ull;
#endif
    if (valid) atomicAdd(&hist[bin], 1u);
}

// The digit that holds rank `rank` of a histogram of NB bins, and the rank within that bin.  Whole workgroup; s_scan: kBlock / kWave
// words, s_pick: 2 words.
template <int NB>
__device__ __forceinline__ void pick_digit(const uint32_t* __restrict__ hist, uint32_t rank, uint32_t* s_scan, uint32_t* s_pick,
                                           uint32_t& digit, uint32_t& rest) {
    constexpr int kPer = NB / kBlock;
    uint32_t c[kPer], sum = 0;
#pragma unroll
    for (int k = 0; k < kPer; ++k) { c[k] = hist[threadIdx.x * kPer + k]; sum += c[k]; }
    uint32_t inc = sum;
#pragma unroll
    for (int off = 1; off < kWave; off <<= 1) {
        const uint32_t t = __shfl_up(inc, off, kWave);
        if (lane_id() >= off) inc += t;
    }
    if (threadIdx.x == 0) { s_pick[0] = 0; s_pick[1] = 0; }
    if (lane_id() == kWave - 1) s_scan[wave_id()] = inc;
    __syncthreads();
    uint32_t excl = inc - sum;
    for (int w = 0; w < wave_id(); ++w) excl += s_scan[w];
#pragma unroll
    for (int k = 0; k < kPer; ++k) {
        if (rank >= excl && rank - excl < c[k]) { s_pick[0] = threadIdx.x * kPer + k; s_pick[1] = rank - excl; }
        excl += c[k];
    }
    __syncthreads();
    digit = s_pick[0];
    rest = s_pick[1];
    __syncthreads();
}

// the prefixes and remaining ranks of rank lo and rank hi in front of pass PASS (1, 2) or of the last digit's choice (3)
struct Chosen { uint32_t prefix[2], rank[2]; };

template <int PASS>
__device__ __forceinline__ Chosen choose(const uint32_t* __restrict__ scratch, uint32_t lo, uint32_t hi, uint32_t* s_scan, uint32_t* s_pick) {
    Chosen c;
    c.prefix[0] = c.prefix[1] = 0; c.rank[0] = lo; c.rank[1] = hi;
    uint32_t d;
#pragma unroll
    for (int w = 0; w < 2; ++w) {
        pick_digit<kBins0>(scratch + kOffHist0, c.rank[w], s_scan, s_pick, d, c.rank[w]);
        c.prefix[w] = d;
    }
    if (PASS >= 2) {
        const bool same = c.prefix[0] == c.prefix[1];
#pragma unroll
        for (int w = 0; w < 2; ++w) {
            pick_digit<kBins1>(scratch + kOffHist1 + ((w && !same) ? kBins1 : 0), c.rank[w], s_scan, s_pick, d, c.rank[w]);
            c.prefix[w] = (c.prefix[w] << kBits1) | d;
        }
    }
    if (PASS >= 3) {
        const bool same = c.prefix[0] == c.prefix[1];
#pragma unroll
        for (int w = 0; w < 2; ++w) {
            pick_digit<kBins2>(scratch + kOffHist2 + ((w && !same) ? kBins2 : 0), c.rank[w], s_scan, s_pick, d, c.rank[w]);
            c.prefix[w] = (c.prefix[w] << kBits2) | d;
        }
    }
    return c;
}

template <int PASS>
__global__ __launch_bounds__(kBlock) void select_pass_kernel(const float* __restrict__ depth, const float* __restrict__ range, int n,
                                                             uint32_t lo, uint32_t hi, uint32_t* __restrict__ scratch) {
    constexpr int kBins = PASS == 0 ? kBins0 : (PASS == 1 ? kBins1 : kBins2);
    constexpr int kShift = PASS == 0 ? kBits1 + kBits2 : (PASS == 1 ? kBits2 : 0);          // of this pass's digit
    constexpr int kHists = PASS == 0 ? 1 : 2;
    constexpr int kCopies = (PASS == 0 && SCG_VIZ_HIST_MODE == 2) ? kBlock / kWave : 1;          // one per wave, or one
    __shared__ uint32_t s_hist[kCopies * kHists * kBins];
    __shared__ uint32_t s_scan[kBlock / kWave], s_pick[2], s_red[2][kBlock / kWave];
    for (int i = threadIdx.x; i < kCopies * kHists * kBins; i += kBlock) s_hist[i] = 0;
    Chosen c;
    c.prefix[0] = c.prefix[1] = 0;
    if (PASS > 0) c = choose<PASS>(scratch, lo, hi, s_scan, s_pick);
    const bool two = c.prefix[0] != c.prefix[1];
    __syncthreads();
    uint32_t max_inv = 0, nans = 0;
    const int base = blockIdx.x * kSelBlock + threadIdx.x;
#pragma unroll 4
    for (int k = 0; k < kSelPerThread; ++k) {
        const int i = base + k * kBlock;
        const bool in = i < n;
        const float x = in ? viz_x(depth[i], range) : 0.f;
        const uint32_t key = key_of(x);
        const uint32_t bin = (key >> kShift) & (uint32_t)(kBins - 1);
        if (PASS == 0) {
            if (in) { max_inv = max(max_inv, ~key); nans += x != x; }
            wave_hist_add(s_hist + (kCopies > 1 ? wave_id() * kBins : 0), bin, in);
        } else {
            const uint32_t pre = key >> (kShift + (PASS == 1 ? kBits1 : kBits2));
            wave_hist_add(s_hist, bin, in && pre == c.prefix[0]);
            if (two) wave_hist_add(s_hist + kBins, bin, in && pre == c.prefix[1]);          // `two` is uniform
        }
    }
    __syncthreads();
    uint32_t* g_hist = scratch + (PASS == 0 ? kOffHist0 : (PASS == 1 ? kOffHist1 : kOffHist2));
    for (int i = threadIdx.x; i < kHists * kBins; i += kBlock) {
        uint32_t v = 0;
#pragma unroll
        for (int w = 0; w < kCopies; ++w) v += s_hist[w * kHists * kBins + i];
        if (v) atomicAdd(&g_hist[i], v);
    }
    if (PASS == 0) {
        wave_publish(max_inv, nans, s_red[0], s_red[1], Max(), Sum());
        __syncthreads();
        if (threadIdx.x == 0) {
            const uint32_t m = wg_fold<kBlock / kWave>(s_red[0], Max()), z = wg_fold<kBlock / kWave>(s_red[1], Sum());
            if (m) atomicMax(&scratch[kOffMaxInv], m);
            if (z) atomicAdd(&scratch[kOffNan], z);
        }
    }
}

__global__ __launch_bounds__(kBlock) void select_finish_kernel(const uint32_t* __restrict__ scratch, uint32_t lo, uint32_t hi, float g,
                                                               float* __restrict__ stats, int32_t* __restrict__ nan_count) {
    __shared__ uint32_t s_scan[kBlock / kWave], s_pick[2];
    const Chosen c = choose<3>(scratch, lo, hi, s_scan, s_pick);
    if (threadIdx.x != 0) return;
    const uint32_t nans = scratch[kOffNan];
    const float a = value_of(c.prefix[0]), b = value_of(c.prefix[1]);
    float vmin = value_of(~scratch[kOffMaxInv]);
    const float d = b - a;
    float vmax = g < 0.5f ? a + d * g : b - d * (1.f - g);          // numpy's _lerp; contraction is off for this file
    if (nans) vmin = vmax = __uint_as_float(0x7FC00000u);
    stats[0] = vmin; stats[1] = vmax; stats[2] = a; stats[3] = b;
    *nan_count = (int32_t)nans;
}

constexpr int kPxPerThread = 4;                            // 12 bytes of an interleaved image: three aligned words

// p[k] = byte0 | byte1 << 8 | byte2 << 16 of pixel i0 + k; `count` of them are inside the image
__device__ __forceinline__ void store_pixels(uint8_t* __restrict__ out, size_t i0, int count, const uint32_t (&p)[kPxPerThread]) {
    uint8_t* dst = out + i0 * 3;
    if (count == kPxPerThread && (reinterpret_cast<uintptr_t>(dst) & 3) == 0) {
        uint32_t* w = reinterpret_cast<uint32_t*>(dst);
        w[0] = p[0] | (p[1] << 24);
        w[1] = (p[1] >> 8) | (p[2] << 16);
        w[2] = (p[2] >> 16) | (p[3] << 8);
        return;
    }
    for (int k = 0; k < count; ++k) {
        dst[3 * k] = (uint8_t)p[k]; dst[3 * k + 1] = (uint8_t)(p[k] >> 8); dst[3 * k + 2] = (uint8_t)(p[k] >> 16);
    }
}

__device__ __forceinline__ uint32_t swap_rb(uint32_t p) { return ((p & 0xFFu) << 16) | (p & 0xFF00u) | (p >> 16); }

__global__ __launch_bounds__(kBlock) void viz_frame_kernel(const float* __restrict__ render, const float* __restrict__ depth,
                                                           const float* __restrict__ range, const float* __restrict__ stats,
                                                           const int32_t* __restrict__ nan_count, const uint8_t* __restrict__ lut,
                                                           size_t plane, uint8_t* __restrict__ color_rgb, uint8_t* __restrict__ color_bgr,
                                                           uint8_t* __restrict__ depth_u8, uint8_t* __restrict__ render_u8,
                                                           uint8_t* __restrict__ frame_bgr) {
    __shared__ uint32_t s_lut[256];
    s_lut[threadIdx.x] = (uint32_t)lut[3 * threadIdx.x] | ((uint32_t)lut[3 * threadIdx.x + 1] << 8) | ((uint32_t)lut[3 * threadIdx.x + 2] << 16);
    __syncthreads();
    const size_t i0 = ((size_t)blockIdx.x * kBlock + threadIdx.x) * kPxPerThread;
    if (i0 >= plane) return;
    const int count = (int)min((size_t)kPxPerThread, plane - i0);
    const float vmin = stats[0], vmax = stats[1];
    const bool flat = vmin == vmax, bad_image = *nan_count > 0;
    const double den = (double)vmax - (double)vmin;       // Normalize holds vmin and vmax as Python floats: the difference is fp64
    uint32_t col[kPxPerThread], grey[kPxPerThread];
#pragma unroll
    for (int k = 0; k < kPxPerThread; ++k) {
        col[k] = 0; grey[k] = 0;
        if (k >= count) continue;
        const float x = viz_x(depth[i0 + k], range);
        grey[k] = quantise(x);
        if (flat) { col[k] = s_lut[0]; continue; }
        const float t = (float)__ddiv_rn((double)(x - vmin), den);          // numpy's fp32 array /= fp64 scalar: one fp64 division, rounded to fp32
        if (t != t || bad_image) continue;                 // matplotlib's "bad" colour: (0, 0, 0)
        const float s = t * 256.f;
        col[k] = s_lut[s < 0.f ? 0 : (s >= 256.f ? 255 : (int)s)];
    }
    store_pixels(color_rgb, i0, count, col);
    if (color_bgr) {
#pragma unroll
        for (int k = 0; k < kPxPerThread; ++k) col[k] = swap_rb(col[k]);
        store_pixels(color_bgr, i0, count, col);
    }
    if (depth_u8) {
        uint8_t* dst = depth_u8 + i0;
        if (count == kPxPerThread && (reinterpret_cast<uintptr_t>(dst) & 3) == 0)
            *reinterpret_cast<uint32_t*>(dst) = grey[0] | (grey[1] << 8) | (grey[2] << 16) | (grey[3] << 24);
        else
            for (int k = 0; k < count; ++k) dst[k] = (uint8_t)grey[k];
    }
    if (render_u8 || frame_bgr) {
        uint32_t q[kPxPerThread], v[kPxPerThread];
#pragma unroll
        for (int k = 0; k < kPxPerThread; ++k) {
            q[k] = 0; v[k] = 0;
            if (k >= count) continue;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float r = render[c * plane + i0 + k];
                q[k] |= quantise(unit_clamp(r)) << (8 * c);
                v[k] |= video_byte(r) << (8 * (2 - c));    // B, G, R
            }
        }
        if (render_u8) store_pixels(render_u8, i0, count, q);
        if (frame_bgr) store_pixels(frame_bgr, i0, count, v);
    }
}

}  // namespace scg

using namespace scg;

extern "C" {

int32_t scg_viz_select_block(void) { return kSelBlock; }

size_t scg_viz_select_scratch_bytes(int64_t n) {
    if (n < 1 || n > kSelMaxN) return 0;
    return (size_t)kSelWords * sizeof(uint32_t);
}

int scg_viz_select(const float* depth, const float* range, int64_t n, double percentile, float* stats, int32_t* nan_count,
                   void* scratch, size_t scratch_bytes, void* stream) {
    if (n < 1 || n > kSelMaxN) return fail(SCG_E_RANGE, "viz_select: n out of range (1 .. 2^24: n - 1 must be exact in fp32)");
    if (!(percentile >= 0.0 && percentile <= 100.0)) return fail(SCG_E_RANGE, "viz_select: percentile out of range (0 .. 100)");
    if (!depth || !stats || !nan_count || !scratch) return fail(SCG_E_NULL, "viz_select pointer is NULL");
    if (scratch_bytes < scg_viz_select_scratch_bytes(n)) return fail(SCG_E_SCRATCH, "viz_select scratch too small");
    if (reinterpret_cast<uintptr_t>(scratch) % 4) return fail(SCG_E_ALIGN, "viz_select scratch not 4-byte aligned");
    // numpy's virtual index of method 'linear' on a float32 array: every operation in fp32
    const float q = (float)percentile / 100.0f;
    const float pos = (float)(n - 1) * q;
    const float fl = floorf(pos);
    const uint32_t lo = (uint32_t)fl, hi = (uint32_t)(lo + 1 < (uint32_t)n ? lo + 1 : n - 1);
    const float g = pos - fl;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    uint32_t* words = reinterpret_cast<uint32_t*>(scratch);
    int rc = check_hip(hipMemsetAsync(words, 0, (size_t)kSelWords * sizeof(uint32_t), s), "viz_select scratch reset");
    if (rc) return rc;
    const int blocks = (int)((n + kSelBlock - 1) / kSelBlock);
    hipLaunchKernelGGL(select_pass_kernel<0>, dim3(blocks), dim3(kBlock), 0, s, depth, range, (int)n, lo, hi, words);
    hipLaunchKernelGGL(select_pass_kernel<1>, dim3(blocks), dim3(kBlock), 0, s, depth, range, (int)n, lo, hi, words);
    hipLaunchKernelGGL(select_pass_kernel<2>, dim3(blocks), dim3(kBlock), 0, s, depth, range, (int)n, lo, hi, words);
    hipLaunchKernelGGL(select_finish_kernel, dim3(1), dim3(kBlock), 0, s, words, lo, hi, g, stats, nan_count);
    return check_hip(hipGetLastError(), "viz_select");
}

int scg_viz_frame(const float* render, const float* depth, const float* range, const float* stats, const int32_t* nan_count,
                  const uint8_t* lut, int32_t H, int32_t W, uint8_t* depth_color_u8, uint8_t* depth_color_bgr_u8, uint8_t* depth_u8,
                  uint8_t* render_u8, uint8_t* frame_bgr_u8, void* stream) {
    if (H < 1 || W < 1 || (int64_t)H * W >= (1ll << 31)) return fail(SCG_E_RANGE, "viz_frame: image dims out of range");
    if (!depth || !stats || !nan_count || !lut || !depth_color_u8) return fail(SCG_E_NULL, "viz_frame pointer is NULL");
    if (!render && (render_u8 || frame_bgr_u8)) return fail(SCG_E_NULL, "viz_frame: render is NULL with render_u8 or frame_bgr_u8");
    const size_t plane = (size_t)H * W;
    const unsigned blocks = (unsigned)((plane + (size_t)kBlock * kPxPerThread - 1) / ((size_t)kBlock * kPxPerThread));
    hipLaunchKernelGGL(viz_frame_kernel, dim3(blocks), dim3(kBlock), 0, reinterpret_cast<hipStream_t>(stream), render, depth, range,
                       stats, nan_count, lut, plane, depth_color_u8, depth_color_bgr_u8, depth_u8, render_u8, frame_bgr_u8);
    return check_hip(hipGetLastError(), "viz_frame_kernel");
}

}  // extern "C"

// evalview.hip — the reference's test-set evaluation, per view (include/scg_eval.h).
//
//   render.py:143      depth.min(), depth.max()                                   -> depth_range_kernel / depth_range_reduce_kernel
//   render.py:143-156  normalised depth, get_pixel_loss (utils/loss_utils.py:162-205), the five save_image calls
//   metrics.py:26-47   the PNGs read back, image * mask + (1 - mask), mask == 1.
//   metrics.py:89      the sums under the PSNR                                    -> eval_view_kernel
//
// One thread per pixel, one workgroup per kTileW x kTileH pixel tile.  The error map needs the 5x5 neighbourhood of a pixel in the
// six planes of render and ground truth: a workgroup stages its tile of them in LDS with a halo of 2, reflected at the image border
// (ReflectionPad2d(2)), and every other input is read once by the pixel's own thread.  No workgroup waits for another.
//
// Compiled with -ffp-contract=off: the masked images fl(fl(a * m) + fl(1 - m)) are held bit for bit to torch's separately rounded
// operators, and the error map's products are rounded before they are summed, as torch's x ** 2 and x * y are (the quantiser of
// pixel_rules.h pins its own two roundings).  Divisions are the correctly rounded __fdiv_rn (seed.hip).
//
// S and K are integers: a workgroup adds its pixels' in 32 bits (at most 256 * 3 * 255^2 < 2^26) and issues one 64-bit atomic each;
// the totals are exact in any order.
#include <math.h>

#include "scg_common.h"
#include "reduce.h"
#include "pixel_rules.h"
#include "../../include/scg_eval.h"

namespace scg {

constexpr int kTileW = 32, kTileH = 8;           // kBlock pixels: a wave reads two 32-float rows of the LDS tile, free of conflicts
constexpr int kHalo = 2;                         // ReflectionPad2d(2) in front of AvgPool2d(5, 1)
constexpr int kLdsW = kTileW + 2 * kHalo, kLdsH = kTileH + 2 * kHalo;
constexpr int kRangeChunk = 4096;                // depths a workgroup of the range kernel reads
constexpr int kRangeReduceBlock = 1024;
static_assert(kTileW * kTileH == kBlock, "one thread per pixel of the tile");

// (min, max) over the workgroup of NW waves in the order of reduce.h, one barrier; every thread gets the result
template <int NW>
__device__ __forceinline__ float2 wg_min_max(float mn, float mx, float (*s_red)[NW]) {
    wave_publish(mn, mx, s_red[0], s_red[1], NanMin(), NanMax());
    __syncthreads();
    return make_float2(wg_fold<NW>(s_red[0], NanMin()), wg_fold<NW>(s_red[1], NanMax()));
}

__global__ __launch_bounds__(kBlock) void depth_range_kernel(const float* __restrict__ depth, int64_t n, float2* __restrict__ partials) {
    __shared__ float s_red[2][kBlock / kWave];
    const int64_t base = (int64_t)blockIdx.x * kRangeChunk + threadIdx.x;
    float mn = INFINITY, mx = -INFINITY;
#pragma unroll
    for (int k = 0; k < kRangeChunk / kBlock; ++k) {
        const int64_t i = base + (int64_t)k * kBlock;
        if (i < n) { const float v = depth[i]; mn = nan_min(mn, v); mx = nan_max(mx, v); }
    }
    const float2 t = wg_min_max<kBlock / kWave>(mn, mx, s_red);
    if (threadIdx.x == 0) partials[blockIdx.x] = t;
}

__global__ __launch_bounds__(kRangeReduceBlock) void depth_range_reduce_kernel(const float2* __restrict__ partials, int chunks,
                                                                               float* __restrict__ range) {
    __shared__ float s_red[2][kRangeReduceBlock / kWave];
    float mn = INFINITY, mx = -INFINITY;
    for (int i = threadIdx.x; i < chunks; i += kRangeReduceBlock) { const float2 p = partials[i]; mn = nan_min(mn, p.x); mx = nan_max(mx, p.y); }
    const float2 t = wg_min_max<kRangeReduceBlock / kWave>(mn, mx, s_red);
    if (threadIdx.x == 0) { range[0] = t.x; range[1] = t.y; }
}

// index i of a reflection-padded axis of n >= 3 entries, i in [-2, n + 1]; the tile's overhang past the image is pinned to the
// last entry (no pixel inside the image reads those slots)
__device__ __forceinline__ int reflect(int i, int n) {
    const int r = i < 0 ? -i : (i >= n ? 2 * n - 2 - i : i);
    return min(max(r, 0), n - 1);
}

__global__ __launch_bounds__(kBlock) void eval_view_kernel(const float* __restrict__ render, const float* __restrict__ gt,
                                                           const float* __restrict__ depth, const float* __restrict__ dtumask,
                                                           const float* __restrict__ range, int H, int W,
                                                           uint8_t* __restrict__ render_u8, uint8_t* __restrict__ gt_u8,
                                                           uint8_t* __restrict__ depth_u8, uint8_t* __restrict__ error_u8,
                                                           uint8_t* __restrict__ mask_u8, float* __restrict__ error_f32,
                                                           float* __restrict__ render_masked, float* __restrict__ gt_masked,
                                                           unsigned long long* __restrict__ sk) {
    __shared__ float s_in[6][kLdsH][kLdsW];            // render 0..2, ground truth 3..5
    __shared__ uint32_t s_red[2][kBlock / kWave];
    const int x0 = blockIdx.x * kTileW, y0 = blockIdx.y * kTileH;
    const size_t plane = (size_t)H * W;
    for (int i = threadIdx.x; i < kLdsH * kLdsW; i += kBlock) {
        const int ly = i / kLdsW, lx = i - ly * kLdsW;
        const size_t p = (size_t)reflect(y0 + ly - kHalo, H) * W + reflect(x0 + lx - kHalo, W);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            s_in[c][ly][lx] = render[c * plane + p];
            s_in[3 + c][ly][lx] = gt[c * plane + p];
        }
    }
    __syncthreads();
    const int tx = threadIdx.x % kTileW, ty = threadIdx.x / kTileW;
    const int x = x0 + tx, y = y0 + ty;
    uint32_t s = 0, k = 0;
    if (x < W && y < H) {
        const size_t p = (size_t)y * W + x;
        uint32_t qm = 255u;
        if (dtumask) { qm = quantise(dtumask[p]); mask_u8[p] = (uint8_t)qm; }
        const float m = __fdiv_rn((float)qm, 255.f), one_minus_m = 1.f - m;
        float abs_sum = 0.f, ssim_sum = 0.f;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            // utils/loss_utils.py:176-193 without a mask: AvgPool2d(5, 1) is the sum of the 25 taps divided by 25
            float sx = 0.f, sy = 0.f, sxx = 0.f, syy = 0.f, sxy = 0.f;
#pragma unroll
            for (int dy = 0; dy < 5; ++dy) {
#pragma unroll
                for (int dx = 0; dx < 5; ++dx) {
                    const float a = s_in[c][ty + dy][tx + dx], b = s_in[3 + c][ty + dy][tx + dx];
                    sx += a; sy += b; sxx += a * a; syy += b * b; sxy += a * b;
                }
            }
            const float mu_x = __fdiv_rn(sx, 25.f), mu_y = __fdiv_rn(sy, 25.f);
            const float sigma_x = __fdiv_rn(sxx, 25.f) - mu_x * mu_x;
            const float sigma_y = __fdiv_rn(syy, 25.f) - mu_y * mu_y;
            const float sigma_xy = __fdiv_rn(sxy, 25.f) - mu_x * mu_y;
            const float ssim_n = (2.f * mu_x * mu_y + 1e-4f) * (2.f * sigma_xy + 9e-4f);
            const float ssim_d = (mu_x * mu_x + mu_y * mu_y + 1e-4f) * (sigma_x + sigma_y + 9e-4f);
            ssim_sum += unit_clamp((1.f - __fdiv_rn(ssim_n, ssim_d)) * 0.5f);
            const float r = s_in[c][ty + kHalo][tx + kHalo], g = s_in[3 + c][ty + kHalo][tx + kHalo];
            abs_sum += fabsf(r - g);
            // what the PNGs hold, and what metrics.py makes of them
            const uint32_t qr = quantise(r), qg = quantise(g);
            render_u8[p * 3 + c] = (uint8_t)qr;
            gt_u8[p * 3 + c] = (uint8_t)qg;
            render_masked[c * plane + p] = __fdiv_rn((float)qr, 255.f) * m + one_minus_m;
            gt_masked[c * plane + p] = __fdiv_rn((float)qg, 255.f) * m + one_minus_m;
            const int d = (int)qr - (int)qg;
            s += (uint32_t)(d * d);
        }
        if (qm == 255u) k = 3u; else s = 0u;           // metrics.py:42: mask == 1.
        // get_pixel_loss: l1 * 0.5 + ssim_l.mean(dim=0) * 0.5
        const float err = __fdiv_rn(abs_sum, 3.f) * 0.5f + __fdiv_rn(ssim_sum, 3.f) * 0.5f;
        if (error_f32) error_f32[p] = err;
        error_u8[p] = (uint8_t)quantise(err);
        // render.py:143
        const float lo = range[0], hi = range[1];
        depth_u8[p] = (uint8_t)quantise(__fdiv_rn(depth[p] - lo, hi - lo));
    }
    wave_publish(s, k, s_red[0], s_red[1], Sum(), Sum());
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint32_t ts = wg_fold<kBlock / kWave>(s_red[0], Sum()), tk = wg_fold<kBlock / kWave>(s_red[1], Sum());
        if (ts) atomicAdd(&sk[0], (unsigned long long)ts);
        if (tk) atomicAdd(&sk[1], (unsigned long long)tk);
    }
}

static int64_t range_chunks(int64_t n) { return (n + kRangeChunk - 1) / kRangeChunk; }

}  // namespace scg

using namespace scg;

extern "C" {

size_t scg_eval_depth_range_scratch_bytes(int64_t n) {
    if (n <= 0) return 256;
    return (size_t)range_chunks(n) * sizeof(float2) + 256;
}

int scg_eval_depth_range(const float* depth, int64_t n, float* range, void* scratch, size_t scratch_bytes, void* stream) {
    if (n <= 0 || n >= (1ll << 31)) return fail(SCG_E_RANGE, "eval_depth_range: n out of range");
    if (!depth || !range || !scratch) return fail(SCG_E_NULL, "eval_depth_range pointer is NULL");
    if (scratch_bytes < scg_eval_depth_range_scratch_bytes(n)) return fail(SCG_E_SCRATCH, "eval depth range scratch too small");
    if (reinterpret_cast<uintptr_t>(scratch) % 8) return fail(SCG_E_ALIGN, "eval depth range scratch not 8-byte aligned");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    float2* partials = reinterpret_cast<float2*>(scratch);
    const int chunks = (int)range_chunks(n);
    hipLaunchKernelGGL(depth_range_kernel, dim3(chunks), dim3(kBlock), 0, s, depth, n, partials);
    hipLaunchKernelGGL(depth_range_reduce_kernel, dim3(1), dim3(kRangeReduceBlock), 0, s, partials, chunks, range);
    return check_hip(hipGetLastError(), "eval_depth_range");
}

int32_t scg_eval_view_tile(int32_t axis) { return axis == 0 ? kTileW : (axis == 1 ? kTileH : 0); }

int scg_eval_view(const float* render, const float* gt, const float* depth, const float* dtumask, const float* range, int32_t H,
                  int32_t W, uint8_t* render_u8, uint8_t* gt_u8, uint8_t* depth_u8, uint8_t* error_u8, uint8_t* mask_u8,
                  float* error_f32, float* render_masked, float* gt_masked, uint64_t* sk, void* stream) {
    if (H < 3 || W < 3) return fail(SCG_E_RANGE, "eval_view: %d x %d is smaller than 3 x 3 (the reflection pad of 2 needs 3 rows and columns)", H, W);
    if ((int64_t)H * W >= (1ll << 31) || (H + kTileH - 1) / kTileH > 65535) return fail(SCG_E_RANGE, "eval_view: image dims out of range");
    if (!render || !gt || !depth || !range || !render_u8 || !gt_u8 || !depth_u8 || !error_u8 || !render_masked || !gt_masked || !sk)
        return fail(SCG_E_NULL, "eval_view pointer is NULL");
    if (dtumask && !mask_u8) return fail(SCG_E_NULL, "eval_view: mask_u8 is NULL with a dtumask");
    if (reinterpret_cast<uintptr_t>(sk) % 8) return fail(SCG_E_ALIGN, "eval_view: sk not 8-byte aligned");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    int rc = check_hip(hipMemsetAsync(sk, 0, 2 * sizeof(uint64_t), s), "eval_view sums reset");
    if (rc) return rc;
    const dim3 grid((W + kTileW - 1) / kTileW, (H + kTileH - 1) / kTileH);
    hipLaunchKernelGGL(eval_view_kernel, grid, dim3(kBlock), 0, s, render, gt, depth, dtumask, range, H, W, render_u8, gt_u8, depth_u8,
                       error_u8, mask_u8, error_f32, render_masked, gt_masked, reinterpret_cast<unsigned long long*>(sk));
    return check_hip(hipGetLastError(), "eval_view_kernel");
}

}  // extern "C"

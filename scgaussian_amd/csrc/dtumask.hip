// dtumask.hip — what the reference's training loop does only on DTU scenes (include/scg_loss.h, "DTU scenes").
//
//   train.py:149-158  background mask of the ground truth, ground truth zeroed under it      -> dtu_bg_mask_kernel
//   train.py:167-168  loss += rendered_alpha[bg_mask].mean()                                 -> masked_sum / masked_mean_reduce /
//                                                                                               masked_mean_backward kernels
//   train.py:252-265  clamped L1 and PSNR under `dtumask > 0`                                -> eval_metrics kernels
//
// The mask rule in closed form: mask[y, x] = dark(y, x) and (the run of dark pixels ending at row y in column x) >= min(y + 1, run),
// dark = max over the channels < thr.  The reference's loop ANDs the dark map with itself shifted down by 1 .. run - 1 rows, a
// shift past the top taking nothing away — the same statement.  Every column is independent and a row needs the run - 1 rows
// above it, so a thread owns one column of one row segment and re-reads up to run - 1 rows above the segment for its seed: loads
// coalesce along x, no workgroup waits for another.  Comparisons only: exact.
//
// The sums follow loss.hip: per-workgroup partial sums, then ONE workgroup adds them, all in the fixed order of reduce.h.
// All three are bandwidth-trivial next to a render (one or two reads per pixel); what they replace is a hundred launches and three
// host reads per iteration.
#include <math.h>

#include "scg_common.h"
#include "reduce.h"
#include "pixel_rules.h"
#include "../../include/scg_loss.h"

namespace scg {

constexpr int kMaskSegRows = 32;                 // rows of a mask segment: 1600 x 1200 -> 7 x 38 workgroups
constexpr int kChunk = 4096;                     // elements a workgroup of the sums reads
constexpr int kPerThread = kChunk / kBlock;      // 16, all loaded before the first is used
constexpr int kReduceBlock = 1024;
constexpr int kMaxMetricChannels = 16;

// ---- background mask --------------------------------------------------------------------------------------------------------
// `out` may be `gt` itself: a pixel is read by its own thread before that thread writes it, and by the threads of the segments
// below as part of their seed — those see the old value or 0, both dark when thr > 0 (the host side refuses thr <= 0 then).
__global__ __launch_bounds__(kBlock) void dtu_bg_mask_kernel(const float* gt, int H, int W, float thr, int run,
                                                             uint8_t* __restrict__ mask, float* out, uint32_t* __restrict__ count) {
    __shared__ uint32_t s_red[kBlock / kWave];
    const int x = blockIdx.x * kBlock + threadIdx.x;
    const int y0 = blockIdx.y * kMaskSegRows;
    const int y1 = min(y0 + kMaskSegRows, H);
    const size_t plane = (size_t)H * W;
    uint32_t n = 0;
    if (x < W) {
        int len = 0;                                      // dark pixels in a row, ending at the row above the current one
        for (int y = max(y0 - (run - 1), 0); y < y0; ++y) {
            const size_t p = (size_t)y * W + x;
            const bool dark = gt[p] < thr && gt[plane + p] < thr && gt[2 * plane + p] < thr;
            len = dark ? len + 1 : 0;
        }
        for (int y = y0; y < y1; ++y) {
            const size_t p = (size_t)y * W + x;
            const float r = gt[p], g = gt[plane + p], b = gt[2 * plane + p];
            const bool dark = r < thr && g < thr && b < thr;        // max(r, g, b) < thr; a NaN channel is not dark, as in torch
            len = dark ? len + 1 : 0;
            const bool m = len >= min(y + 1, run);
            mask[p] = m ? 1 : 0;
            out[p] = m ? 0.f : r; out[plane + p] = m ? 0.f : g; out[2 * plane + p] = m ? 0.f : b;
            n += m ? 1u : 0u;
        }
    }
    const uint32_t total = wg_reduce<kBlock / kWave>(n, s_red, Sum());
    if (threadIdx.x == 0 && total) atomicAdd(count, total);         // integers: the sum does not depend on the order
}

// ---- masked mean ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void masked_sum_kernel(const float* __restrict__ x, const uint8_t* __restrict__ mask, int64_t n,
                                                            float* __restrict__ partials) {
    __shared__ float s_red[kBlock / kWave];
    const int64_t base = (int64_t)blockIdx.x * kChunk + threadIdx.x;
    float v[kPerThread];
    uint8_t m[kPerThread];
#pragma unroll
    for (int k = 0; k < kPerThread; ++k) {
        const int64_t i = min(base + (int64_t)k * kBlock, n - 1);
        v[k] = x[i]; m[k] = mask[i];
    }
    float acc = 0.f;
#pragma unroll
    for (int k = 0; k < kPerThread; ++k) acc += (base + (int64_t)k * kBlock < n && m[k]) ? v[k] : 0.f;      // selected, not multiplied
    const float total = wg_reduce<kBlock / kWave>(acc, s_red, Sum());
    if (threadIdx.x == 0) partials[blockIdx.x] = total;
}

__global__ __launch_bounds__(kReduceBlock) void masked_mean_reduce_kernel(const float* __restrict__ partials, int n,
                                                                          const uint32_t* __restrict__ count, float* __restrict__ out) {
    __shared__ float s_red[kReduceBlock / kWave];
    float a = 0.f;
    for (int i = threadIdx.x; i < n; i += kReduceBlock) a += partials[i];
    const float total = wg_reduce<kReduceBlock / kWave>(a, s_red, Sum());
    if (threadIdx.x == 0) {
        const uint32_t c = count[0];
        out[0] = c ? total / (float)c : __builtin_nanf("");          // torch: the mean of an empty selection is NaN
    }
}

__global__ __launch_bounds__(kBlock) void masked_mean_backward_kernel(const uint8_t* __restrict__ mask, int64_t n,
                                                                      const uint32_t* __restrict__ count,
                                                                      const float* __restrict__ upstream, float* __restrict__ d_x) {
    const uint32_t c = count[0];
    const float g = c ? upstream[0] / (float)c : 0.f;               // correctly rounded: the fp32 quotient torch forms
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) d_x[i] = mask[i] ? g : 0.f;
}

// ---- evaluation metrics -----------------------------------------------------------------------------------------------------
// grid (chunks, C): partials[c * chunks + chunk] = (sum |a - b|, sum (a - b)^2) over the selected pixels of the chunk
__global__ __launch_bounds__(kBlock) void eval_metrics_kernel(const float* __restrict__ img, const float* __restrict__ gt,
                                                              const float* __restrict__ mask, int64_t hw, float2* __restrict__ partials,
                                                              uint32_t* __restrict__ selected) {
    __shared__ float s_red[kBlock / kWave];
    __shared__ uint32_t s_cnt[kBlock / kWave];
    const int c = blockIdx.y;
    const int64_t base = (int64_t)blockIdx.x * kChunk + threadIdx.x;
    const size_t plane = (size_t)c * hw;
    float a[kPerThread], b[kPerThread], m[kPerThread];
#pragma unroll
    for (int k = 0; k < kPerThread; ++k) {
        const int64_t i = min(base + (int64_t)k * kBlock, hw - 1);
        a[k] = img[plane + i]; b[k] = gt[plane + i]; m[k] = mask ? mask[i] : 1.f;
    }
    float sa = 0.f, sq = 0.f;
    uint32_t n = 0;
#pragma unroll
    for (int k = 0; k < kPerThread; ++k) {
        const bool sel = base + (int64_t)k * kBlock < hw && m[k] > 0.f;
        const float d = unit_clamp(a[k]) - unit_clamp(b[k]);
        sa += sel ? fabsf(d) : 0.f;
        sq += sel ? d * d : 0.f;
        n += sel ? 1u : 0u;
    }
    const float t_a = wg_reduce<kBlock / kWave>(sa, s_red, Sum());
    const float t_q = wg_reduce<kBlock / kWave>(sq, s_red, Sum());
    const uint32_t t_n = wg_reduce<kBlock / kWave>(n, s_cnt, Sum());
    if (threadIdx.x == 0) {
        partials[(size_t)c * gridDim.x + blockIdx.x] = make_float2(t_a, t_q);
        if (c == 0) selected[blockIdx.x] = t_n;
    }
}

// out[0] = l1, out[1] = psnr, out[2 + c] = mse[c]
__global__ __launch_bounds__(kReduceBlock) void eval_metrics_reduce_kernel(const float2* __restrict__ partials,
                                                                           const uint32_t* __restrict__ selected, int chunks, int C,
                                                                           float* __restrict__ out) {
    __shared__ float s_red[kReduceBlock / kWave];
    __shared__ uint32_t s_cnt[kReduceBlock / kWave];
    uint32_t n = 0;
    for (int i = threadIdx.x; i < chunks; i += kReduceBlock) n += selected[i];
    const uint32_t count = wg_reduce<kReduceBlock / kWave>(n, s_cnt, Sum());
    float abs_all = 0.f, psnr_all = 0.f;
    for (int c = 0; c < C; ++c) {
        float a = 0.f, q = 0.f;
        for (int i = threadIdx.x; i < chunks; i += kReduceBlock) { const float2 p = partials[(size_t)c * chunks + i]; a += p.x; q += p.y; }
        const float t_a = wg_reduce<kReduceBlock / kWave>(a, s_red, Sum());
        const float t_q = wg_reduce<kReduceBlock / kWave>(q, s_red, Sum());
        // utils/image_utils.py:18-19 per channel
        const float mse = count ? t_q / (float)count : __builtin_nanf("");
        abs_all += t_a;
        psnr_all += 20.f * log10f(1.0f / sqrtf(mse));
        if (threadIdx.x == 0) out[2 + c] = mse;
    }
    if (threadIdx.x == 0) {
        out[0] = count ? abs_all / ((float)C * (float)count) : __builtin_nanf("");
        out[1] = psnr_all / (float)C;
    }
}

static int64_t chunks_of(int64_t n) { return (n + kChunk - 1) / kChunk; }

static int check_plane(int32_t H, int32_t W) {
    if (H <= 0 || W <= 0 || (int64_t)H * W >= (1ll << 31)) return fail(SCG_E_RANGE, "image dims out of range");
    return 0;
}

}  // namespace scg

using namespace scg;

extern "C" {

int32_t scg_dtu_bg_mask_segment_rows(void) { return kMaskSegRows; }

int scg_dtu_bg_mask(const float* gt, int32_t H, int32_t W, float thr, int32_t run, uint8_t* mask, float* gt_masked, uint32_t* count,
                    void* stream) {
    int rc = check_plane(H, W);
    if (rc) return rc;
    if ((H + kMaskSegRows - 1) / kMaskSegRows > 65535) return fail(SCG_E_RANGE, "image height out of range");
    if (!gt || !mask || !gt_masked || !count) return fail(SCG_E_NULL, "dtu_bg_mask pointer is NULL");
    if (run < 1) return fail(SCG_E_RANGE, "run = %d < 1", run);
    if (thr != thr) return fail(SCG_E_RANGE, "thr is NaN");
    const size_t n3 = (size_t)3 * H * W;
    if (gt_masked == gt) {
        if (!(thr > 0.f)) return fail(SCG_E_RANGE, "gt_masked may alias gt only with thr > 0 (a zeroed pixel must stay dark)");
    } else if (gt_masked < gt + n3 && gt < gt_masked + n3) {
        return fail(SCG_E_RANGE, "gt_masked overlaps gt without being gt");
    }
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    rc = check_hip(hipMemsetAsync(count, 0, sizeof(uint32_t), s), "dtu_bg_mask count reset");
    if (rc) return rc;
    const dim3 grid((W + kBlock - 1) / kBlock, (H + kMaskSegRows - 1) / kMaskSegRows);
    hipLaunchKernelGGL(dtu_bg_mask_kernel, grid, dim3(kBlock), 0, s, gt, H, W, thr, run, mask, gt_masked, count);
    return check_hip(hipGetLastError(), "dtu_bg_mask_kernel");
}

size_t scg_masked_mean_scratch_bytes(int64_t n) {
    if (n <= 0) return 256;
    return (size_t)chunks_of(n) * sizeof(float) + 256;
}

int scg_masked_mean_forward(const float* x, const uint8_t* mask, int64_t n, const uint32_t* count, float* out, void* scratch,
                            size_t scratch_bytes, void* stream) {
    if (n <= 0 || n >= (1ll << 31)) return fail(SCG_E_RANGE, "masked_mean: n out of range");
    if (!x || !mask || !count || !out || !scratch) return fail(SCG_E_NULL, "masked_mean_forward pointer is NULL");
    if (scratch_bytes < scg_masked_mean_scratch_bytes(n)) return fail(SCG_E_SCRATCH, "masked mean scratch too small");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    float* partials = reinterpret_cast<float*>(scratch);
    const int chunks = (int)chunks_of(n);
    hipLaunchKernelGGL(masked_sum_kernel, dim3(chunks), dim3(kBlock), 0, s, x, mask, n, partials);
    hipLaunchKernelGGL(masked_mean_reduce_kernel, dim3(1), dim3(kReduceBlock), 0, s, partials, chunks, count, out);
    return check_hip(hipGetLastError(), "masked_mean_forward");
}

int scg_masked_mean_backward(const uint8_t* mask, int64_t n, const uint32_t* count, const float* upstream, float* d_x, void* stream) {
    if (n <= 0 || n >= (1ll << 31)) return fail(SCG_E_RANGE, "masked_mean: n out of range");
    if (!mask || !count || !upstream || !d_x) return fail(SCG_E_NULL, "masked_mean_backward pointer is NULL");
    const int64_t want = (n + kBlock * 4 - 1) / (kBlock * 4);
    const int blocks = (int)(want < 2048 ? want : 2048);
    hipLaunchKernelGGL(masked_mean_backward_kernel, dim3(blocks), dim3(kBlock), 0, reinterpret_cast<hipStream_t>(stream), mask, n,
                       count, upstream, d_x);
    return check_hip(hipGetLastError(), "masked_mean_backward_kernel");
}

static int check_metric_dims(int32_t C, int32_t H, int32_t W) {
    if (C <= 0 || C > kMaxMetricChannels) return fail(SCG_E_RANGE, "eval_metrics: C = %d not in 1..%d", C, kMaxMetricChannels);
    return check_plane(H, W);
}

size_t scg_eval_metrics_scratch_bytes(int32_t C, int32_t H, int32_t W) {
    if (C <= 0 || H <= 0 || W <= 0) return 256;
    const size_t chunks = (size_t)chunks_of((int64_t)H * W);
    return chunks * C * sizeof(float2) + chunks * sizeof(uint32_t) + 256;
}

int scg_eval_metrics(const float* img, const float* gt, const float* mask, int32_t C, int32_t H, int32_t W, float* out, void* scratch,
                     size_t scratch_bytes, void* stream) {
    int rc = check_metric_dims(C, H, W);
    if (rc) return rc;
    if (!img || !gt || !out || !scratch) return fail(SCG_E_NULL, "eval_metrics pointer is NULL");
    if (scratch_bytes < scg_eval_metrics_scratch_bytes(C, H, W)) return fail(SCG_E_SCRATCH, "eval metrics scratch too small");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const int64_t hw = (int64_t)H * W;
    const int chunks = (int)chunks_of(hw);
    float2* partials = reinterpret_cast<float2*>(scratch);
    uint32_t* selected = reinterpret_cast<uint32_t*>(partials + (size_t)chunks * C);
    hipLaunchKernelGGL(eval_metrics_kernel, dim3(chunks, C), dim3(kBlock), 0, s, img, gt, mask, hw, partials, selected);
    hipLaunchKernelGGL(eval_metrics_reduce_kernel, dim3(1), dim3(kReduceBlock), 0, s, partials, selected, chunks, C, out);
    return check_hip(hipGetLastError(), "eval_metrics");
}

}  // extern "C"

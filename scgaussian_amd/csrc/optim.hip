// optim.hip — the gradient consumers of a training step (include/scg_raster.h, "The training loop's gradient consumers").
//
// adam_step_kernel: torch's single-tensor Adam (weight_decay 0, no amsgrad, no maximize) over up to SCG_ADAM_MAX_SEGMENTS
// parameter tensors in ONE launch.  The segment table travels by value in the kernel arguments; each workgroup owns one chunk of
// kAdamChunk elements of one segment and streams it as float4 (scalar when a segment's pointers are not 16-byte aligned, and for
// the numel % 4 elements at its end).  Compiled with -ffp-contract=off: torch's order of operations, every operation rounded on
// its own.  The bits may differ from torch's where torch fuses (its lerp); tests/optim_refs.py restates what is computed here.
//
// Step counters live on the device (state['step']): every workgroup reads s and uses s+1; the LAST workgroup to finish writes
// s+1 back.  It learns that it is last from a device-scope ticket (release fence before the ticket add, acquire fence in the
// last arriver, which resets the ticket; the workspace starts zeroed).  Nothing else is handed between workgroups: the one other
// shared word per row segment, live_next, is only ever touched by atomics.
//
// The SH-tail skip (row segments: features_rest, 45 floats per Gaussian).  Invariant of the watermark live[seg]: in every row m
// and v are exact zeros at every column >= live.  Such an element costs a read of g alone when g == 0 (torch's update of it is an
// exact no-op: m = lerp(0, 0, w) = 0, v = 0, p + (-lr/bc1) * 0 / (0 + eps) = p), and is updated from m = v = 0 otherwise.  Every
// workgroup reduces the largest column whose new m or v is non-zero (+1) into live_next with atomicMax; the last arriver moves
// live_next into live (lowering it is safe there: every workgroup has read live by then).  The watermark is thereby re-derived
// exactly on every step and heals after any step that ran with SCG_ADAM_FORCE_FULL.
//
// densify_stats_kernel: the densification statistics of one render (train.py:191-192, gaussian_model.py:932-934), one thread per
// Gaussian, no atomics (each Gaussian's three words belong to its thread).
#include "scg_common.h"
#include "adam_math.h"

namespace scg {

constexpr int kAdamBlock = 256;
constexpr int kAdamChunk = kAdamBlock * 4 * 4;       // elements per workgroup: 4 float4 per thread
// workspace words: [0] ticket, [kWsLiveNext + i] live_next of slot i, [kWsLive + i] live of slot i
constexpr int kWsLiveNext = 16;
constexpr int kWsLive = 32;
constexpr size_t kAdamWsBytes = 256;

struct AdamSegDev {
    float* p;
    const float* g;
    float* m;
    float* v;
    float* step;
    int64_t numel;
    int32_t row_len;
    int32_t force;
    int32_t vec;                 // all four tensors 16-byte aligned
    int32_t first_block;         // first workgroup of this segment
    double lr, b1, b2;
    float w1, b2f, w2, eps;      // (float)(1 - b1), (float)b2, (float)(1 - b2), (float)eps: torch's Python scalars as fp32
};

struct AdamArgs {
    AdamSegDev seg[SCG_ADAM_MAX_SEGMENTS];
    int32_t nseg;
    int32_t work_blocks;
    const double* lr_table;      // nullptr: seg[i].lr
    uint32_t* ws;
};

// (AdamCoef, adam_bias_coefs and adam_update: adam_math.h, shared with the init stage)

__device__ __forceinline__ uint32_t live_col(float m, float v, uint32_t col) {
    return (m != 0.f || v != 0.f) ? col + 1 : 0u;
}

// one element of a row segment; col = its column
__device__ __forceinline__ void row_elem(const AdamSegDev& sg, int64_t i, uint32_t col, uint32_t live, const AdamCoef& c,
                                         uint32_t& top) {
    const float g = sg.g[i];
    float m = 0.f, v = 0.f;
    if (col < live) {
        m = sg.m[i];
        v = sg.v[i];
    } else if (g == 0.f) {
        return;
    }
    float p = sg.p[i];
    adam_update(p, m, v, g, c);
    sg.p[i] = p;
    sg.m[i] = m;
    sg.v[i] = v;
    top = max(top, live_col(m, v, col));
}

__device__ __forceinline__ void plain_elem(const AdamSegDev& sg, int64_t i, const AdamCoef& c) {
    float p = sg.p[i], m = sg.m[i], v = sg.v[i];
    adam_update(p, m, v, sg.g[i], c);
    sg.p[i] = p;
    sg.m[i] = m;
    sg.v[i] = v;
}

__global__ __launch_bounds__(kAdamBlock) void adam_step_kernel(AdamArgs a) {
    __shared__ uint32_t s_top[kAdamBlock / kWave];
    const int b = blockIdx.x;
    const int tid = threadIdx.x;
    uint32_t top = 0;
    int s = 0;
    bool rows = false;
    if (b < a.work_blocks) {
        while (s + 1 < a.nseg && a.seg[s + 1].first_block <= b) ++s;
        const AdamSegDev& sg = a.seg[s];
        // the step this launch takes, as torch forms it: step_t += 1 (fp32), then Python floats (double)
        const float step1 = sg.step[0] + 1.0f;
        const double lr = a.lr_table ? a.lr_table[s] : sg.lr;
        AdamCoef c;
        c.w1 = sg.w1; c.b2f = sg.b2f; c.w2 = sg.w2; c.eps = sg.eps;
        adam_bias_coefs(sg.b1, sg.b2, lr, (double)step1, c.bc2s, c.nss);
        const int64_t e0 = (int64_t)(b - sg.first_block) * kAdamChunk;
        const int64_t e1 = min(e0 + (int64_t)kAdamChunk, sg.numel);
        rows = sg.row_len > 0;
        if (!rows) {
            if (sg.vec) {
                const int64_t q1 = e1 >> 2;
                for (int64_t q = (e0 >> 2) + tid; q < q1; q += kAdamBlock) {
                    float4 p = reinterpret_cast<const float4*>(sg.p)[q];
                    float4 m = reinterpret_cast<const float4*>(sg.m)[q];
                    float4 v = reinterpret_cast<const float4*>(sg.v)[q];
                    const float4 g = reinterpret_cast<const float4*>(sg.g)[q];
                    adam_update(p.x, m.x, v.x, g.x, c);
                    adam_update(p.y, m.y, v.y, g.y, c);
                    adam_update(p.z, m.z, v.z, g.z, c);
                    adam_update(p.w, m.w, v.w, g.w, c);
                    reinterpret_cast<float4*>(sg.p)[q] = p;
                    reinterpret_cast<float4*>(sg.m)[q] = m;
                    reinterpret_cast<float4*>(sg.v)[q] = v;
                }
                const int64_t i = (q1 << 2) + tid;
                if (i < e1) plain_elem(sg, i, c);
            } else {
                for (int64_t i = e0 + tid; i < e1; i += kAdamBlock) plain_elem(sg, i, c);
            }
        } else {
            const uint32_t L = (uint32_t)sg.row_len;
            const uint32_t live = sg.force ? L : min(L, __hip_atomic_load(a.ws + kWsLive + s, __ATOMIC_RELAXED,
                                                                          __HIP_MEMORY_SCOPE_AGENT));
            if (sg.vec) {
                const int64_t q1 = e1 >> 2;
                for (int64_t q = (e0 >> 2) + tid; q < q1; q += kAdamBlock) {
                    uint32_t col[4];
                    col[0] = (uint32_t)((q << 2) % L);
                    for (int k = 1; k < 4; ++k) col[k] = col[k - 1] + 1 == L ? 0u : col[k - 1] + 1;
                    const float4 g4 = reinterpret_cast<const float4*>(sg.g)[q];
                    const bool any_live = col[0] < live || col[1] < live || col[2] < live || col[3] < live;
                    if (!any_live && g4.x == 0.f && g4.y == 0.f && g4.z == 0.f && g4.w == 0.f) continue;
                    float4 m4 = make_float4(0.f, 0.f, 0.f, 0.f), v4 = m4;
                    if (any_live) {             // the tail lanes of a mixed group hold zeros (the invariant)
                        m4 = reinterpret_cast<const float4*>(sg.m)[q];
                        v4 = reinterpret_cast<const float4*>(sg.v)[q];
                    }
                    float4 p4 = reinterpret_cast<const float4*>(sg.p)[q];
                    float pv[4] = {p4.x, p4.y, p4.z, p4.w}, mv[4] = {m4.x, m4.y, m4.z, m4.w};
                    float vv[4] = {v4.x, v4.y, v4.z, v4.w};
                    const float gv[4] = {g4.x, g4.y, g4.z, g4.w};
                    for (int k = 0; k < 4; ++k) {
                        adam_update(pv[k], mv[k], vv[k], gv[k], c);
                        top = max(top, live_col(mv[k], vv[k], col[k]));
                    }
                    reinterpret_cast<float4*>(sg.p)[q] = make_float4(pv[0], pv[1], pv[2], pv[3]);
                    reinterpret_cast<float4*>(sg.m)[q] = make_float4(mv[0], mv[1], mv[2], mv[3]);
                    reinterpret_cast<float4*>(sg.v)[q] = make_float4(vv[0], vv[1], vv[2], vv[3]);
                }
                const int64_t i = (q1 << 2) + tid;
                if (i < e1) row_elem(sg, i, (uint32_t)(i % L), live, c, top);
            } else {
                for (int64_t i = e0 + tid; i < e1; i += kAdamBlock) row_elem(sg, i, (uint32_t)(i % L), live, c, top);
            }
        }
    }
    // the workgroup's watermark: wave maximum, then one atomicMax per workgroup
    if (rows) {
        for (int off = kWave / 2; off > 0; off >>= 1) top = max(top, (uint32_t)__shfl_xor((int)top, off, kWave));
        if ((tid & (kWave - 1)) == 0) s_top[tid / kWave] = top;
    }
    __syncthreads();
    if (tid != 0) return;
    if (rows) {
        for (int w = 0; w < kAdamBlock / kWave; ++w) top = max(top, s_top[w]);
        if (top > 0) __hip_atomic_fetch_max(a.ws + kWsLiveNext + s, top, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    // the ticket: release (this workgroup's atomics and its reads of step / live are done), then one add
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    __builtin_amdgcn_s_waitcnt(0);
    const uint32_t ticket = __hip_atomic_fetch_add(a.ws, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (ticket != gridDim.x - 1) return;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    for (int k = 0; k < a.nseg; ++k) {
        const AdamSegDev& q = a.seg[k];
        q.step[0] = q.step[0] + 1.0f;
        if (q.row_len > 0) {
            const uint32_t nl = __hip_atomic_exchange(a.ws + kWsLiveNext + k, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(a.ws + kWsLive + k, nl, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    __hip_atomic_store(a.ws, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(kBlock) void densify_stats_kernel(int P, const int32_t* __restrict__ radii,
                                                               const float* __restrict__ g2d, int64_t stride,
                                                               float* __restrict__ accum, float* __restrict__ denom,
                                                               float* __restrict__ max_radii) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= P) return;
    const int r = radii[i];
    if (r <= 0) return;
    const float gx = g2d[(int64_t)i * stride], gy = g2d[(int64_t)i * stride + 1];
    accum[i] = accum[i] + sqrtf(gx * gx + gy * gy);
    denom[i] = denom[i] + 1.0f;
    max_radii[i] = fmaxf(max_radii[i], (float)r);
}

}  // namespace scg

using namespace scg;

extern "C" {

size_t scg_adam_workspace_bytes(int32_t nseg) {
    return (nseg >= 1 && nseg <= SCG_ADAM_MAX_SEGMENTS) ? kAdamWsBytes : 0;
}

int scg_adam_step(const ScgAdamSegment* segments, int32_t nseg, const double* lr_table, void* workspace,
                  size_t workspace_bytes, void* stream) {
    if (!segments) return fail(SCG_E_NULL, "adam: segment table is NULL");
    if (nseg < 1 || nseg > SCG_ADAM_MAX_SEGMENTS) return fail(SCG_E_RANGE, "adam: nseg = %d not in 1..%d", nseg, SCG_ADAM_MAX_SEGMENTS);
    if (!workspace) return fail(SCG_E_NULL, "adam: workspace is NULL");
    if (workspace_bytes < kAdamWsBytes) return fail(SCG_E_SCRATCH, "adam: workspace of %zu bytes < %zu", workspace_bytes, kAdamWsBytes);
    if (reinterpret_cast<uintptr_t>(workspace) % 4) return fail(SCG_E_ALIGN, "adam: workspace not 4-byte aligned");
    AdamArgs a;
    int64_t blocks = 0;
    for (int i = 0; i < nseg; ++i) {
        const ScgAdamSegment& s = segments[i];
        if (s.numel < 0) return fail(SCG_E_RANGE, "adam: segment %d: numel %lld < 0", i, (long long)s.numel);
        if (s.row_len < 0) return fail(SCG_E_RANGE, "adam: segment %d: row_len %d < 0", i, s.row_len);
        if (s.row_len > 0 && s.numel % s.row_len) return fail(SCG_E_RANGE, "adam: segment %d: numel is not a multiple of row_len", i);
        if (!s.step) return fail(SCG_E_NULL, "adam: segment %d: step is NULL", i);
        if (s.numel > 0 && (!s.param || !s.grad || !s.exp_avg || !s.exp_avg_sq))
            return fail(SCG_E_NULL, "adam: segment %d: a tensor pointer is NULL", i);
        if ((s.flags & ~SCG_ADAM_FORCE_FULL) != 0) return fail(SCG_E_RANGE, "adam: segment %d: unknown flags 0x%x", i, s.flags);
        AdamSegDev& d = a.seg[i];
        d.p = s.param; d.g = s.grad; d.m = s.exp_avg; d.v = s.exp_avg_sq; d.step = s.step;
        d.numel = s.numel;
        d.row_len = s.row_len;
        d.force = (s.flags & SCG_ADAM_FORCE_FULL) ? 1 : 0;
        d.vec = ((reinterpret_cast<uintptr_t>(s.param) | reinterpret_cast<uintptr_t>(s.grad) |
                  reinterpret_cast<uintptr_t>(s.exp_avg) | reinterpret_cast<uintptr_t>(s.exp_avg_sq)) % 16) == 0;
        d.first_block = (int32_t)blocks;
        d.lr = s.lr; d.b1 = s.beta1; d.b2 = s.beta2;
        d.w1 = (float)(1.0 - s.beta1);
        d.b2f = (float)s.beta2;
        d.w2 = (float)(1.0 - s.beta2);
        d.eps = (float)s.eps;
        blocks += (s.numel + kAdamChunk - 1) / kAdamChunk;
        if (blocks > 0x7FFFFFFFll) return fail(SCG_E_RANGE, "adam: too many elements");
    }
    for (int i = nseg; i < SCG_ADAM_MAX_SEGMENTS; ++i) a.seg[i] = AdamSegDev{};
    a.nseg = nseg;
    a.work_blocks = (int32_t)blocks;
    a.lr_table = lr_table;
    a.ws = reinterpret_cast<uint32_t*>(workspace);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const unsigned grid = blocks > 0 ? (unsigned)blocks : 1u;     // one workgroup at least: it advances the step counters
    hipLaunchKernelGGL(adam_step_kernel, dim3(grid), dim3(kAdamBlock), 0, st, a);
    return check_hip(hipGetLastError(), "adam_step");
}

int scg_densify_stats(int32_t P, const int32_t* radii, const float* means2D_grad, int64_t grad_row_stride, float* accum,
                      float* denom, float* max_radii2D, void* stream) {
    if (P < 0) return fail(SCG_E_RANGE, "densify_stats: P = %d < 0", P);
    if (grad_row_stride < 2) return fail(SCG_E_RANGE, "densify_stats: grad_row_stride %lld < 2", (long long)grad_row_stride);
    if (P == 0) return 0;
    if (!radii || !means2D_grad || !accum || !denom || !max_radii2D) return fail(SCG_E_NULL, "densify_stats: pointer is NULL");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(densify_stats_kernel, dim3((P + kBlock - 1) / kBlock), dim3(kBlock), 0, st, P, radii, means2D_grad,
                       grad_row_stride, accum, denom, max_radii2D);
    return check_hip(hipGetLastError(), "densify_stats");
}

}  // extern "C"

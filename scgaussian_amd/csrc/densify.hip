// densify.hip — densify-and-prune and the opacity reset (include/scg_raster.h, "Densify-and-prune and the opacity reset").
//
// The reference's rule (scene/gaussian_model.py:758-930) decides every source row from that row alone — the gradient test, the
// clone / split choice, and the final prune of the original, of its clone and of its children — so the whole call is three launches
// around ONE host read:
//
//   densify_classify_kernel   one thread per source: the fate byte (keep-original, clone-survives, children-survive, split) with
//                             the final prune folded in, and the workgroup's count of the first three
//   densify_scan_kernel       one workgroup: exclusive scan of the per-workgroup counts in workgroup order (compact.h: fixed order,
//                             no atomics), the section totals into the head of the workspace
//   (the caller reads the four totals and allocates the new background tensors)
//   densify_scatter_kernel    the same partition of the sources: ranks within the workgroup recomputed from the fate bits, every
//                             surviving row copied or computed at base + rank; the 45-float features_rest rows and their moments
//                             move with the lanes running across the floats of a row.  The same launch divides the raw scaling of
//                             split ray-bound sources, zeroes the ray optimizer's scaling moments and the new statistics tensors.
//
// Sources are read through the two-segment model (ray-bound set, then background set): no concatenated copy exists.  Compiled with
// -ffp-contract=off: the clone's xyz (one multiply, one add) and the divisions by 1.6 round where torch rounds them.
#include "compact.h"

namespace scg {

constexpr int kDnBlock = 256;
constexpr int kDnHeadWords = 8;                       // [0..3] section totals, [4..7] zero
constexpr int kDnRest = 45;                           // floats of a features_rest row
constexpr int32_t kDnMaxP = 1 << 29;                  // 3 P rows at most leave a call: they are counted in 32 bits
constexpr float kSplitShrink = 1.6f;                  // 0.8 * N of densify_and_split, N = 2

enum : uint32_t { kFateKeep = 1, kFateClone = 2, kFateChild = 4, kFateSplit = 8 };
enum { kTXyz = 0, kTDc = 1, kTRest = 2, kTOpacity = 3, kTScaling = 4, kTRotation = 5, kTensors = 6 };

__host__ __device__ inline int dn_groups(int P) { return (P + kDnBlock - 1) / kDnBlock; }
inline size_t dn_workspace_bytes(int P) {
    return (size_t)kDnHeadWords * 4 + (size_t)dn_groups(P) * 12 + (((size_t)P + 3) & ~(size_t)3);
}

struct DnClassifyArgs {
    ScgModel m;
    const float* accum;
    const float* denom;
    float max_grad, min_opacity, dense_scale, big_scale;
    int P;
    uint32_t* counts;
    uint8_t* fate;
};

struct DnScatterArgs {
    ScgModel m;
    float* out[kTensors];
    float* om[kTensors];              // exp_avg of the new set (nullptr: the group has no state)
    float* ov[kTensors];              // exp_avg_sq
    const float* im[kTensors];        // moments of the current background set
    const float* iv[kTensors];
    float* ray_scaling;
    float* ray_m;
    float* ray_v;
    float* accum;
    float* denom;
    float* max_radii;
    const float* noise;
    const uint32_t* head;
    const uint32_t* bases;
    const uint8_t* fate;
    int P;
    int out_rows;
};

// torch.max over a dimension: a NaN wins
__device__ __forceinline__ float max_nan(float a, float b) { return (a > b || a != a) ? a : b; }
__device__ __forceinline__ float max3_nan(float a, float b, float c) { return max_nan(max_nan(a, b), c); }
__device__ __forceinline__ float sigmoidf(float x) { return 1.0f / (1.0f + expf(-x)); }

// prune_mask of densify_and_prune for one background row
__device__ __forceinline__ bool pruned(float o, float smax, float min_opacity, float big_scale) {
    return (o < min_opacity) || (big_scale >= 0.0f && smax > big_scale);
}

__global__ __launch_bounds__(kDnBlock) void densify_classify_kernel(DnClassifyArgs a) {
    const int64_t i = (int64_t)blockIdx.x * kDnBlock + threadIdx.x;
    uint32_t f = 0;
    if (i < a.P) {
        const int nr = a.m.ray.count;
        const bool ray = i < nr;
        const ScgModelSet& st = ray ? a.m.ray : a.m.bg;
        const int64_t j = ray ? i : i - nr;
        float g = a.accum[i] / a.denom[i];
        if (g != g) g = 0.0f;                                             // grads[grads.isnan()] = 0; an inf stays
        const float e0 = expf(st.scaling[j * 3]), e1 = expf(st.scaling[j * 3 + 1]), e2 = expf(st.scaling[j * 3 + 2]);
        const float smax = max3_nan(e0, e1, e2);
        const float o = sigmoidf(st.opacity[j]);
        // the clone test takes the norm of the one-element gradient row (|g|), the split test the padded gradient itself
        const bool clone = fabsf(g) >= a.max_grad && smax <= a.dense_scale;
        const bool split = g >= a.max_grad && smax > a.dense_scale;
        const bool gone = pruned(o, smax, a.min_opacity, a.big_scale);
        if (!ray && !split && !gone) f |= kFateKeep;
        if (clone && !gone) f |= kFateClone;                              // the clone carries its source's opacity and scaling
        if (split) {
            f |= kFateSplit;
            // the children carry log(exp(s) / 1.6): the world-size term sees exp of that
            const float c0 = expf(logf(e0 / kSplitShrink)), c1 = expf(logf(e1 / kSplitShrink)), c2 = expf(logf(e2 / kSplitShrink));
            if (!pruned(o, max3_nan(c0, c1, c2), a.min_opacity, a.big_scale)) f |= kFateChild;
        }
        a.fate[i] = (uint8_t)f;
    }
    uint32_t rank[3], tot[3];
    block_counts<3, kDnBlock>(f, rank, tot);                              // bits 0..2: keep, clone, child
    if (threadIdx.x == 0)
        for (int k = 0; k < 3; ++k) a.counts[(int64_t)blockIdx.x * 3 + k] = tot[k];
}

// counts (groups x 3) -> exclusive bases in place, the section totals into the head
__global__ __launch_bounds__(kDnBlock) void densify_scan_kernel(uint32_t* head, uint32_t* counts, int groups) {
    uint32_t tot[3];
    carry_scan<3, kDnBlock>(counts, groups, tot);
    if (threadIdx.x == 0) {
        head[0] = tot[0];
        head[1] = tot[1];
        head[2] = tot[2];
        head[3] = tot[2];                                                 // the children of copy 1
        for (int k = 4; k < kDnHeadWords; ++k) head[k] = 0;
    }
}

// the W floats of tensor T of new row d: moments gathered from background row j, or zero for a new row (j < 0)
template <int T, int W>
__device__ __forceinline__ void put_moments(const DnScatterArgs& a, int64_t d, int64_t j) {
    if (!a.om[T]) return;
#pragma unroll
    for (int k = 0; k < W; ++k) {
        a.om[T][d * W + k] = j >= 0 ? a.im[T][j * W + k] : 0.0f;
        a.ov[T][d * W + k] = j >= 0 ? a.iv[T][j * W + k] : 0.0f;
    }
}

struct DnRow {                        // the 14 floats of a row outside features_rest
    float xyz[3], dc[3], opacity, scaling[3], rotation[4];
};

__device__ __forceinline__ void put_row(const DnScatterArgs& a, int64_t d, const DnRow& r, int64_t moments_from) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        a.out[kTXyz][d * 3 + k] = r.xyz[k];
        a.out[kTDc][d * 3 + k] = r.dc[k];
        a.out[kTScaling][d * 3 + k] = r.scaling[k];
    }
    a.out[kTOpacity][d] = r.opacity;
#pragma unroll
    for (int k = 0; k < 4; ++k) a.out[kTRotation][d * 4 + k] = r.rotation[k];
    put_moments<kTXyz, 3>(a, d, moments_from);
    put_moments<kTDc, 3>(a, d, moments_from);
    put_moments<kTOpacity, 1>(a, d, moments_from);
    put_moments<kTScaling, 3>(a, d, moments_from);
    put_moments<kTRotation, 4>(a, d, moments_from);
}

__global__ __launch_bounds__(kDnBlock) void densify_scatter_kernel(DnScatterArgs a) {
    __shared__ int32_t s_dst[4][kDnBlock];                               // keep, clone, child 0, child 1: new row or -1
    const int tid = threadIdx.x;
    const int64_t g0 = (int64_t)blockIdx.x * kDnBlock;
    const int nr = a.m.ray.count;
    if (g0 < a.P) {                                                       // (uniform: the whole workgroup or none of it)
        const int64_t i = g0 + tid;
        const uint32_t f = i < a.P ? a.fate[i] : 0u;
        uint32_t v[3], tot[3];
        block_counts<3, kDnBlock>(f, v, tot);                             // v: the rank among the workgroup's keeps, clones, children
        const uint32_t K = a.head[0], C = a.head[1], S = a.head[2];
        const uint32_t* b = a.bases + (int64_t)blockIdx.x * 3;
        int64_t dst[4] = {-1, -1, -1, -1};
        if (f & kFateKeep) dst[0] = (int64_t)b[0] + v[0];
        if (f & kFateClone) dst[1] = (int64_t)K + b[1] + v[1];
        if (f & kFateChild) {
            dst[2] = (int64_t)K + C + b[2] + v[2];
            dst[3] = dst[2] + S;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (dst[k] >= a.out_rows) dst[k] = -1;                        // never beyond what the caller allocated
            s_dst[k][tid] = (int32_t)dst[k];
        }
        if (f) {
            const bool ray = i < nr;
            const ScgModelSet& st = ray ? a.m.ray : a.m.bg;
            const int64_t j = ray ? i : i - nr;
            DnRow r;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                r.xyz[k] = ray ? st.rayo[j * 3 + k] + st.rayd[j * 3 + k] * st.zval[j] : st.xyz[j * 3 + k];
                r.dc[k] = st.features_dc[j * 3 + k];
                r.scaling[k] = st.scaling[j * 3 + k];
            }
            r.opacity = st.opacity[j];
#pragma unroll
            for (int k = 0; k < 4; ++k) r.rotation[k] = st.rotation[j * 4 + k];
            if (dst[0] >= 0) put_row(a, dst[0], r, j);
            if (dst[1] >= 0) put_row(a, dst[1], r, -1);
            if (f & kFateSplit) {
                if (dst[2] >= 0 || dst[3] >= 0) {
                    // build_rotation (utils/general_utils.py:84-105): it normalises the quaternion itself
                    const float qr0 = r.rotation[0], qx0 = r.rotation[1], qy0 = r.rotation[2], qz0 = r.rotation[3];
                    const float norm = sqrtf(qr0 * qr0 + qx0 * qx0 + qy0 * qy0 + qz0 * qz0);
                    const float qr = qr0 / norm, x = qx0 / norm, y = qy0 / norm, z = qz0 / norm;
                    const float R[3][3] = {{1.0f - 2.0f * (y * y + z * z), 2.0f * (x * y - qr * z), 2.0f * (x * z + qr * y)},
                                           {2.0f * (x * y + qr * z), 1.0f - 2.0f * (x * x + z * z), 2.0f * (y * z - qr * x)},
                                           {2.0f * (x * z - qr * y), 2.0f * (y * z + qr * x), 1.0f - 2.0f * (x * x + y * y)}};
                    float e[3];
                    DnRow c = r;
#pragma unroll
                    for (int k = 0; k < 3; ++k) {
                        e[k] = expf(r.scaling[k]);
                        c.scaling[k] = logf(e[k] / kSplitShrink);
                    }
#pragma unroll
                    for (int copy = 0; copy < 2; ++copy) {
                        if (dst[2 + copy] < 0) continue;
                        const float* u = a.noise + ((int64_t)copy * a.P + i) * 3;
                        const float s0 = e[0] * u[0], s1 = e[1] * u[1], s2 = e[2] * u[2];
#pragma unroll
                        for (int k = 0; k < 3; ++k) c.xyz[k] = (R[k][0] * s0 + R[k][1] * s1 + R[k][2] * s2) + r.xyz[k];
                        put_row(a, dst[2 + copy], c, -1);
                    }
                }
                // a split ray-bound source stays; its RAW log-scale row is divided (the reference's own arithmetic)
                if (ray)
#pragma unroll
                    for (int k = 0; k < 3; ++k) a.ray_scaling[j * 3 + k] = r.scaling[k] / kSplitShrink;
            }
        }
        __syncthreads();
        // features_rest and its moments: the lanes run across the floats of the workgroup's rows
        const int rows = (int)min((int64_t)kDnBlock, (int64_t)a.P - g0);
        for (int e = tid; e < rows * kDnRest; e += kDnBlock) {
            const int r = e / kDnRest, col = e - r * kDnRest;
            const int32_t dk = s_dst[0][r], dc = s_dst[1][r], d0 = s_dst[2][r], d1 = s_dst[3][r];
            if ((dk & dc & d0 & d1) < 0) continue;                        // all four are -1
            const int64_t i = g0 + r;
            const bool ray = i < nr;
            const int64_t j = ray ? i : i - nr;
            const float val = (ray ? a.m.ray.features_rest : a.m.bg.features_rest)[j * kDnRest + col];
            if (dk >= 0) {
                const int64_t o = (int64_t)dk * kDnRest + col;
                a.out[kTRest][o] = val;
                if (a.om[kTRest]) {
                    a.om[kTRest][o] = a.im[kTRest][j * kDnRest + col];
                    a.ov[kTRest][o] = a.iv[kTRest][j * kDnRest + col];
                }
            }
            const int32_t fresh[3] = {dc, d0, d1};
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                if (fresh[k] < 0) continue;
                const int64_t o = (int64_t)fresh[k] * kDnRest + col;
                a.out[kTRest][o] = val;
                if (a.om[kTRest]) {
                    a.om[kTRest][o] = 0.0f;
                    a.ov[kTRest][o] = 0.0f;
                }
            }
        }
    }
    // the tensors that are zeroed whole, spread over the grid
    const int64_t gt = (int64_t)blockIdx.x * kDnBlock + tid, stride = (int64_t)gridDim.x * kDnBlock;
    if (a.ray_m)
        for (int64_t k = gt; k < (int64_t)nr * 3; k += stride) {
            a.ray_m[k] = 0.0f;
            a.ray_v[k] = 0.0f;
        }
    for (int64_t k = gt; k < (int64_t)nr + a.out_rows; k += stride) {
        a.accum[k] = 0.0f;
        a.denom[k] = 0.0f;
        a.max_radii[k] = 0.0f;
    }
}

__global__ __launch_bounds__(kDnBlock) void reset_opacity_kernel(int nr, float* ro, float* rm, float* rv, int nb, float* bo,
                                                                 float* bm, float* bv) {
    const int64_t i = (int64_t)blockIdx.x * kDnBlock + threadIdx.x;
    if (i >= (int64_t)nr + nb) return;
    const bool ray = i < nr;
    const int64_t j = ray ? i : i - nr;
    float* o = ray ? ro : bo;
    float* m = ray ? rm : bm;
    float* v = ray ? rv : bv;
    float s = sigmoidf(o[j]);
    s = (s < 0.01f || s != s) ? s : 0.01f;                                // torch.min(opacity, 0.01): a NaN stays
    o[j] = logf(s / (1.0f - s));                                          // inverse_sigmoid
    if (m) m[j] = 0.0f;
    if (v) v[j] = 0.0f;
}

static int validate_model(const char* who, const ScgModel* m) {
    if (!m) return fail(SCG_E_NULL, "%s: model is NULL", who);
    if (m->ray.count < 0 || m->bg.count < 0)
        return fail(SCG_E_RANGE, "%s: negative count (ray %d, bg %d)", who, m->ray.count, m->bg.count);
    if ((int64_t)m->ray.count + m->bg.count > kDnMaxP)
        return fail(SCG_E_RANGE, "%s: %lld sources > %d", who, (long long)m->ray.count + m->bg.count, kDnMaxP);
    return 0;
}

static int validate_model_pointers(const char* who, const ScgModel* m) {
    const ScgModelSet& r = m->ray;
    const ScgModelSet& b = m->bg;
    if (r.count > 0 && (!r.zval || !r.rayo || !r.rayd || !r.features_dc || !r.features_rest || !r.opacity || !r.scaling || !r.rotation))
        return fail(SCG_E_NULL, "%s: a tensor of the ray-bound set is NULL", who);
    if (b.count > 0 && (!b.xyz || !b.features_dc || !b.features_rest || !b.opacity || !b.scaling || !b.rotation))
        return fail(SCG_E_NULL, "%s: a tensor of the background set is NULL", who);
    return 0;
}

static void tensors_to_array(const ScgDensifyTensors& t, float* out[kTensors]) {
    out[kTXyz] = t.xyz; out[kTDc] = t.features_dc; out[kTRest] = t.features_rest;
    out[kTOpacity] = t.opacity; out[kTScaling] = t.scaling; out[kTRotation] = t.rotation;
}

}  // namespace scg

using namespace scg;

extern "C" {

size_t scg_densify_workspace_bytes(int32_t P) { return (P >= 0 && P <= kDnMaxP) ? dn_workspace_bytes(P) : 0; }

int scg_densify_classify(const ScgModel* model, const float* accum, const float* denom, float max_grad, float min_opacity,
                         float dense_scale, float big_scale, void* workspace, size_t workspace_bytes, void* stream) {
    if (int rc = validate_model("densify_classify", model)) return rc;
    if (!(max_grad > 0.0f)) return fail(SCG_E_RANGE, "densify_classify: max_grad = %g must be > 0", (double)max_grad);
    const int P = model->ray.count + model->bg.count;
    if (int rc = check_workspace("densify_classify", workspace, workspace_bytes, dn_workspace_bytes(P))) return rc;
    if (int rc = validate_model_pointers("densify_classify", model)) return rc;
    if (P > 0 && (!accum || !denom)) return fail(SCG_E_NULL, "densify_classify: accum / denom is NULL");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    uint32_t* head = reinterpret_cast<uint32_t*>(workspace);
    const int groups = dn_groups(P);
    DnClassifyArgs a;
    a.m = *model;
    a.accum = accum; a.denom = denom;
    a.max_grad = max_grad; a.min_opacity = min_opacity; a.dense_scale = dense_scale; a.big_scale = big_scale;
    a.P = P;
    a.counts = head + kDnHeadWords;
    a.fate = reinterpret_cast<uint8_t*>(a.counts + (size_t)groups * 3);
    if (groups > 0) {
        hipLaunchKernelGGL(densify_classify_kernel, dim3(groups), dim3(kDnBlock), 0, st, a);
        if (int rc = check_hip(hipGetLastError(), "densify_classify")) return rc;
    }
    hipLaunchKernelGGL(densify_scan_kernel, dim3(1), dim3(kDnBlock), 0, st, head, a.counts, groups);
    return check_hip(hipGetLastError(), "densify_scan");
}

int scg_densify_scatter(const ScgModel* model, const ScgDensifyScatter* args, const void* workspace, size_t workspace_bytes,
                        void* stream) {
    if (int rc = validate_model("densify_scatter", model)) return rc;
    if (!args) return fail(SCG_E_NULL, "densify_scatter: args is NULL");
    const int P = model->ray.count + model->bg.count;
    if (args->out_rows < 0 || (int64_t)args->out_rows > 3ll * P)
        return fail(SCG_E_RANGE, "densify_scatter: out_rows = %d not in 0..3 P", args->out_rows);
    if (int rc = check_workspace("densify_scatter", workspace, workspace_bytes, dn_workspace_bytes(P))) return rc;
    if (int rc = validate_model_pointers("densify_scatter", model)) return rc;
    DnScatterArgs a;
    a.m = *model;
    float *im[kTensors], *iv[kTensors];
    tensors_to_array(args->out, a.out);
    tensors_to_array(args->out_exp_avg, a.om);
    tensors_to_array(args->out_exp_avg_sq, a.ov);
    tensors_to_array(args->in_exp_avg, im);
    tensors_to_array(args->in_exp_avg_sq, iv);
    for (int t = 0; t < kTensors; ++t) {
        a.im[t] = im[t];
        a.iv[t] = iv[t];
        if (args->out_rows > 0 && !a.out[t]) return fail(SCG_E_NULL, "densify_scatter: output tensor %d is NULL", t);
        if ((a.om[t] == nullptr) != (a.ov[t] == nullptr))
            return fail(SCG_E_NULL, "densify_scatter: tensor %d has one output moment but not the other", t);
        if (a.om[t] && model->bg.count > 0 && (!im[t] || !iv[t]))
            return fail(SCG_E_NULL, "densify_scatter: tensor %d has output moments but no input moments", t);
    }
    if (model->ray.count > 0 && args->ray_scaling != model->ray.scaling)
        return fail(SCG_E_RANGE, "densify_scatter: ray_scaling is not the model's ray-bound scaling tensor");
    if ((args->ray_scaling_exp_avg == nullptr) != (args->ray_scaling_exp_avg_sq == nullptr))
        return fail(SCG_E_NULL, "densify_scatter: one ray scaling moment without the other");
    if ((int64_t)model->ray.count + args->out_rows > 0 && (!args->accum || !args->denom || !args->max_radii2D))
        return fail(SCG_E_NULL, "densify_scatter: a statistics tensor is NULL");
    if (P > 0 && !args->noise) return fail(SCG_E_NULL, "densify_scatter: noise is NULL");
    a.ray_scaling = args->ray_scaling;
    a.ray_m = model->ray.count > 0 ? args->ray_scaling_exp_avg : nullptr;
    a.ray_v = model->ray.count > 0 ? args->ray_scaling_exp_avg_sq : nullptr;
    a.accum = args->accum; a.denom = args->denom; a.max_radii = args->max_radii2D;
    a.noise = args->noise;
    a.head = reinterpret_cast<const uint32_t*>(workspace);
    a.bases = a.head + kDnHeadWords;
    const int groups = dn_groups(P);
    a.fate = reinterpret_cast<const uint8_t*>(a.bases + (size_t)groups * 3);
    a.P = P;
    a.out_rows = args->out_rows;
    if (groups == 0) return 0;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(densify_scatter_kernel, dim3(groups), dim3(kDnBlock), 0, st, a);
    return check_hip(hipGetLastError(), "densify_scatter");
}

int scg_reset_opacity(int32_t n_ray, float* ray_opacity, float* ray_exp_avg, float* ray_exp_avg_sq, int32_t n_bg,
                      float* bg_opacity, float* bg_exp_avg, float* bg_exp_avg_sq, void* stream) {
    if (n_ray < 0 || n_bg < 0) return fail(SCG_E_RANGE, "reset_opacity: negative count (ray %d, bg %d)", n_ray, n_bg);
    if ((n_ray > 0 && !ray_opacity) || (n_bg > 0 && !bg_opacity)) return fail(SCG_E_NULL, "reset_opacity: an opacity tensor is NULL");
    const int64_t n = (int64_t)n_ray + n_bg;
    if (n == 0) return 0;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(reset_opacity_kernel, dim3((unsigned)((n + kDnBlock - 1) / kDnBlock)), dim3(kDnBlock), 0, st, n_ray,
                       ray_opacity, n_ray > 0 ? ray_exp_avg : nullptr, n_ray > 0 ? ray_exp_avg_sq : nullptr, n_bg, bg_opacity,
                       n_bg > 0 ? bg_exp_avg : nullptr, n_bg > 0 ? bg_exp_avg_sq : nullptr);
    return check_hip(hipGetLastError(), "reset_opacity");
}

}  // extern "C"

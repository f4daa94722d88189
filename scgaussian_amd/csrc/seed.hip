// seed.hip — the model seeded from the init stage (include/scg_raster.h, "Seeding the model from the init stage").
//
// The reference's create_from_pcd (scene/gaussian_model.py:362-468) walks the ordered view pairs in a Python loop; its rule decides
// every match from that match alone, and the arena of the init stage already lies in the order it walks.  So the call is a stable
// stream compaction plus a few per-row formulas, around ONE host read:
//
//   seed_classify_kernel   one thread per match: the keep byte (min_loss < threshold) and the workgroup's count; the same grid sets
//                          the winner map (one int32 per pixel of sparse_depths) to -1
//   seed_scan_kernel       one workgroup: exclusive scan of the per-workgroup counts in workgroup order (compact.h), the total into
//                          the head
//   (the caller reads the total n and allocates the model's tensors)
//   seed_scatter_kernel    the same partition: ranks within the workgroup recomputed from the keep bytes, the per-row values written
//                          at base + rank; a workgroup's rows are consecutive, so features_rest, rotation, opacity and max_radii2D
//                          are filled with the lanes running across them.  Every kept match with a finite uv puts its arena index
//                          into the winner map of its source view's pixel with an integer atomicMax: the latest in arena order wins,
//                          whatever order the threads run in.
//   (the caller runs the kNN on `points`)
//   seed_finish_kernel     scaling = log(sqrt(max(dist2, 1e-7))) three times per row; sparse_depths and masks from the winner map,
//                          one thread per pixel — pixels no match hit become 0 in the same pass
//
// No workgroup waits for another inside a kernel.  Compiled with -ffp-contract=off: points = rays_o + rays_d * z is one multiply
// and one add, as torch's two operators are.
#include "compact.h"

namespace scg {

constexpr int kSdBlock = 256;
constexpr int kSdHeadWords = 8;                       // [0] the row count n, [1..7] zero
constexpr int kSdRest = 45;                           // floats of a features_rest row
constexpr int kSdMaxFillGroups = 1024;                // workgroups that share the fill of the winner map when N is small
constexpr int64_t kSdMaxPixels = (int64_t)1 << 31;    // pixel indices are formed in 64 bits; the map itself stays below 8 GiB
constexpr float kSdC0 = 0.28209479177387814f;         // SH band 0 (utils/sh_utils.py RGB2SH)

__host__ __device__ inline int sd_groups(int N) { return N > 0 ? (N + kSdBlock - 1) / kSdBlock : 1; }
inline bool sd_sizes_ok(int64_t N, int64_t pixels) { return N >= 0 && N <= INT32_MAX && pixels >= 0 && pixels <= kSdMaxPixels; }
inline size_t sd_workspace_bytes(int N, int64_t pixels) {
    return ((size_t)kSdHeadWords + (size_t)sd_groups(N) + (size_t)pixels) * 4 + (((size_t)N + 3) & ~(size_t)3);
}

struct SdWorkspace {
    uint32_t* head;
    uint32_t* counts;
    int32_t* winner;
    uint8_t* keep;
};
inline SdWorkspace sd_carve(void* ws, int N, int64_t pixels) {
    SdWorkspace w;
    w.head = reinterpret_cast<uint32_t*>(ws);
    w.counts = w.head + kSdHeadWords;
    w.winner = reinterpret_cast<int32_t*>(w.counts + sd_groups(N));
    w.keep = reinterpret_cast<uint8_t*>(w.winner + pixels);
    return w;
}

struct SdScatterArgs {
    int N, n_out, V, H, W, nseg;
    const ScgSeedSegment* seg;
    const float* rays_o;
    const float* rays_d;
    const float* z;
    const float* color;
    const float* uv;
    float opacity;
    float* zval;
    float* rayo;
    float* rayd;
    float* points;
    float* dc;
    float* rest;
    float* rotation;
    float* opacity_out;
    float* max_radii;
    const uint32_t* bases;
    const uint8_t* keep;
    int32_t* winner;
};

__global__ __launch_bounds__(kSdBlock) void seed_classify_kernel(const float* min_loss, int N, float threshold, int groups,
                                                                 uint8_t* keep, uint32_t* counts, int32_t* winner, int64_t pixels) {
    const int64_t i = (int64_t)blockIdx.x * kSdBlock + threadIdx.x;
    bool k = false;
    if (i < N) {
        k = min_loss ? (min_loss[i] < threshold) : true;                  // a NaN compares false: dropped
        keep[i] = (uint8_t)k;
    }
    uint32_t rank, n;
    block_counts<1, kSdBlock>(k, &rank, &n);
    if (threadIdx.x == 0 && (int)blockIdx.x < groups) counts[blockIdx.x] = n;
    const int64_t stride = (int64_t)gridDim.x * kSdBlock;
    for (int64_t p = i; p < pixels; p += stride) winner[p] = -1;
}

// counts -> exclusive bases in place, the total into the head
__global__ __launch_bounds__(kSdBlock) void seed_scan_kernel(uint32_t* head, uint32_t* counts, int groups) {
    uint32_t n;
    carry_scan<1, kSdBlock>(counts, groups, &n);
    if (threadIdx.x == 0) {
        head[0] = n;
        for (int k = 1; k < kSdHeadWords; ++k) head[k] = 0;
    }
}

__global__ __launch_bounds__(kSdBlock) void seed_scatter_kernel(SdScatterArgs a) {
    __shared__ int32_t s_off[SCG_SEED_MAX_SEGMENTS];
    __shared__ int32_t s_view[SCG_SEED_MAX_SEGMENTS];
    const int tid = threadIdx.x;
    for (int s = tid; s < a.nseg; s += kSdBlock) {
        s_off[s] = a.seg[s].offset;
        s_view[s] = a.seg[s].view;
    }
    const int64_t i = (int64_t)blockIdx.x * kSdBlock + tid;
    const bool k = i < a.N && a.keep[i] != 0;
    uint32_t rank, tot;                                                   // rank of this match among the workgroup's kept ones
    block_counts<1, kSdBlock>(k, &rank, &tot);                            // ... and its barrier: the segment table is in LDS
    const int64_t base = a.bases[blockIdx.x];
    const int64_t r = base + rank;
    if (k && r < a.n_out) {                                               // never beyond what the caller allocated
        const float z = a.z[i];
        a.zval[r] = z;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float o = a.rays_o[i * 3 + c], d = a.rays_d[i * 3 + c];
            a.rayo[r * 3 + c] = o;
            a.rayd[r * 3 + c] = d;
            a.points[r * 3 + c] = o + d * z;
            a.dc[r * 3 + c] = __fdiv_rn(a.color[i * 3 + c] - 0.5f, kSdC0);
        }
        const float u = a.uv[i * 2], v = a.uv[i * 2 + 1];
        if (isfinite(u) && isfinite(v)) {
            // the segment of match i: the last one whose offset is <= i (the table is sorted and tiles [0, N))
            int lo = 0, hi = a.nseg - 1;
            while (lo < hi) {
                const int mid = (lo + hi + 1) >> 1;
                if (s_off[mid] <= i) lo = mid; else hi = mid - 1;
            }
            const int view = s_view[lo];
            const int64_t row = (int64_t)fminf(fmaxf(v, 0.0f), (float)(a.H - 1));      // clamp on the float, then truncate
            const int64_t col = (int64_t)fminf(fmaxf(u, 0.0f), (float)(a.W - 1));
            if (view >= 0 && view < a.V && row >= 0 && row < a.H && col >= 0 && col < a.W)
                atomicMax(&a.winner[((int64_t)view * a.H + row) * a.W + col], (int32_t)i);
        }
    }
    // the workgroup's rows are [base, base + tot): the constant tensors with the lanes running across them
    const int64_t end = base + tot < a.n_out ? base + tot : (int64_t)a.n_out;
    const int64_t rows = end - base;
    for (int64_t e = tid; e < rows * kSdRest; e += kSdBlock) a.rest[base * kSdRest + e] = 0.0f;
    for (int64_t e = tid; e < rows * 4; e += kSdBlock) a.rotation[base * 4 + e] = (e & 3) == 0 ? 1.0f : 0.0f;
    for (int64_t e = tid; e < rows; e += kSdBlock) {
        a.opacity_out[base + e] = a.opacity;
        a.max_radii[base + e] = 0.0f;
    }
}

__global__ __launch_bounds__(kSdBlock) void seed_finish_kernel(int n_out, const float* dist2, float* scaling, int N, const float* z,
                                                               const float* cam_z, const int32_t* winner, int64_t pixels,
                                                               float* sparse, uint8_t* masks) {
    const int64_t t = (int64_t)blockIdx.x * kSdBlock + threadIdx.x;
    if (t < n_out) {
        const float s = logf(sqrtf(fmaxf(dist2[t], 1e-7f)));
        scaling[t * 3] = s;
        scaling[t * 3 + 1] = s;
        scaling[t * 3 + 2] = s;
    }
    const int64_t stride = (int64_t)gridDim.x * kSdBlock;
    for (int64_t p = t; p < pixels; p += stride) {
        const int32_t wi = winner[p];
        const float d = (wi >= 0 && wi < N) ? z[wi] * cam_z[wi] : 0.0f;
        sparse[p] = d;
        masks[p] = (uint8_t)(d > 0.0f);
    }
}

static int validate_sizes(const char* who, int64_t N, int64_t V, int64_t H, int64_t W) {
    if (N < 0) return fail(SCG_E_RANGE, "%s: N = %lld < 0", who, (long long)N);
    if (V < 0) return fail(SCG_E_RANGE, "%s: V = %lld < 0", who, (long long)V);
    if (H <= 0 || W <= 0) return fail(SCG_E_RANGE, "%s: H = %lld, W = %lld must be > 0", who, (long long)H, (long long)W);
    if (V * H * W > kSdMaxPixels) return fail(SCG_E_RANGE, "%s: %lld pixels > %lld", who, (long long)(V * H * W), (long long)kSdMaxPixels);
    return 0;
}

static int fill_groups(int N, int64_t pixels) {
    int64_t fill = (pixels + 4 * kSdBlock - 1) / (4 * kSdBlock);
    if (fill > kSdMaxFillGroups) fill = kSdMaxFillGroups;
    return fill > sd_groups(N) ? (int)fill : sd_groups(N);
}

}  // namespace scg

using namespace scg;

extern "C" {

size_t scg_seed_workspace_bytes(int32_t N, int64_t pixels) { return sd_sizes_ok(N, pixels) ? sd_workspace_bytes(N, pixels) : 0; }

int scg_seed_classify(const float* min_loss, int32_t N, float threshold, int64_t pixels, void* workspace, size_t workspace_bytes,
                      void* stream) {
    if (N < 0) return fail(SCG_E_RANGE, "seed_classify: N = %d < 0", N);
    if (pixels < 0 || pixels > kSdMaxPixels) return fail(SCG_E_RANGE, "seed_classify: pixels = %lld out of range", (long long)pixels);
    if (int rc = check_workspace("seed_classify", workspace, workspace_bytes, sd_workspace_bytes(N, pixels))) return rc;
    if (min_loss && reinterpret_cast<uintptr_t>(min_loss) % 4) return fail(SCG_E_ALIGN, "seed_classify: min_loss not 4-byte aligned");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const SdWorkspace w = sd_carve(workspace, N, pixels);
    const int groups = sd_groups(N);
    hipLaunchKernelGGL(seed_classify_kernel, dim3(fill_groups(N, pixels)), dim3(kSdBlock), 0, st, min_loss, N, threshold, groups,
                       w.keep, w.counts, w.winner, pixels);
    if (int rc = check_hip(hipGetLastError(), "seed_classify")) return rc;
    hipLaunchKernelGGL(seed_scan_kernel, dim3(1), dim3(kSdBlock), 0, st, w.head, w.counts, groups);
    return check_hip(hipGetLastError(), "seed_scan");
}

int scg_seed_scatter(const ScgSeedScatter* p, void* workspace, size_t workspace_bytes, void* stream) {
    if (!p) return fail(SCG_E_NULL, "seed_scatter: args is NULL");
    if (p->struct_bytes != (int32_t)sizeof(ScgSeedScatter))
        return fail(SCG_E_RANGE, "seed_scatter: struct_bytes = %d, the library's ScgSeedScatter has %zu", p->struct_bytes,
                    sizeof(ScgSeedScatter));
    if (int rc = validate_sizes("seed_scatter", p->N, p->V, p->H, p->W)) return rc;
    const int N = p->N;
    if (p->n_out < 0 || p->n_out > N) return fail(SCG_E_RANGE, "seed_scatter: n_out = %d not in 0..N = %d", p->n_out, N);
    if (p->nseg < 0 || p->nseg > SCG_SEED_MAX_SEGMENTS)
        return fail(SCG_E_RANGE, "seed_scatter: nseg = %d not in 0..%d", p->nseg, SCG_SEED_MAX_SEGMENTS);
    if (N > 0 && p->nseg < 1) return fail(SCG_E_RANGE, "seed_scatter: %d matches but no segment", N);
    if (p->nseg > 0 && (!p->segments || !p->segments_dev)) return fail(SCG_E_NULL, "seed_scatter: a segment table is NULL");
    int64_t at = 0;
    for (int s = 0; s < p->nseg; ++s) {
        const ScgSeedSegment& g = p->segments[s];
        if (g.view < 0 || g.view >= p->V) return fail(SCG_E_RANGE, "seed_scatter: segment %d has view %d outside [0, %d)", s, g.view, p->V);
        if (g.count < 0 || g.offset < 0) return fail(SCG_E_RANGE, "seed_scatter: segment %d has offset %d, count %d", s, g.offset, g.count);
        if ((int64_t)g.offset + g.count > N)
            return fail(SCG_E_RANGE, "seed_scatter: segment %d [%d, %lld) runs past N = %d", s, g.offset, (long long)g.offset + g.count, N);
        if (g.offset != at) return fail(SCG_E_RANGE, "seed_scatter: segment %d starts at %d, the one before it ends at %lld", s, g.offset, (long long)at);
        at += g.count;
    }
    if (at != N) return fail(SCG_E_RANGE, "seed_scatter: the segments cover %lld of N = %d matches", (long long)at, N);
    const int64_t pixels = (int64_t)p->V * p->H * p->W;
    if (int rc = check_workspace("seed_scatter", workspace, workspace_bytes, sd_workspace_bytes(N, pixels))) return rc;
    if (N > 0 && (!p->rays_o || !p->rays_d || !p->z || !p->color || !p->uv)) return fail(SCG_E_NULL, "seed_scatter: an input tensor is NULL");
    if (p->n_out > 0 && (!p->zval || !p->rayo || !p->rayd || !p->points || !p->features_dc || !p->features_rest || !p->rotation ||
                         !p->opacity_out || !p->max_radii2D))
        return fail(SCG_E_NULL, "seed_scatter: an output tensor is NULL");
    if (N == 0) return 0;
    const SdWorkspace w = sd_carve(workspace, N, pixels);
    SdScatterArgs a;
    a.N = N; a.n_out = p->n_out; a.V = p->V; a.H = p->H; a.W = p->W; a.nseg = p->nseg;
    a.seg = p->segments_dev;
    a.rays_o = p->rays_o; a.rays_d = p->rays_d; a.z = p->z; a.color = p->color; a.uv = p->uv;
    a.opacity = p->opacity;
    a.zval = p->zval; a.rayo = p->rayo; a.rayd = p->rayd; a.points = p->points; a.dc = p->features_dc; a.rest = p->features_rest;
    a.rotation = p->rotation; a.opacity_out = p->opacity_out; a.max_radii = p->max_radii2D;
    a.bases = w.counts; a.keep = w.keep; a.winner = w.winner;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(seed_scatter_kernel, dim3(sd_groups(N)), dim3(kSdBlock), 0, st, a);
    return check_hip(hipGetLastError(), "seed_scatter");
}

int scg_seed_finish(int32_t n_out, const float* dist2, float* scaling, int32_t N, const float* z, const float* cam_z, int32_t V,
                    int32_t H, int32_t W, float* sparse_depths, uint8_t* masks, const void* workspace, size_t workspace_bytes,
                    void* stream) {
    if (int rc = validate_sizes("seed_finish", N, V, H, W)) return rc;
    if (n_out < 0 || n_out > N) return fail(SCG_E_RANGE, "seed_finish: n_out = %d not in 0..N = %d", n_out, N);
    const int64_t pixels = (int64_t)V * H * W;
    if (int rc = check_workspace("seed_finish", workspace, workspace_bytes, sd_workspace_bytes(N, pixels))) return rc;
    if (n_out > 0 && (!dist2 || !scaling)) return fail(SCG_E_NULL, "seed_finish: dist2 / scaling is NULL");
    if (N > 0 && (!z || !cam_z)) return fail(SCG_E_NULL, "seed_finish: z / cam_z is NULL");
    if (pixels > 0 && (!sparse_depths || !masks)) return fail(SCG_E_NULL, "seed_finish: sparse_depths / masks is NULL");
    if (n_out == 0 && pixels == 0) return 0;
    const SdWorkspace w = sd_carve(const_cast<void*>(workspace), N, pixels);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(seed_finish_kernel, dim3(fill_groups(n_out, pixels)), dim3(kSdBlock), 0, st, n_out, dist2, scaling, N, z,
                       cam_z, w.winner, pixels, sparse_depths, masks);
    return check_hip(hipGetLastError(), "seed_finish");
}

}  // extern "C"

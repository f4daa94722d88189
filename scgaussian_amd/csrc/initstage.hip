// initstage.hip — the reference's ray-depth init stage (train.py:49-95 over scene/gaussian_model.py:175-239) with n_steps Adam
// iterations per launch (include/scg_matchloss.h, "The ray-depth init stage").
//
// valid_mask = mask0 * mask1 > 0 does not depend on z_val and every z_val element appears in exactly one loss term, so once the
// valid counts are folded into a per-element weight each match is independent of every other: ONE THREAD carries one match
// through all iterations of the launch in registers (z, both Adam moments, best z, smallest loss).  The arena of the reference
// scene holds ~12 000 matches — a few dozen waves on 256 compute units — so the kernel is a chain of dependent instructions, not
// a bandwidth problem.  What it does about that:
//   * one wave per workgroup: no barrier inside the iteration loop, and the waves spread over as many compute units as there are;
//   * (X, Y, Z) = K_b (R_b (o + d z) + t_b) is affine in z: A = K_b (R_b o + t_b) and B = K_b R_b d are formed once per launch
//     (in double, rounded once), an iteration starts with three multiply-adds;
//   * the two step-dependent Adam coefficients of every step of the launch are built once into LDS (double pow, as
//     adam_step_kernel forms them) and the next step's pair is fetched while this step's chain runs;
//   * the progress scalar (sum of wgt * ml per iteration) costs the loop one LDS store per iteration: every 64 iterations thread j
//     adds up row j of a 64 x 64 tile in lane order and writes partials[k][workgroup].  Fixed order, no atomics.
// Compiled with -ffp-contract=off, like optim.hip: Adam in torch's order, one rounding per operation (csrc/adam_math.h).
#include "scg_common.h"
#include "adam_math.h"
#include "../../include/scg_matchloss.h"

namespace scg {

constexpr int kIsBlock = kWave;                // one wave per workgroup
constexpr int kIsRows = 64;                    // iterations between two flushes of the partial sums
constexpr int kIsMaxSteps = SCG_INIT_STAGE_MAX_STEPS;

struct InitArgs {
    const ScgInitSegment* seg;
    int nseg, N;
    const float* rays_o;
    const float* rays_d;
    const float2* uv_t;
    const float* wgt;
    float* z;
    float* m;
    float* v;
    float* best;
    float* minl;
    int first_iter, n_steps;
    double lr, b1, b2;
    float w1, b2f, w2, eps;                    // (float)(1 - b1), (float)b2, (float)(1 - b2), (float)eps, as optim.hip passes them
    float loss_scale;
    float* loss_state;
    float* grad;
    float* partials;
    int W;                                     // workgroups = row length of partials
};

// What does not depend on z
struct ElemConst {
    float aX, aY, aZ, bX, bY, bZ;              // (X, Y, Z) = a + b z
    float u, v, cw, ch;                        // target pixel; 0.5 / width, 0.5 / height
    float wgt;
};

struct Term { float ml, g1; };                 // loss_state entry; wgt * d ml / d z

__device__ __forceinline__ ElemConst load_elem(const InitArgs& a, int i) {
    // the segment of element i: the last one whose offset is <= i (the table is sorted by offset); always inside [0, nseg)
    int lo = 0, hi = a.nseg - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (a.seg[mid].offset <= i) lo = mid; else hi = mid - 1;
    }
    const ScgInitSegment& s = a.seg[lo];
    const double ox = a.rays_o[3 * i], oy = a.rays_o[3 * i + 1], oz = a.rays_o[3 * i + 2];
    const double dx = a.rays_d[3 * i], dy = a.rays_d[3 * i + 1], dz = a.rays_d[3 * i + 2];
    double co[3], cd[3];
    for (int r = 0; r < 3; ++r) {
        co[r] = (double)s.w2c[4 * r] * ox + (double)s.w2c[4 * r + 1] * oy + (double)s.w2c[4 * r + 2] * oz + (double)s.w2c[4 * r + 3];
        cd[r] = (double)s.w2c[4 * r] * dx + (double)s.w2c[4 * r + 1] * dy + (double)s.w2c[4 * r + 2] * dz;
    }
    double A[3], B[3];
    for (int r = 0; r < 3; ++r) {
        A[r] = (double)s.intr[3 * r] * co[0] + (double)s.intr[3 * r + 1] * co[1] + (double)s.intr[3 * r + 2] * co[2];
        B[r] = (double)s.intr[3 * r] * cd[0] + (double)s.intr[3 * r + 1] * cd[1] + (double)s.intr[3 * r + 2] * cd[2];
    }
    ElemConst c;
    c.aX = (float)A[0]; c.aY = (float)A[1]; c.aZ = (float)A[2];
    c.bX = (float)B[0]; c.bY = (float)B[1]; c.bZ = (float)B[2];
    const float2 t = a.uv_t[i];
    c.u = t.x; c.v = t.y;
    c.cw = 0.5f / s.width; c.ch = 0.5f / s.height;
    c.wgt = a.wgt[i];
    return c;
}

__device__ __forceinline__ Term eval_term(const ElemConst& c, float z) {
    const float X = c.aX + c.bX * z, Y = c.aY + c.bY * z, Z = c.aZ + c.bZ * z;
    const float inv = 1.f / (Z + 1e-8f);
    const float px = X * inv, py = Y * inv;
    const float ex = px - c.u, ey = py - c.v;
    Term t;
    t.ml = fabsf(ex) * c.cw + fabsf(ey) * c.ch;
    const float sx = (ex > 0.f) ? 1.f : ((ex < 0.f) ? -1.f : 0.f), sy = (ey > 0.f) ? 1.f : ((ey < 0.f) ? -1.f : 0.f);
    const float dpx = (c.bX - px * c.bZ) * inv, dpy = (c.bY - py * c.bZ) * inv;
    // a masked-out match has gradient zero whatever its term is (the reference indexes it away: an infinite term must not reach it)
    t.g1 = (c.wgt != 0.f) ? c.wgt * (sx * dpx * c.cw + sy * dpy * c.ch) : 0.f;
    return t;
}

// rows [0, rows) of the tile hold one value per lane: thread j adds up row j in lane order and writes it to iteration k0 + j
__device__ __forceinline__ void flush_partials(const InitArgs& a, float (*tile)[kIsBlock + 1], int k0, int rows) {
    __syncthreads();
    const int j = threadIdx.x;
    if (j < rows) {
        float s = 0.f;
        for (int l = 0; l < kIsBlock; ++l) s += tile[j][l];
        a.partials[(size_t)(k0 + j) * a.W + blockIdx.x] = s;
    }
    __syncthreads();
}

template <bool kPartials>
__global__ __launch_bounds__(kIsBlock) void init_stage_kernel(InitArgs a) {
    extern __shared__ float2 s_coef[];                             // (bc2s, nss) of every step of this launch
    __shared__ float s_tile[kIsRows][kIsBlock + 1];
    const int tid = threadIdx.x;
    for (int k = tid; k < a.n_steps; k += kIsBlock) {
        float bc2s, nss;
        adam_bias_coefs(a.b1, a.b2, a.lr, (double)(a.first_iter + k + 1), bc2s, nss);
        s_coef[k] = make_float2(bc2s, nss);
    }
    __syncthreads();
    const int i = blockIdx.x * kIsBlock + tid;
    const bool live = i < a.N;
    const int ic = live ? i : a.N - 1;                             // the tail lanes of the last wave repeat its last element
    ElemConst c = load_elem(a, ic);
    if (!live) c.wgt = 0.f;
    float z = a.z[ic];
    if (a.n_steps == 0) {                                          // evaluate: no state is touched
        const Term t = eval_term(c, z);
        if (live && a.loss_state) a.loss_state[i] = t.ml;
        if (live && a.grad) a.grad[i] = a.loss_scale * t.g1;
        if (kPartials) {
            s_tile[0][tid] = (c.wgt != 0.f) ? c.wgt * t.ml : 0.f;
            flush_partials(a, s_tile, 0, 1);
        }
        return;
    }
    float m = a.m[ic], v = a.v[ic];
    float best = z, minl = 0.f;
    if (a.first_iter > 0) { best = a.best[ic]; minl = a.minl[ic]; }
    AdamCoef cf;
    cf.w1 = a.w1; cf.b2f = a.b2f; cf.w2 = a.w2; cf.eps = a.eps;
    float2 next = s_coef[0];
    for (int k = 0; k < a.n_steps; ++k) {
        const int it = a.first_iter + k;
        cf.bc2s = next.x; cf.nss = next.y;
        next = s_coef[min(k + 1, a.n_steps - 1)];
        const Term t = eval_term(c, z);
        // the best-state rule as the reference executes it (train.py:68-76); `keep` is false when either side is a NaN
        if (it == 0) {
            minl = t.ml;
        } else {
            const bool keep = minl < t.ml;
            if (it >= 2) best = keep ? best : z;
            minl = keep ? minl : t.ml;
        }
        adam_update(z, m, v, a.loss_scale * t.g1, cf);
        if (it == 0) best = z;                                     // get_z_val() aliases the parameter through the first step
        if (kPartials) {
            const int row = k & (kIsRows - 1);
            s_tile[row][tid] = (c.wgt != 0.f) ? c.wgt * t.ml : 0.f;
            if (row == kIsRows - 1 || k == a.n_steps - 1) flush_partials(a, s_tile, k - row, row + 1);
        }
    }
    if (live) {
        a.z[i] = z; a.m[i] = m; a.v[i] = v; a.best[i] = best; a.minl[i] = minl;
    }
}

static inline int init_stage_groups(int32_t N) { return (N + kIsBlock - 1) / kIsBlock; }

}  // namespace scg

using namespace scg;

extern "C" {

size_t scg_init_stage_partials_bytes(int32_t N, int32_t n_steps) {
    if (N < 1 || n_steps < 0 || n_steps > kIsMaxSteps) return 0;
    return (size_t)(n_steps > 0 ? n_steps : 1) * (size_t)init_stage_groups(N) * sizeof(float);
}

int scg_init_stage_run(const ScgInitSegment* segments, int32_t nseg, int32_t N, const float* rays_o, const float* rays_d,
                       const float* uv_t, const float* wgt, float* z, float* exp_avg, float* exp_avg_sq, float* best_z,
                       float* min_loss, int32_t first_iter, int32_t n_steps, double lr, double beta1, double beta2, double eps,
                       float loss_scale, float* loss_state, float* grad, float* partials, size_t partials_bytes, void* stream) {
    if (N < 0 || nseg < 0) return fail(SCG_E_RANGE, "init stage: N = %d, nseg = %d", N, nseg);
    if (n_steps < 0 || n_steps > kIsMaxSteps) return fail(SCG_E_RANGE, "init stage: n_steps = %d not in 0..%d", n_steps, kIsMaxSteps);
    if (first_iter < 0 || first_iter > 0x7FFFFFFF - kIsMaxSteps) return fail(SCG_E_RANGE, "init stage: first_iter = %d out of range", first_iter);
    if (N == 0) return 0;
    if (nseg < 1) return fail(SCG_E_RANGE, "init stage: %d elements but no segment", N);
    if (!segments || !rays_o || !rays_d || !uv_t || !wgt || !z) return fail(SCG_E_NULL, "init stage: an input pointer is NULL");
    if (n_steps > 0 && (!exp_avg || !exp_avg_sq || !best_z || !min_loss)) return fail(SCG_E_NULL, "init stage: a state pointer is NULL");
    if (n_steps > 0 && !(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0))
        return fail(SCG_E_RANGE, "init stage: betas (%g, %g) not in [0, 1)", beta1, beta2);
    if (reinterpret_cast<uintptr_t>(uv_t) % 8) return fail(SCG_E_ALIGN, "init stage: uv_t must be 8-byte aligned");
    const void* words[] = {segments, rays_o, rays_d, wgt, z, exp_avg, exp_avg_sq, best_z, min_loss, loss_state, grad, partials};
    for (const void* p : words)
        if (reinterpret_cast<uintptr_t>(p) % 4) return fail(SCG_E_ALIGN, "init stage: a pointer is not 4-byte aligned");
    const size_t need = scg_init_stage_partials_bytes(N, n_steps);
    if (partials && partials_bytes < need) return fail(SCG_E_SCRATCH, "init stage: partials of %zu bytes < %zu", partials_bytes, need);
    InitArgs a;
    a.seg = segments; a.nseg = nseg; a.N = N;
    a.rays_o = rays_o; a.rays_d = rays_d; a.uv_t = reinterpret_cast<const float2*>(uv_t); a.wgt = wgt;
    a.z = z; a.m = exp_avg; a.v = exp_avg_sq; a.best = best_z; a.minl = min_loss;
    a.first_iter = first_iter; a.n_steps = n_steps;
    a.lr = lr; a.b1 = beta1; a.b2 = beta2;
    a.w1 = (float)(1.0 - beta1); a.b2f = (float)beta2; a.w2 = (float)(1.0 - beta2); a.eps = (float)eps;
    a.loss_scale = loss_scale;
    a.loss_state = loss_state; a.grad = grad; a.partials = partials;
    a.W = init_stage_groups(N);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const size_t lds = (size_t)(n_steps > 0 ? n_steps : 1) * sizeof(float2);
    if (partials) hipLaunchKernelGGL(init_stage_kernel<true>, dim3(a.W), dim3(kIsBlock), lds, st, a);
    else hipLaunchKernelGGL(init_stage_kernel<false>, dim3(a.W), dim3(kIsBlock), lds, st, a);
    return check_hip(hipGetLastError(), "init_stage_kernel");
}

}  // extern "C"

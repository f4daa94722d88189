// camgrad.hip — libscg_camgrad.so: the rasterizer's gradient with respect to the camera (scg_camgrad.h states the rule and the call).
//
// Two launches.  camgrad_kernel: one thread per Gaussian, 256-thread workgroups; every load of a thread (its inputs, the three
// float4 of its gradient record, its radius, its SH record) is issued up front, the load discipline of geometry_backward_kernel;
// the forward chain is recomputed with the geometry kernels' own device functions (csrc/geometry_math.h) and the backward chain of
// geometry_backward_one (csrc/geometry.hip) is RESTATED here as far as the camera needs it (camgrad_one: each piece names its
// origin) — that function is on the benchmark's path and is not re-cut; tests/test_gpu_camgrad.py holds the two copies together
// with the translation identity.  The 27 contributions of a workgroup are reduced in the fixed order of csrc/reduce.h into
// partials[block][27].  camgrad_finish_kernel: one workgroup folds the partials in fp64 in block order and writes the 35 floats.
// No atomics, no host read, nothing allocated: bitwise reproducible and capturable.
//
// Compiled with -ffp-contract=off (build.SIDE_LIBRARIES): the colour clamp is RECOMPUTED here and must take the forward's
// decision, i.e. evaluate the forward's chain of single fp32 operations (csrc/sh_eval.h at the direction geometry_forward_one forms).
#include "../../include/camgrad/scg_camgrad.h"

#include "scg_common.h"
#include "host_align.h"
#include "host_error.h"
#include "reduce.h"
#include "sh_eval.h"
#include "geometry_math.h"

#pragma clang fp contract(off)

namespace scg {

static thread_local ErrorText g_err = {};

constexpr int kSums = SCG_CAMGRAD_SUMS;
constexpr int kOut = SCG_CAMGRAD_OUT_FLOATS;
static_assert(SCG_CAMGRAD_BLOCK == kBlock, "the first launch's workgroup is the geometry kernels' 256 threads");

// Where the sums live in a partial record:  [3j + i] = dV[4j + i] (i = 0..2),  [12 + 3j + {0, 1, 2}] = dPM[4j + {0, 1, 3}],
// [24 + c] = dcampos[c].  The place of output word t (0..34) in it, -1 for the twelve words that are always zero.
__host__ __device__ __forceinline__ int sum_slot(int t) {
    if (t < 16) return (t & 3) == 3 ? -1 : 3 * (t >> 2) + (t & 3);
    if (t < 32) { const int e = t - 16, i = e & 3; return i == 2 ? -1 : 12 + 3 * (e >> 2) + (i == 3 ? 2 : i); }
    return 24 + (t - 32);
}

// One visible Gaussian's 27 contributions.  DEG: the active SH degree when dL/dcampos is wanted and exists (1..3), else 0.
template <int DEG>
__device__ __forceinline__ void camgrad_one(const FrameDev& f, const Mat16& V, const Mat16& PM, const float* cam, const GeoIn& in,
                                            bool has_cov, const float4& ga, const float4& gb, const float4& gc, const float* sh,
                                            float* c) {
    const float pos[4] = {in.x, in.y, in.z, 1.0f};
    // ---- the forward chain, recomputed (geometry_backward_one, csrc/geometry.hip: "Proj p; project ... cov2d")
    Proj p;
    project(f, V, PM, in.x, in.y, in.z, p);
    if (has_cov) {
#pragma unroll
        for (int k = 0; k < 6; ++k) p.cov[k] = in.a[k];
    } else {
        cov3d_from_scale_rot(in, f.mod, p);
    }
    cov2d(f, V, p);
    // ---- the record's raw sums -> dL/dxy, dL/dconic (geometry_backward_one: the block behind cov2d)
    const float con_a = p.C * p.det_inv, con_b = -p.B * p.det_inv, con_c = p.A * p.det_inv;
    const float dxy_x = -(con_a * ga.x + con_b * ga.y);
    const float dxy_y = -(con_b * ga.x + con_c * ga.y);
    const float d_a = gb.x * -0.5f, d_b = -gb.y, d_c = gb.z * -0.5f;                    // (ga.w, dL/dopacity's sum: not the camera's)
    // ---- conic = inverse(cov2D) (geometry_backward_one: "a = C/det, b = -B/det, c = A/det")
    const float di2 = p.det_inv * p.det_inv;
    const float dA = di2 * (-p.C * p.C * d_a + p.B * p.C * d_b - p.B * p.B * d_c);
    const float dC = di2 * (-p.B * p.B * d_a + p.A * p.B * d_b - p.A * p.A * d_c);
    const float dB = di2 * (2.0f * p.B * p.C * d_a - (p.A * p.C + p.B * p.B) * d_b + 2.0f * p.A * p.B * d_c);
    // ---- cov2D = Tm Sigma Tm^T -> dTm (geometry_backward_one: dT0, dT1)
    const float u[3] = {p.u0, p.u1, p.u2};
    const float v[3] = {p.v0, p.v1, p.v2};
    float dT0[3], dT1[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        dT0[k] = 2.0f * dA * u[k] + dB * v[k];
        dT1[k] = dB * u[k] + 2.0f * dC * v[k];
    }
    // ---- Tm = J . Wm, Wm[i][j] = V[4j+i] -> dJ -> dt (geometry_backward_one: dJ00 .. dtz; D2: a clamped component is a constant)
    const float dJ00 = dT0[0] * V.m[0] + dT0[1] * V.m[4] + dT0[2] * V.m[8];
    const float dJ02 = dT0[0] * V.m[2] + dT0[1] * V.m[6] + dT0[2] * V.m[10];
    const float dJ11 = dT1[0] * V.m[1] + dT1[1] * V.m[5] + dT1[2] * V.m[9];
    const float dJ12 = dT1[0] * V.m[2] + dT1[1] * V.m[6] + dT1[2] * V.m[10];
    const float itz = 1.0f / p.tz;
    const float itz2 = itz * itz;
    const float itz3 = itz2 * itz;
    const float dtx = p.cl_x ? 0.f : -f.focal_x * itz2 * dJ02;
    const float dty = p.cl_y ? 0.f : -f.focal_y * itz2 * dJ12;
    float dtz = -f.focal_x * itz2 * dJ00 - f.focal_y * itz2 * dJ11 +
                2.0f * f.focal_x * p.t_x * itz3 * dJ02 + 2.0f * f.focal_y * p.t_y * itz3 * dJ12;
    dtz += ga.z;                                        // depth = view z
    // ---- pixel -> NDC (geometry_backward_one: dndc_x, dndc_y)
    const float dndc_x = dxy_x * 0.5f * (float)f.W;
    const float dndc_y = dxy_y * 0.5f * (float)f.H;
    // ---- the Jacobian's entries as cov2d (csrc/geometry_math.h) forms them
    const float tz2 = p.tz * p.tz;
    const float J00 = f.focal_x / p.tz;
    const float J02 = -(f.focal_x * p.t_x) / tz2;
    const float J11 = f.focal_y / p.tz;
    const float J12 = -(f.focal_y * p.t_y) / tz2;

    // ---- the camera's own part: the same chain contracted with the Gaussian's position instead of the camera's matrix
    const float dhx = dndc_x * p.m_w, dhy = dndc_y * p.m_w;
    const float dhw = -(p.hx * dndc_x + p.hy * dndc_y) * p.m_w * p.m_w;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        c[3 * j + 0] = dtx * pos[j];
        c[3 * j + 1] = dty * pos[j];
        c[3 * j + 2] = dtz * pos[j];
        c[12 + 3 * j + 0] = dhx * pos[j];
        c[12 + 3 * j + 1] = dhy * pos[j];
        c[12 + 3 * j + 2] = dhw * pos[j];
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        c[3 * k + 0] += dT0[k] * J00;
        c[3 * k + 1] += dT1[k] * J11;
        c[3 * k + 2] += dT0[k] * J02 + dT1[k] * J12;
    }

    // ---- dL/dcampos = -(the SH-direction part of dL/dmeans3D)
    if (DEG > 0) {
        constexpr int K = (DEG + 1) * (DEG + 1);
        float dx = in.x - cam[0], dy = in.y - cam[1], dz = in.z - cam[2];
        const float len = sqrtf(dx * dx + dy * dy + dz * dz);
        // the channel clamp, recomputed as the forward took it (geometry_forward_one: dir = d / len, eval_sh, + 0.5, < 0)
        float rgb[3];
        eval_sh<DEG>(sh, dx / len, dy / len, dz / len, rgb);
        const float dRGB[3] = {(rgb[0] + 0.5f < 0.0f) ? 0.f : gc.x, (rgb[1] + 0.5f < 0.0f) ? 0.f : gc.y,
                               (rgb[2] + 0.5f < 0.0f) ? 0.f : gc.z};
        // the direction's gradient (geometry_backward_kernel's colour part: dir = d * (1 / len); sh_backward's ddx, ddy, ddz)
        const float ilen = 1.0f / len;
        dx *= ilen; dy *= ilen; dz *= ilen;
        float basis[K], bx[K], by[K], bz[K];
        sh_basis_grads<DEG>(dx, dy, dz, basis, bx, by, bz);
        float gx_ = 0.f, gy_ = 0.f, gz_ = 0.f;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const float g = sh[3 * k] * dRGB[0] + sh[3 * k + 1] * dRGB[1] + sh[3 * k + 2] * dRGB[2];
            gx_ += g * bx[k]; gy_ += g * by[k]; gz_ += g * bz[k];
        }
        // through dir = d / |d| (geometry_backward_kernel: "dm[0] += (gx_ - dx * dot) * ilen"), negated
        const float dot = dx * gx_ + dy * gy_ + dz * gz_;
        c[24] = -((gx_ - dx * dot) * ilen);
        c[25] = -((gy_ - dy * dot) * ilen);
        c[26] = -((gz_ - dz * dot) * ilen);
    }
}

template <int DEG, class Src>
__device__ __forceinline__ void camgrad_body(const FrameDev& f, const Src& src, const int32_t* __restrict__ radii,
                                             const float4* __restrict__ dsplats, float* __restrict__ partials) {
    __shared__ float s_red[kSums][kBlock / kWave];
    const int i = blockIdx.x * kBlock + threadIdx.x;
    const bool valid = i < f.P;
    const int ic = valid ? i : f.P - 1;                    // (lanes without a Gaussian load the last one's: no branch around the loads)
    // every load of the thread, issued before anything is waited for.  The SH record is fetched for the thread's OWN Gaussian
    // whether it is visible or not: asking the radius first would put a second round trip to memory behind the first
    int radius = radii[ic];
    GeoIn in = src.template load<false>(ic);
    constexpr int kRec = SCG_DSPLAT_FLOATS / 4;
    float4 ga = dsplats[kRec * (size_t)ic + 0];
    float4 gb = dsplats[kRec * (size_t)ic + 1];
    float4 gc = dsplats[kRec * (size_t)ic + 2];
    constexpr int K = DEG > 0 ? (DEG + 1) * (DEG + 1) : 1;
    float sh[(3 * K + 3) / 4 * 4];
    if (DEG > 0) src.template load_sh<K>(ic, sh);
    const Mat16 V = load16(f.view);
    const Mat16 PM = load16(f.proj);
    const float cam[3] = {f.campos[0], f.campos[1], f.campos[2]};
    __builtin_amdgcn_sched_barrier(0);

    const bool visible = valid && radius > 0;
    const bool wave_visible = __builtin_amdgcn_ballot_w64(visible) != 0;      // the same in every lane of the wave
    const int lane = lane_id(), wave = wave_id();
    if (wave_visible) {
        float c[kSums];
#pragma unroll
        for (int k = 0; k < kSums; ++k) c[k] = 0.f;
        if (visible) camgrad_one<DEG>(f, V, PM, cam, in, src.has_cov(), ga, gb, gc, sh, c);
#pragma unroll
        for (int k = 0; k < kSums; ++k) {
            const float s = wave_reduce(c[k], Sum());
            if (lane == 0) s_red[k][wave] = s;
        }
    } else if (lane < kSums) {
        s_red[lane][wave] = 0.f;                           // a wave with nothing to add: past the arithmetic, not past the barrier
    }
    __syncthreads();
    if ((int)threadIdx.x < kSums)
        partials[(size_t)blockIdx.x * kSums + threadIdx.x] = wg_fold<kBlock / kWave>(s_red[threadIdx.x], Sum());
}

template <int DEG>
__global__ __launch_bounds__(kBlock) void camgrad_kernel(
    FrameDev f, const float* __restrict__ means3D, const float* __restrict__ opacities, const float* __restrict__ shs,
    const float* __restrict__ scales, const float* __restrict__ rotations, const float* __restrict__ cov3D_precomp,
    const int32_t* __restrict__ radii, const float4* __restrict__ dsplats, float* __restrict__ partials, int sh_vec16) {
    const TensorSource src{means3D, opacities, shs, nullptr, scales, rotations, cov3D_precomp, f.M, sh_vec16};
    camgrad_body<DEG>(f, src, radii, dsplats, partials);
}

template <int DEG>
__global__ __launch_bounds__(kBlock) void camgrad_model_kernel(FrameDev f, ScgModel model, const int32_t* __restrict__ radii,
                                                               const float4* __restrict__ dsplats, float* __restrict__ partials) {
    const ModelSource src{model};
    camgrad_body<DEG>(f, src, radii, dsplats, partials);
}

// ONE workgroup of 1 024 threads.  Thread (run r = t / 32, sum s = t % 32) adds partials[b][s] over the blocks b of run r in block
// order, in fp64; the 32 runs are consecutive ranges of blocks, folded in run order: the sum is taken in block order throughout, and
// the parenthesisation is a function of n_blocks alone.  (The loads of a run do not depend on its adds: eight are in flight at a time.
// Measured at 782 blocks with eight runs of 98 and no unrolling: the fold, not the per-Gaussian launch, was most of the pass.)
constexpr int kFinishThreads = 1024;
constexpr int kRuns = kFinishThreads / 32;

__global__ __launch_bounds__(kFinishThreads) void camgrad_finish_kernel(const float* __restrict__ partials, int n_blocks,
                                                                        float* __restrict__ out) {
    __shared__ double s_run[kRuns][32];
    const int r = threadIdx.x >> 5, s = threadIdx.x & 31;
    const int per = (n_blocks + kRuns - 1) / kRuns;
    const int b0 = min(r * per, n_blocks), b1 = min(b0 + per, n_blocks);
    double acc = 0.0;
    if (s < kSums) {
        int b = b0;
        for (; b + 8 <= b1; b += 8) {
            float v[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) v[k] = partials[(size_t)(b + k) * kSums + s];
#pragma unroll
            for (int k = 0; k < 8; ++k) acc += (double)v[k];
        }
        for (; b < b1; ++b) acc += (double)partials[(size_t)b * kSums + s];
    }
    s_run[r][s] = acc;
    __syncthreads();
    if ((int)threadIdx.x < kOut) {
        const int slot = sum_slot(threadIdx.x);
        double t = 0.0;
        if (slot >= 0) {
            t = s_run[0][slot];
#pragma unroll
            for (int k = 1; k < kRuns; ++k) t += s_run[k][slot];
        }
        out[threadIdx.x] = (float)t;
    }
}

// ---- host ----------------------------------------------------------------------------------------------------------------------
static int check_common(const char* who, int32_t H, int32_t W, float tanfovx, float tanfovy, int32_t sh_degree, int32_t P,
                 const float* view, const float* proj, const float* campos, const int32_t* radii, const float* dsplats,
                 const float* partials, const float* out35, int32_t flags) {
    if (P < 0) return g_err.fail(SCG_E_RANGE, "%s: P = %d < 0", who, P);
    if (H <= 0 || W <= 0 || H > SCG_CAMGRAD_MAX_DIM || W > SCG_CAMGRAD_MAX_DIM)
        return g_err.fail(SCG_E_RANGE, "%s: image size %d x %d out of range", who, W, H);
    if (sh_degree < 0 || sh_degree > 3) return g_err.fail(SCG_E_RANGE, "%s: sh_degree %d not in 0..3", who, sh_degree);
    if (!(tanfovx > 0.f) || !(tanfovy > 0.f)) return g_err.fail(SCG_E_RANGE, "%s: tanfov must be positive", who);
    if (flags & ~SCG_CAMGRAD_NO_CAMPOS) return g_err.fail(SCG_E_RANGE, "%s: unknown flag bits 0x%x", who, flags);
    if (!view || !proj || !campos) return g_err.fail(SCG_E_NULL, "%s: view / proj / campos is NULL", who);
    if (int rc = g_err.check_ptr(who, out35, "out35", 4)) return rc;
    if (P == 0) return 0;
    if (int rc = g_err.check_ptr(who, radii, "radii", 4)) return rc;
    if (int rc = g_err.check_ptr(who, dsplats, "dsplats", 16)) return rc;
    if (int rc = g_err.check_ptr(who, partials, "partials", 4)) return rc;
    return 0;
}

static FrameDev frame_of(int32_t H, int32_t W, float tanfovx, float tanfovy, float scale_modifier, int32_t sh_degree, int32_t M, int32_t P,
                  const float* view, const float* proj, const float* campos) {
    FrameDev d = {};
    d.P = P; d.D = sh_degree; d.M = M; d.W = W; d.H = H;
    d.gx = (W + kTile - 1) / kTile;
    d.gy = (H + kTile - 1) / kTile;
    d.tanfovx = tanfovx; d.tanfovy = tanfovy;
    // the host scalars exactly as make_frame_dev (csrc/scg_common.h) and oracle.host_scalars form them
    d.focal_x = (float)W / (2.0f * tanfovx);
    d.focal_y = (float)H / (2.0f * tanfovy);
    d.limx = 1.3f * tanfovx;
    d.limy = 1.3f * tanfovy;
    d.mod = scale_modifier;
    d.view = view; d.proj = proj; d.campos = campos;
    return d;
}

static inline int n_blocks_of(int32_t P) { return (P + kBlock - 1) / kBlock; }

static int finish(const float* partials, int nb, float* out35, hipStream_t st) {
    hipLaunchKernelGGL(camgrad_finish_kernel, dim3(1), dim3(kFinishThreads), 0, st, partials, nb, out35);
    return g_err.check_hip(hipGetLastError(), "camgrad_finish_kernel");
}

static int check_model_set(const char* who, const ScgModelSet& m, bool ray, const char* name) {
    if (m.count < 0) return g_err.fail(SCG_E_RANGE, "%s: %s.count = %d < 0", who, name, m.count);
    if (m.count == 0) return 0;
    if (ray ? (!m.zval || !m.rayo || !m.rayd) : !m.xyz)
        return g_err.fail(SCG_E_NULL, ray ? "%s: %s: zval / rayo / rayd is NULL" : "%s: %s: xyz is NULL", who, name);
    if (!m.features_dc || !m.features_rest || !m.opacity || !m.scaling || !m.rotation)
        return g_err.fail(SCG_E_NULL, "%s: %s: features_dc / features_rest / opacity / scaling / rotation is NULL", who, name);
    if (!aligned16(m.rotation)) return g_err.fail(SCG_E_ALIGN, "%s: %s: rotation must be 16-byte aligned", who, name);
    return 0;
}

}  // namespace scg

using namespace scg;

extern "C" {

const char* scg_camgrad_last_error(void) { return g_err.text; }
int32_t scg_camgrad_abi_version(void) { return SCG_CAMGRAD_ABI_VERSION; }

int scg_camgrad_sizes(int32_t P, int32_t* n_blocks, uint64_t* partial_bytes) {
    const char* who = "scg_camgrad_sizes";
    if (!n_blocks || !partial_bytes) return g_err.fail(SCG_E_NULL, "%s: n_blocks / partial_bytes is NULL", who);
    if (P < 0) return g_err.fail(SCG_E_RANGE, "%s: P = %d < 0", who, P);
    *n_blocks = n_blocks_of(P);
    *partial_bytes = (uint64_t)n_blocks_of(P) * kSums * sizeof(float);
    return 0;
}

int scg_camgrad_backward(int32_t H, int32_t W, float tanfovx, float tanfovy, float scale_modifier, int32_t sh_degree, int32_t M,
                         int32_t P, const float* view, const float* proj, const float* campos, const float* means3D,
                         const float* opacities, const float* shs, const float* colors_precomp, const float* scales,
                         const float* rotations, const float* cov3D_precomp, const int32_t* radii, const float* dsplats,
                         float* partials, float* out35, int32_t flags, void* stream) {
    const char* who = "scg_camgrad_backward";
    if (int rc = check_common(who, H, W, tanfovx, tanfovy, sh_degree, P, view, proj, campos, radii, dsplats, partials, out35, flags))
        return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (P == 0) return finish(nullptr, 0, out35, st);
    if (!means3D || !opacities) return g_err.fail(SCG_E_NULL, "%s: means3D / opacities is NULL", who);
    if ((shs == nullptr) == (colors_precomp == nullptr))
        return g_err.fail(SCG_E_EXCLUSIVE, "%s: Please provide exactly one of either SHs or precomputed colors!", who);
    const bool has_sr = scales != nullptr && rotations != nullptr;
    if ((scales != nullptr) != (rotations != nullptr) || has_sr == (cov3D_precomp != nullptr))
        return g_err.fail(SCG_E_EXCLUSIVE,
                          "%s: Please provide exactly one of either scale/rotation pair or precomputed 3D covariance!", who);
    if (shs && (M < (sh_degree + 1) * (sh_degree + 1) || M > 65536))
        return g_err.fail(SCG_E_RANGE, "%s: M = %d, (sh_degree+1)^2 = %d", who, M, (sh_degree + 1) * (sh_degree + 1));
    if (rotations && !aligned16(rotations)) return g_err.fail(SCG_E_ALIGN, "%s: rotations must be 16-byte aligned", who);

    const FrameDev f = frame_of(H, W, tanfovx, tanfovy, scale_modifier, sh_degree, shs ? M : 0, P, view, proj, campos);
    const int vec16 = (shs && aligned16(shs) && ((M * 3 * 4) % 16 == 0)) ? 1 : 0;
    // degree -> instantiation; 0: no colour part (precomputed colours, degree 0, or dL/dcampos not wanted)
    static constexpr decltype(&camgrad_kernel<0>) kKernels[4] = {camgrad_kernel<0>, camgrad_kernel<1>, camgrad_kernel<2>,
                                                                 camgrad_kernel<3>};
    const int d = (!shs || (flags & SCG_CAMGRAD_NO_CAMPOS)) ? 0 : sh_degree;
    const int nb = n_blocks_of(P);
    hipLaunchKernelGGL(kKernels[d], dim3(nb), dim3(kBlock), 0, st, f, means3D, opacities, shs, scales, rotations, cov3D_precomp,
                       radii, reinterpret_cast<const float4*>(dsplats), partials, vec16);
    if (int rc = g_err.check_hip(hipGetLastError(), "camgrad_kernel")) return rc;
    return finish(partials, nb, out35, st);
}

int scg_camgrad_backward_model(int32_t H, int32_t W, float tanfovx, float tanfovy, float scale_modifier, int32_t sh_degree,
                               int32_t P, const float* view, const float* proj, const float* campos, const ScgModel* model,
                               const int32_t* radii, const float* dsplats, float* partials, float* out35, int32_t flags,
                               void* stream) {
    const char* who = "scg_camgrad_backward_model";
    if (int rc = check_common(who, H, W, tanfovx, tanfovy, sh_degree, P, view, proj, campos, radii, dsplats, partials, out35, flags))
        return rc;
    if (!model) return g_err.fail(SCG_E_NULL, "%s: model is NULL", who);
    if (int rc = check_model_set(who, model->ray, true, "ray")) return rc;
    if (int rc = check_model_set(who, model->bg, false, "bg")) return rc;
    if ((int64_t)model->ray.count + model->bg.count != P)
        return g_err.fail(SCG_E_RANGE, "%s: P = %d != ray.count + bg.count = %d + %d", who, P, model->ray.count, model->bg.count);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (P == 0) return finish(nullptr, 0, out35, st);

    const FrameDev f = frame_of(H, W, tanfovx, tanfovy, scale_modifier, sh_degree, 16, P, view, proj, campos);
    static constexpr decltype(&camgrad_model_kernel<0>) kKernels[4] = {camgrad_model_kernel<0>, camgrad_model_kernel<1>,
                                                                       camgrad_model_kernel<2>, camgrad_model_kernel<3>};
    const int d = (flags & SCG_CAMGRAD_NO_CAMPOS) ? 0 : sh_degree;
    const int nb = n_blocks_of(P);
    hipLaunchKernelGGL(kKernels[d], dim3(nb), dim3(kBlock), 0, st, f, *model, radii, reinterpret_cast<const float4*>(dsplats),
                       partials);
    if (int rc = g_err.check_hip(hipGetLastError(), "camgrad_model_kernel")) return rc;
    return finish(partials, nb, out35, st);
}

}  // extern "C"

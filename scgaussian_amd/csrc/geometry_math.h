// geometry_math.h — the per-Gaussian forward math, once: the projection, the two covariances, the input sources and the SH basis
// with its derivatives, as the geometry kernels (geometry.hip) and the camera-gradient pass (cam/camgrad.hip) both recompute them.
// Moved out of geometry.hip word for word (its gfx950 disassembly did not change: profiles/README.md).  Include it inside a
// translation unit that is compiled with contraction off (both are: -ffp-contract=off and the pragma below): every value that
// decides an INTEGER (radius, tile rectangle, depth key bits, the clamp bits) is a chain of single correctly-rounded fp32 operations
// in the order of oracle/torch_rasterizer.py::preprocess.
#pragma once

#include "scg_common.h"
#include "sh_eval.h"

#pragma clang fp contract(off)

namespace scg {

struct Mat16 { float m[16]; };

__device__ __forceinline__ Mat16 load16(const float* __restrict__ p) {
    Mat16 r;
#pragma unroll
    for (int i = 0; i < 16; ++i) r.m[i] = p[i];
    return r;
}

// Quantities of the forward projection that the backward recomputes identically.
struct Proj {
    float tx, ty, tz;            // view-space position
    float hx, hy, m_w;           // homogeneous clip x, y and 1/(w+eps)
    float t_x, t_y;              // clamped view x, y used by the Jacobian
    bool cl_x, cl_y;             // whether the 1.3*tanfov clamp was active
    float cov[6];                // 3D covariance, packed xx xy xz yy yz zz
    float T00, T01, T02, T10, T11, T12;   // Tm = J . Wm
    float u0, u1, u2, v0, v1, v2;         // Sigma . T0^T, Sigma . T1^T
    float A, B, C, det, det_inv;          // 2D covariance (+low-pass), determinant
    float L[9];                  // R.S (only when built from scale/rotation)
    float R[9];
};

// The per-Gaussian inputs that depend on nothing computed: ALL loaded together at the top of a Gaussian's work, in front of
// the cull (round 5).  Round 4's kernels fetched them where they were first used — means3D, then (behind the cull test) scales
// and rotations, then the SH record, then the opacity: four dependent round trips to HBM per Gaussian, each with a few hundred
// bytes of a wave in flight; the streaming kernels ran at 0.49-0.57 of the HBM roofline on latency, not on bytes.
struct GeoIn {
    float x, y, z, opacity;
    float a[7];                  // rotation (r, x, y, z) + scales (not yet multiplied by the modifier) — or cov3D_precomp's six
                                 // floats in a[0..5]: one set of registers for the two exclusive input paths
    float rgb[3];                // colors_precomp path
};

template <bool WITH_RGB>
__device__ __forceinline__ GeoIn load_geo_in(int i, const float* __restrict__ means3D, const float* __restrict__ opacities,
                                             const float* __restrict__ colors_precomp, const float* __restrict__ scales,
                                             const float* __restrict__ rotations, const float* __restrict__ cov3D_precomp) {
    GeoIn g;
    g.x = means3D[3 * (size_t)i + 0];
    g.y = means3D[3 * (size_t)i + 1];
    g.z = means3D[3 * (size_t)i + 2];
    g.opacity = opacities[i];
    if (cov3D_precomp) {
#pragma unroll
        for (int k = 0; k < 6; ++k) g.a[k] = cov3D_precomp[6 * (size_t)i + k];
        g.a[6] = 0.f;
    } else {
        const float4 q = *reinterpret_cast<const float4*>(rotations + 4 * (size_t)i);
        g.a[0] = q.x; g.a[1] = q.y; g.a[2] = q.z; g.a[3] = q.w;
        g.a[4] = scales[3 * (size_t)i + 0];
        g.a[5] = scales[3 * (size_t)i + 1];
        g.a[6] = scales[3 * (size_t)i + 2];
    }
    if (WITH_RGB) {
        g.rgb[0] = colors_precomp[3 * (size_t)i + 0];
        g.rgb[1] = colors_precomp[3 * (size_t)i + 1];
        g.rgb[2] = colors_precomp[3 * (size_t)i + 2];
    } else {
        g.rgb[0] = g.rgb[1] = g.rgb[2] = 0.f;
    }
    return g;
}

__device__ __forceinline__ void cov3d_from_scale_rot(const GeoIn& g, float mod, Proj& p) {
    const float r = g.a[0], x = g.a[1], y = g.a[2], z = g.a[3];
    p.R[0] = 1.0f - 2.0f * (y * y + z * z);
    p.R[1] = 2.0f * (x * y - r * z);
    p.R[2] = 2.0f * (x * z + r * y);
    p.R[3] = 2.0f * (x * y + r * z);
    p.R[4] = 1.0f - 2.0f * (x * x + z * z);
    p.R[5] = 2.0f * (y * z - r * x);
    p.R[6] = 2.0f * (x * z - r * y);
    p.R[7] = 2.0f * (y * z + r * x);
    p.R[8] = 1.0f - 2.0f * (x * x + y * y);
    const float s0 = mod * g.a[4];
    const float s1 = mod * g.a[5];
    const float s2 = mod * g.a[6];
    float* L = p.L;
    L[0] = p.R[0] * s0; L[1] = p.R[1] * s1; L[2] = p.R[2] * s2;
    L[3] = p.R[3] * s0; L[4] = p.R[4] * s1; L[5] = p.R[5] * s2;
    L[6] = p.R[6] * s0; L[7] = p.R[7] * s1; L[8] = p.R[8] * s2;
    p.cov[0] = L[0] * L[0] + L[1] * L[1] + L[2] * L[2];
    p.cov[1] = L[0] * L[3] + L[1] * L[4] + L[2] * L[5];
    p.cov[2] = L[0] * L[6] + L[1] * L[7] + L[2] * L[8];
    p.cov[3] = L[3] * L[3] + L[4] * L[4] + L[5] * L[5];
    p.cov[4] = L[3] * L[6] + L[4] * L[7] + L[5] * L[8];
    p.cov[5] = L[6] * L[6] + L[7] * L[7] + L[8] * L[8];
}

// Shared forward math: returns false when the Gaussian is behind the near plane.
__device__ __forceinline__ bool project(const FrameDev& f, const Mat16& V, const Mat16& PM, float x, float y,
                                        float z, Proj& p) {
    p.tx = V.m[0] * x + V.m[4] * y + V.m[8] * z + V.m[12];
    p.ty = V.m[1] * x + V.m[5] * y + V.m[9] * z + V.m[13];
    p.tz = V.m[2] * x + V.m[6] * y + V.m[10] * z + V.m[14];
    if (!(p.tz > kNearZ)) return false;
    p.hx = PM.m[0] * x + PM.m[4] * y + PM.m[8] * z + PM.m[12];
    p.hy = PM.m[1] * x + PM.m[5] * y + PM.m[9] * z + PM.m[13];
    const float hw = PM.m[3] * x + PM.m[7] * y + PM.m[11] * z + PM.m[15];
    p.m_w = 1.0f / (hw + 1e-7f);
    return true;
}

__device__ __forceinline__ void cov2d(const FrameDev& f, const Mat16& V, Proj& p) {
    const float txtz = p.tx / p.tz;
    const float tytz = p.ty / p.tz;
    p.cl_x = (txtz < -f.limx) || (txtz > f.limx);
    p.cl_y = (tytz < -f.limy) || (tytz > f.limy);
    p.t_x = fminf(fmaxf(txtz, -f.limx), f.limx) * p.tz;
    p.t_y = fminf(fmaxf(tytz, -f.limy), f.limy) * p.tz;
    const float tz2 = p.tz * p.tz;
    const float J00 = f.focal_x / p.tz;
    const float J02 = -(f.focal_x * p.t_x) / tz2;
    const float J11 = f.focal_y / p.tz;
    const float J12 = -(f.focal_y * p.t_y) / tz2;
    p.T00 = J00 * V.m[0] + J02 * V.m[2];
    p.T01 = J00 * V.m[4] + J02 * V.m[6];
    p.T02 = J00 * V.m[8] + J02 * V.m[10];
    p.T10 = J11 * V.m[1] + J12 * V.m[2];
    p.T11 = J11 * V.m[5] + J12 * V.m[6];
    p.T12 = J11 * V.m[9] + J12 * V.m[10];
    const float* c = p.cov;
    p.u0 = c[0] * p.T00 + c[1] * p.T01 + c[2] * p.T02;
    p.u1 = c[1] * p.T00 + c[3] * p.T01 + c[4] * p.T02;
    p.u2 = c[2] * p.T00 + c[4] * p.T01 + c[5] * p.T02;
    p.v0 = c[0] * p.T10 + c[1] * p.T11 + c[2] * p.T12;
    p.v1 = c[1] * p.T10 + c[3] * p.T11 + c[4] * p.T12;
    p.v2 = c[2] * p.T10 + c[4] * p.T11 + c[5] * p.T12;
    p.A = p.T00 * p.u0 + p.T01 * p.u1 + p.T02 * p.u2 + kLowpass;
    p.B = p.T00 * p.v0 + p.T01 * p.v1 + p.T02 * p.v2;
    p.C = p.T10 * p.v0 + p.T11 * p.v1 + p.T12 * p.v2 + kLowpass;
    p.det = p.A * p.C - p.B * p.B;
    p.det_inv = 1.0f / p.det;
}

// Load the first K coefficients (3 floats each) of one SH record into sh[(3K + 3) / 4 * 4].
template <int K>
__device__ __forceinline__ void load_sh(const float* __restrict__ rec, bool vec16, float* sh) {
    constexpr int n = 3 * K;
    if (vec16) {
        constexpr int nv = (n + 3) / 4;
        const float4* r4 = reinterpret_cast<const float4*>(rec);
#pragma unroll
        for (int i = 0; i < nv; ++i) {
            const float4 v = r4[i];
            sh[4 * i + 0] = v.x; sh[4 * i + 1] = v.y; sh[4 * i + 2] = v.z; sh[4 * i + 3] = v.w;
        }
    } else {
#pragma unroll
        for (int i = 0; i < n; ++i) sh[i] = rec[i];
#pragma unroll
        for (int i = n; i < (n + 3) / 4 * 4; ++i) sh[i] = 0.f;    // (every element defined on both paths: the array stays in registers)
    }
}

// ---------------------------------------------------------------------------------------------------
// Where a Gaussian's inputs come from: the kernels below are written once over a SOURCE.
//   TensorSource  the operator's seven input tensors, ACTIVATED values (reference gaussian_renderer/__init__.py:100-108)
//   ModelSource   the reference model's RAW parameter tensors (scene/gaussian_model.py:452-468; include/scg_raster.h ScgModel):
//                 position = rayo + rayd * zval or bg_xyz, sigmoid / exp / normalize in registers, the SH record read from
//                 its two parts (features_dc, features_rest) — what the reference's getters (:105-152) compute with ~25 torch
//                 launches and a 192 B / Gaussian concatenation per render() call
// ---------------------------------------------------------------------------------------------------
struct TensorSource {
    const float* means3D; const float* opacities; const float* shs; const float* colors_precomp;
    const float* scales; const float* rotations; const float* cov3D_precomp;
    int M, sh_vec16;
    __device__ __forceinline__ bool has_cov() const { return cov3D_precomp != nullptr; }
    template <bool WITH_RGB>
    __device__ __forceinline__ GeoIn load(int i) const {
        return load_geo_in<WITH_RGB>(i, means3D, opacities, colors_precomp, scales, rotations, cov3D_precomp);
    }
    template <int K>
    __device__ __forceinline__ void load_sh(int i, float* sh) const { scg::load_sh<K>(shs + (size_t)i * M * 3, sh_vec16 != 0, sh); }
};

// The reference's activations (scene/gaussian_model.py:37-51): ONE definition for the forward, the backward's recomputation and
// scg_model_activate — the same instructions, hence the same bits, wherever an activated value is needed.
constexpr float kNormalizeEps = 1e-12f;                       // torch.nn.functional.normalize's eps
__device__ __forceinline__ float act_opacity(float logit) { return 1.0f / (1.0f + expf(-logit)); }
__device__ __forceinline__ float act_scale(float log_s) { return expf(log_s); }
__device__ __forceinline__ float quat_denominator(float r, float x, float y, float z) {
    return fmaxf(sqrtf(r * r + x * x + y * y + z * z), kNormalizeEps);
}

constexpr int kRestCoeffs = 15;                               // features_rest is (n, 15, 3): M = 16 records in two parts

struct ModelSource {
    ScgModel m;
    __device__ __forceinline__ bool has_cov() const { return false; }
    // (lane's set and index inside it: the two sets are indexed one behind the other)
    __device__ __forceinline__ bool locate(int i, int& j) const {
        const bool ray = i < m.ray.count;
        j = ray ? i : i - m.ray.count;
        return ray;
    }
    // A Gaussian's raw parameters as loaded (no arithmetic: the backward issues these loads next to its other loads and
    // activates behind them), and their activation.  den_out / rayd_out (backward only): the quaternion's denominator
    // max(|q|, eps) and the ray direction — what the derivatives of normalize and of rayo + rayd * zval need.
    struct Raw { float o[3], d[3], zv, logit, ls[3]; float4 q; bool ray; };
    __device__ __forceinline__ Raw load_raw(int i) const {
        int j;
        Raw r;
        r.ray = locate(i, j);
        r.zv = 0.f; r.o[0] = r.o[1] = r.o[2] = 0.f;
        if (r.ray) {
            r.zv = m.ray.zval[j];
#pragma unroll
            for (int c = 0; c < 3; ++c) { r.o[c] = m.ray.rayo[3 * (size_t)j + c]; r.d[c] = m.ray.rayd[3 * (size_t)j + c]; }
        } else {
#pragma unroll
            for (int c = 0; c < 3; ++c) r.d[c] = m.bg.xyz[3 * (size_t)j + c];
        }
        const float* op = r.ray ? m.ray.opacity : m.bg.opacity;
        const float* sc = r.ray ? m.ray.scaling : m.bg.scaling;
        const float* ro = r.ray ? m.ray.rotation : m.bg.rotation;
        r.logit = op[j];
        r.q = *reinterpret_cast<const float4*>(ro + 4 * (size_t)j);
#pragma unroll
        for (int c = 0; c < 3; ++c) r.ls[c] = sc[3 * (size_t)j + c];
        return r;
    }
    static __device__ __forceinline__ GeoIn activate(const Raw& r, float* den_out = nullptr, float* rayd_out = nullptr) {
        GeoIn g;
        // rayo + rayd * zval: two roundings (this file is compiled with contraction off), as torch evaluates it (:127)
        g.x = r.ray ? r.o[0] + r.d[0] * r.zv : r.d[0];
        g.y = r.ray ? r.o[1] + r.d[1] * r.zv : r.d[1];
        g.z = r.ray ? r.o[2] + r.d[2] * r.zv : r.d[2];
        g.opacity = act_opacity(r.logit);
        const float den = quat_denominator(r.q.x, r.q.y, r.q.z, r.q.w);
        g.a[0] = r.q.x / den; g.a[1] = r.q.y / den; g.a[2] = r.q.z / den; g.a[3] = r.q.w / den;
        g.a[4] = act_scale(r.ls[0]); g.a[5] = act_scale(r.ls[1]); g.a[6] = act_scale(r.ls[2]);
        g.rgb[0] = g.rgb[1] = g.rgb[2] = 0.f;
        if (den_out) *den_out = den;
        if (rayd_out) { rayd_out[0] = r.ray ? r.d[0] : 0.f; rayd_out[1] = r.ray ? r.d[1] : 0.f; rayd_out[2] = r.ray ? r.d[2] : 0.f; }
        return g;
    }
    template <bool WITH_RGB>
    __device__ __forceinline__ GeoIn load(int i) const { return activate(load_raw(i)); }
    // coefficient 0 from features_dc (12 bytes per Gaussian: a dense stream at degree 0), 1 .. K-1 from the head of the
    // Gaussian's 180-byte features_rest record
    template <int K>
    __device__ __forceinline__ void load_sh(int i, float* sh) const {
        int j;
        const bool ray = locate(i, j);
        const float* dc = (ray ? m.ray.features_dc : m.bg.features_dc) + 3 * (size_t)j;
        sh[0] = dc[0]; sh[1] = dc[1]; sh[2] = dc[2];
        if (K > 1) {
            const float* rest = (ray ? m.ray.features_rest : m.bg.features_rest) + 3 * kRestCoeffs * (size_t)j;
#pragma unroll
            for (int k = 0; k < 3 * (K - 1); ++k) sh[3 + k] = rest[k];
        }
#pragma unroll
        for (int k = 3 * K; k < (3 * K + 3) / 4 * 4; ++k) sh[k] = 0.f;
    }
};

// The K = (DEG + 1)^2 basis values at a unit direction and their derivatives by its three components (the polynomials of
// utils/sh_utils.py:57-103 and their analytic gradients).
template <int DEG>
__device__ __forceinline__ void sh_basis_grads(float x, float y, float z, float* basis, float* bx, float* by, float* bz) {
    basis[0] = kC0; bx[0] = by[0] = bz[0] = 0.f;
    if (DEG > 0) {
        basis[1] = -kC1 * y; bx[1] = 0.f; by[1] = -kC1; bz[1] = 0.f;
        basis[2] = kC1 * z;  bx[2] = 0.f; by[2] = 0.f; bz[2] = kC1;
        basis[3] = -kC1 * x; bx[3] = -kC1; by[3] = 0.f; bz[3] = 0.f;
    }
    if (DEG > 1) {
        const float xx = x * x, yy = y * y, zz = z * z, xy = x * y, yz = y * z, xz = x * z;
        basis[4] = kC2[0] * xy;                    bx[4] = kC2[0] * y; by[4] = kC2[0] * x; bz[4] = 0.f;
        basis[5] = kC2[1] * yz;                    bx[5] = 0.f; by[5] = kC2[1] * z; bz[5] = kC2[1] * y;
        basis[6] = kC2[2] * (2.0f * zz - xx - yy); bx[6] = kC2[2] * -2.0f * x; by[6] = kC2[2] * -2.0f * y; bz[6] = kC2[2] * 4.0f * z;
        basis[7] = kC2[3] * xz;                    bx[7] = kC2[3] * z; by[7] = 0.f; bz[7] = kC2[3] * x;
        basis[8] = kC2[4] * (xx - yy);             bx[8] = kC2[4] * 2.0f * x; by[8] = kC2[4] * -2.0f * y; bz[8] = 0.f;
        if (DEG > 2) {
            basis[9] = kC3[0] * y * (3.0f * xx - yy);
            bx[9] = kC3[0] * 6.0f * xy; by[9] = kC3[0] * (3.0f * xx - 3.0f * yy); bz[9] = 0.f;
            basis[10] = kC3[1] * xy * z;
            bx[10] = kC3[1] * yz; by[10] = kC3[1] * xz; bz[10] = kC3[1] * xy;
            basis[11] = kC3[2] * y * (4.0f * zz - xx - yy);
            bx[11] = kC3[2] * -2.0f * xy; by[11] = kC3[2] * (4.0f * zz - xx - 3.0f * yy); bz[11] = kC3[2] * 8.0f * yz;
            basis[12] = kC3[3] * z * (2.0f * zz - 3.0f * xx - 3.0f * yy);
            bx[12] = kC3[3] * -6.0f * xz; by[12] = kC3[3] * -6.0f * yz; bz[12] = kC3[3] * (6.0f * zz - 3.0f * xx - 3.0f * yy);
            basis[13] = kC3[4] * x * (4.0f * zz - xx - yy);
            bx[13] = kC3[4] * (4.0f * zz - 3.0f * xx - yy); by[13] = kC3[4] * -2.0f * xy; bz[13] = kC3[4] * 8.0f * xz;
            basis[14] = kC3[5] * z * (xx - yy);
            bx[14] = kC3[5] * 2.0f * xz; by[14] = kC3[5] * -2.0f * yz; bz[14] = kC3[5] * (xx - yy);
            basis[15] = kC3[6] * x * (xx - 3.0f * yy);
            bx[15] = kC3[6] * (3.0f * xx - 3.0f * yy); by[15] = kC3[6] * -6.0f * xy; bz[15] = 0.f;
        }
    }
}

}  // namespace scg

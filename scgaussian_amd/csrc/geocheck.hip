// geocheck.hip — the reference's cross-view depth consistency check (include/scg_geocheck.h).
//
//   utils/geo_check.py:25-31    get_pairs: the nearest other cameras of every camera            -> geocheck_setup_kernel
//   utils/geo_check.py:91-128   reproject_with_depth: reference -> source -> reference
//   utils/geo_check.py:33-88    geocheck: two thresholds, a vote, the mean of the agreeing depths -> geocheck_kernel
//
// The rule decides a reference pixel from that pixel alone, so the check is one thread per pixel with the J source views of its
// view walked in registers.  Everything that does not depend on the pixel is composed once per (view, source) pair by the setup
// kernel, in fp64: a GeoRec of two 3x3 matrices, two translations and the source's index.  A workgroup works on one view, so the
// record of slot s has the same address for all its threads (blockIdx.y and the loop counter only): the compiler fetches it with
// scalar loads, and what a thread itself loads is its own depth and the four taps of the source depth map.  No LDS, no atomics.
//
// Compiled with -ffp-contract=off: the reference is numpy float64 between its fp32 casts, and tests/geocheck_refs.py restates the
// arithmetic below operation by operation; a fused multiply-add would round differently from both.
#include <math.h>

#include "scg_common.h"
#include "../../include/scg_geocheck.h"

namespace scg {

constexpr int kGeoTileW = 32, kGeoTileH = 8;     // kBlock pixels: a wave covers two rows of 32, neighbours gather from neighbouring taps
constexpr int kGeoMaxViews = 1024, kGeoMaxSrc = 64;
constexpr int kGeoSetupBlock = 64;
constexpr double kGeoSelfDist = 1e3;             // utils/geo_check.py:28
static_assert(kGeoTileW * kGeoTileH == kBlock, "one thread per pixel of the tile");

struct GeoRec {
    double M1[9], t1[3];     // K_j R_ji K_i^-1, K_j t_ji: (u d, v d, d) of the reference -> homogeneous source pixel
    double M2[9], t2[3];     // R_ij K_j^-1, t_ij: (xs s, ys s, s) of the source -> reference camera space
    int32_t j, pad;
};
static_assert(sizeof(GeoRec) == 200, "24 doubles and the source index");

struct GeoLayout { size_t pairs, K, recs, total; int J; };

static GeoLayout geo_layout(int N, int num_src) {
    GeoLayout L;
    L.J = num_src < N ? num_src : N;
    auto up = [](size_t b) { return (b + 255) / 256 * 256; };
    L.pairs = 0;
    L.K = up((size_t)N * L.J * sizeof(int32_t));
    L.recs = L.K + up((size_t)N * 9 * sizeof(double));
    L.total = L.recs + up((size_t)N * L.J * sizeof(GeoRec));
    return L;
}

static bool geo_sizes_ok(int N, int num_src) { return N >= 1 && N <= kGeoMaxViews && num_src >= 1 && num_src <= kGeoMaxSrc; }

// ---- fp64 matrix helpers: fixed operation order (tests/geocheck_refs.py repeats it) --------------------------------------------
// adjugate over determinant; a singular matrix gives inf / NaN entries
__device__ void inv3(const double* a, double* b) {
    const double c00 = a[4] * a[8] - a[5] * a[7], c01 = a[5] * a[6] - a[3] * a[8], c02 = a[3] * a[7] - a[4] * a[6];
    const double det = a[0] * c00 + a[1] * c01 + a[2] * c02;
    const double r = 1.0 / det;
    b[0] = c00 * r; b[1] = (a[2] * a[7] - a[1] * a[8]) * r; b[2] = (a[1] * a[5] - a[2] * a[4]) * r;
    b[3] = c01 * r; b[4] = (a[0] * a[8] - a[2] * a[6]) * r; b[5] = (a[2] * a[3] - a[0] * a[5]) * r;
    b[6] = c02 * r; b[7] = (a[1] * a[6] - a[0] * a[7]) * r; b[8] = (a[0] * a[4] - a[1] * a[3]) * r;
}

__device__ void inv4(const double* a, double* b) {
    const double s0 = a[0] * a[5] - a[4] * a[1], s1 = a[0] * a[6] - a[4] * a[2], s2 = a[0] * a[7] - a[4] * a[3];
    const double s3 = a[1] * a[6] - a[5] * a[2], s4 = a[1] * a[7] - a[5] * a[3], s5 = a[2] * a[7] - a[6] * a[3];
    const double c5 = a[10] * a[15] - a[14] * a[11], c4 = a[9] * a[15] - a[13] * a[11], c3 = a[9] * a[14] - a[13] * a[10];
    const double c2 = a[8] * a[15] - a[12] * a[11], c1 = a[8] * a[14] - a[12] * a[10], c0 = a[8] * a[13] - a[12] * a[9];
    const double det = s0 * c5 - s1 * c4 + s2 * c3 + s3 * c2 - s4 * c1 + s5 * c0;
    const double r = 1.0 / det;
    b[0] = (a[5] * c5 - a[6] * c4 + a[7] * c3) * r;
    b[1] = (a[2] * c4 - a[1] * c5 - a[3] * c3) * r;
    b[2] = (a[13] * s5 - a[14] * s4 + a[15] * s3) * r;
    b[3] = (a[10] * s4 - a[9] * s5 - a[11] * s3) * r;
    b[4] = (a[6] * c2 - a[4] * c5 - a[7] * c1) * r;
    b[5] = (a[0] * c5 - a[2] * c2 + a[3] * c1) * r;
    b[6] = (a[14] * s2 - a[12] * s5 - a[15] * s1) * r;
    b[7] = (a[8] * s5 - a[10] * s2 + a[11] * s1) * r;
    b[8] = (a[4] * c4 - a[5] * c2 + a[7] * c0) * r;
    b[9] = (a[1] * c2 - a[0] * c4 - a[3] * c0) * r;
    b[10] = (a[12] * s4 - a[13] * s2 + a[15] * s0) * r;
    b[11] = (a[9] * s2 - a[8] * s4 - a[11] * s0) * r;
    b[12] = (a[5] * c1 - a[4] * c3 - a[6] * c0) * r;
    b[13] = (a[0] * c3 - a[1] * c1 + a[2] * c0) * r;
    b[14] = (a[13] * s1 - a[12] * s3 - a[14] * s0) * r;
    b[15] = (a[8] * s3 - a[9] * s1 + a[10] * s0) * r;
}

// c = a b, n x n row-major, every element summed over k in rising order
template <int n>
__device__ void matmul(const double* a, const double* b, double* c) {
    for (int r = 0; r < n; ++r)
        for (int q = 0; q < n; ++q) {
            double s = a[r * n] * b[q];
            for (int k = 1; k < n; ++k) s = s + a[r * n + k] * b[k * n + q];
            c[r * n + q] = s;
        }
}

// the order get_pairs sorts by: distance, NaN last, equal distances by index
__device__ __forceinline__ bool pair_before(double da, int ia, double db, int ib) {
    const bool na = da != da, nb = db != db;
    if (na || nb) return na == nb ? ia < ib : nb;
    return da < db || (da == db && ia < ib);
}

__global__ __launch_bounds__(kGeoSetupBlock) void geocheck_setup_kernel(const double* __restrict__ intrs, const double* __restrict__ exts,
                                                                        int N, int J, int32_t* __restrict__ pairs,
                                                                        double* __restrict__ Ks, GeoRec* __restrict__ recs) {
    const int i = blockIdx.x * kGeoSetupBlock + threadIdx.x;
    if (i >= N) return;
    double Ki[9], Ei[16], Kinv_i[9], Einv_i[16];
    for (int k = 0; k < 9; ++k) Ki[k] = intrs[(size_t)i * 9 + k];
    for (int k = 0; k < 16; ++k) Ei[k] = exts[(size_t)i * 16 + k];
    inv3(Ki, Kinv_i);
    inv4(Ei, Einv_i);
    for (int k = 0; k < 9; ++k) Ks[(size_t)i * 9 + k] = Ki[k];
    const double px = Ei[3], py = Ei[7], pz = Ei[11];

    int last = -1;
    double last_d = 0.0;
    for (int s = 0; s < J; ++s) {
        // the next camera in get_pairs' order behind the one of the previous slot: nothing is stored, N * J distances are formed again
        int best = -1;
        double best_d = 0.0;
        for (int c = 0; c < N; ++c) {
            const double dx = px - exts[(size_t)c * 16 + 3], dy = py - exts[(size_t)c * 16 + 7], dz = pz - exts[(size_t)c * 16 + 11];
            const double dc = c == i ? kGeoSelfDist : sqrt(dx * dx + dy * dy + dz * dz);
            if (last >= 0 && !pair_before(last_d, last, dc, c)) continue;
            if (best < 0 || pair_before(dc, c, best_d, best)) { best = c; best_d = dc; }
        }
        if (best < 0) best = i;            // J <= N: there always is one
        last = best;
        last_d = best_d;
        const int j = best;
        pairs[(size_t)i * J + s] = j;

        double Kj[9], Ej[16], Kinv_j[9], Einv_j[16], A[16], B[16], R[9], T[9];
        for (int k = 0; k < 9; ++k) Kj[k] = intrs[(size_t)j * 9 + k];
        for (int k = 0; k < 16; ++k) Ej[k] = exts[(size_t)j * 16 + k];
        inv3(Kj, Kinv_j);
        inv4(Ej, Einv_j);
        matmul<4>(Ej, Einv_i, A);          // [R_ji | t_ji]: reference camera -> source camera
        matmul<4>(Ei, Einv_j, B);          // [R_ij | t_ij]: source camera -> reference camera
        GeoRec rec;
        for (int r = 0; r < 3; ++r)
            for (int q = 0; q < 3; ++q) R[r * 3 + q] = A[r * 4 + q];
        matmul<3>(Kj, R, T);
        matmul<3>(T, Kinv_i, rec.M1);
        for (int r = 0; r < 3; ++r) rec.t1[r] = Kj[r * 3] * A[3] + Kj[r * 3 + 1] * A[7] + Kj[r * 3 + 2] * A[11];
        for (int r = 0; r < 3; ++r)
            for (int q = 0; q < 3; ++q) R[r * 3 + q] = B[r * 4 + q];
        matmul<3>(R, Kinv_j, rec.M2);
        rec.t2[0] = B[3]; rec.t2[1] = B[7]; rec.t2[2] = B[11];
        rec.j = j;
        rec.pad = 0;
        recs[(size_t)i * J + s] = rec;
    }
}

// oracle/geo_check_oracle.py bilinear_zero_border for one coordinate pair (the fp32 casts of utils/geo_check.py:109-110)
__device__ __forceinline__ float sample_zero_border(const float* __restrict__ src, int H, int W, float xs32, float ys32) {
    if (!(isfinite(xs32) && isfinite(ys32))) return 0.0f;
    const float xf = floorf(xs32), yf = floorf(ys32);
    // a floor beyond int32 is outside every image: decided on the float, the cast would be undefined
    if (!(fabsf(xf) < 2147483648.0f && fabsf(yf) < 2147483648.0f)) return 0.0f;
    const int x0 = (int)xf, y0 = (int)yf;
    const double wx1 = (double)xs32 - (double)xf, wy1 = (double)ys32 - (double)yf;
    const double wx0 = 1.0 - wx1, wy0 = 1.0 - wy1;
    double acc = 0.0;
#pragma unroll
    for (int oy = 0; oy < 2; ++oy) {
#pragma unroll
        for (int ox = 0; ox < 2; ++ox) {
            const int xi = x0 + ox, yi = y0 + oy;
            if (xi >= 0 && xi < W && yi >= 0 && yi < H) {          // a tap outside adds 0 * wx * wy = +0
                const double v = (double)src[(size_t)yi * W + xi];
                acc = acc + v * (ox ? wx1 : wx0) * (oy ? wy1 : wy0);
            }
        }
    }
    return (float)acc;
}

__global__ __launch_bounds__(kBlock) void geocheck_kernel(const float* __restrict__ depths, const GeoRec* __restrict__ recs,
                                                          const double* __restrict__ Ks, int H, int W, int J, int tiles_x,
                                                          double dist_thresh, double depth_thresh, int view_thresh,
                                                          uint8_t* __restrict__ votes_out, float* __restrict__ masks,
                                                          float* __restrict__ filtered) {
    const int view = blockIdx.y;
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const int x = tx * kGeoTileW + (threadIdx.x & (kGeoTileW - 1)), y = ty * kGeoTileH + threadIdx.x / kGeoTileW;
    if (x >= W || y >= H) return;
    const size_t plane = (size_t)H * W;
    const size_t pix = (size_t)view * plane + (size_t)y * W + x;
    const double d = (double)depths[pix], u = (double)x, v = (double)y;
    const double* __restrict__ K = Ks + (size_t)view * 9;
    const GeoRec* __restrict__ rec = recs + (size_t)view * J;
    const double ud = u * d, vd = v * d;

    int votes = 0;
    double sum = 0.0;
    for (int s = 0; s < J; ++s) {
        const GeoRec& r = rec[s];
        if ((unsigned)r.j >= gridDim.y) continue;          // a workspace the setup never wrote: no source, no read outside depths
        const double k0 = r.M1[0] * ud + r.M1[1] * vd + r.M1[2] * d + r.t1[0];
        const double k1 = r.M1[3] * ud + r.M1[4] * vd + r.M1[5] * d + r.t1[1];
        const double k2 = r.M1[6] * ud + r.M1[7] * vd + r.M1[8] * d + r.t1[2];
        const double xs = k0 / k2, ys = k1 / k2;
        const double smp = (double)sample_zero_border(depths + (size_t)r.j * plane, H, W, (float)xs, (float)ys);
        const double a = xs * smp, b = ys * smp;
        const double X0 = r.M2[0] * a + r.M2[1] * b + r.M2[2] * smp + r.t2[0];
        const double X1 = r.M2[3] * a + r.M2[4] * b + r.M2[5] * smp + r.t2[1];
        const double X2 = r.M2[6] * a + r.M2[7] * b + r.M2[8] * smp + r.t2[2];
        const float d_back = (float)X2;
        const double h0 = K[0] * X0 + K[1] * X1 + K[2] * X2;
        const double h1 = K[3] * X0 + K[4] * X1 + K[5] * X2;
        const double h2 = K[6] * X0 + K[7] * X1 + K[8] * X2;
        const float ub = (float)(h0 / h2), vb = (float)(h1 / h2);
        const double moved = hypot((double)ub - u, (double)vb - v);
        const double rel = fabs((double)d_back - d) / d;
        const bool agree = moved < dist_thresh && rel < depth_thresh;          // NaN: false
        votes += agree ? 1 : 0;
        sum = sum + (agree ? (double)d_back : 0.0);
    }
    const float mask = votes > view_thresh ? 1.0f : 0.0f;
    const float mean = (float)((sum + d) / (double)(votes + 1));
    votes_out[pix] = (uint8_t)votes;
    masks[pix] = mask;
    filtered[pix] = mean * mask;           // a product, not a select: utils/geo_check.py:81
}

}  // namespace scg

using namespace scg;

extern "C" {

size_t scg_geocheck_workspace_bytes(int32_t N, int32_t num_src) {
    if (!geo_sizes_ok(N, num_src)) return 0;
    return geo_layout(N, num_src).total;
}

int32_t scg_geocheck_tile(int32_t axis) { return axis == 0 ? kGeoTileW : (axis == 1 ? kGeoTileH : 0); }

int scg_geocheck_setup(const double* intrs, const double* exts, int32_t N, int32_t num_src, void* workspace, size_t workspace_bytes,
                       void* stream) {
    if (!geo_sizes_ok(N, num_src))
        return fail(SCG_E_RANGE, "geocheck_setup: N = %d (1 ... %d) or num_src = %d (1 ... %d) out of range", N, kGeoMaxViews, num_src, kGeoMaxSrc);
    if (!intrs || !exts || !workspace) return fail(SCG_E_NULL, "geocheck_setup pointer is NULL");
    const GeoLayout L = geo_layout(N, num_src);
    if (workspace_bytes < L.total) return fail(SCG_E_SCRATCH, "geocheck_setup: workspace of %zu bytes < %zu", workspace_bytes, L.total);
    if (reinterpret_cast<uintptr_t>(workspace) % 8) return fail(SCG_E_ALIGN, "geocheck_setup: workspace not 8-byte aligned");
    char* ws = reinterpret_cast<char*>(workspace);
    hipLaunchKernelGGL(geocheck_setup_kernel, dim3((N + kGeoSetupBlock - 1) / kGeoSetupBlock), dim3(kGeoSetupBlock), 0,
                       reinterpret_cast<hipStream_t>(stream), intrs, exts, N, L.J, reinterpret_cast<int32_t*>(ws + L.pairs),
                       reinterpret_cast<double*>(ws + L.K), reinterpret_cast<GeoRec*>(ws + L.recs));
    return check_hip(hipGetLastError(), "geocheck_setup_kernel");
}

int scg_geocheck(const float* depths, int32_t N, int32_t H, int32_t W, int32_t num_src, double dist_thresh, double depth_thresh,
                 int32_t view_thresh, const void* workspace, size_t workspace_bytes, uint8_t* votes, float* masks, float* filtered,
                 void* stream) {
    if (!geo_sizes_ok(N, num_src))
        return fail(SCG_E_RANGE, "geocheck: N = %d (1 ... %d) or num_src = %d (1 ... %d) out of range", N, kGeoMaxViews, num_src, kGeoMaxSrc);
    if (H < 1 || W < 1 || (int64_t)H * W >= (1ll << 31)) return fail(SCG_E_RANGE, "geocheck: image of %d x %d out of range", H, W);
    const int64_t tiles_x = (W + kGeoTileW - 1) / kGeoTileW, tiles_y = (H + kGeoTileH - 1) / kGeoTileH;
    // a launch holds fewer than 2^32 threads per axis: only images thinner than a tile and longer than 2^27 pixels get here
    if (tiles_x * tiles_y * kBlock >= (1ll << 32)) return fail(SCG_E_RANGE, "geocheck: %d x %d needs too many pixel tiles", H, W);
    if (!depths || !workspace || !votes || !masks || !filtered) return fail(SCG_E_NULL, "geocheck pointer is NULL");
    const GeoLayout L = geo_layout(N, num_src);
    if (workspace_bytes < L.total) return fail(SCG_E_SCRATCH, "geocheck: workspace of %zu bytes < %zu", workspace_bytes, L.total);
    if (reinterpret_cast<uintptr_t>(workspace) % 8) return fail(SCG_E_ALIGN, "geocheck: workspace not 8-byte aligned");
    const char* ws = reinterpret_cast<const char*>(workspace);
    hipLaunchKernelGGL(geocheck_kernel, dim3((unsigned)(tiles_x * tiles_y), N), dim3(kBlock), 0, reinterpret_cast<hipStream_t>(stream),
                       depths, reinterpret_cast<const GeoRec*>(ws + L.recs), reinterpret_cast<const double*>(ws + L.K), H, W, L.J,
                       (int)tiles_x, dist_thresh, depth_thresh, view_thresh, votes, masks, filtered);
    return check_hip(hipGetLastError(), "geocheck_kernel");
}

}  // extern "C"

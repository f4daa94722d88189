// virtualwarp.hip — libscg_vw.so: the virtual-view warp loss and the edge-aware depth smoothness of utils/loss_utils.py, forward
// and backward (include/vw/scg_virtualwarp.h states the arithmetic).
//
// The rule is local: a pixel's warp needs that pixel, its loss the 5x5 window around it, its gradient the windows it lies in.  So:
//
//   vw_warp_kernel      a workgroup is a 16 x 16 pixel tile inside ONE view (blockIdx.y: the view's record has one address for all
//                       its threads): project, the in-bounds byte, torch's bilinear sample of the three channels and the sample's
//                       derivative with respect to the pixel's depth, both to scratch
//   vw_ssim_kernel      a tile of pixels, all views in turn: the 5x5 statistics behind the reflection, s_v, the winner, the loss
//                       map, the winner's four coefficient maps per channel, and the tile's partial sum (reduce.h)
//   vw_fold_kernel      one workgroup folds the partial sums in a fixed order and divides
//   vw_backward_kernel  one thread per pixel q GATHERS: over the 5x5 centres around q, each weighted by how many positions of its
//                       padded window reflect onto q, view by view, so that dL/dy_v(q) is a sum of its own and meets dy_v/ddepth
//                       the way torch's chain does (a NaN depth gives a NaN depth gradient there and here)
//   vw_smooth_kernel / vw_smooth_fold_kernel / vw_smooth_backward_kernel   the smoothness loss, the same way
//
// No scatter, no atomics, no allocation, no host read.  Compiled with -ffp-contract=off.  fp32 in, fp32 out, fp64 in between (the
// header says why): the kernels are bound by their gathers, not by the fp64 rate.
#include "../../include/vw/scg_virtualwarp.h"
#include "host_error.h"
#include "reduce.h"

#pragma clang fp contract(off)

namespace scg {
namespace {

constexpr int kSide = SCG_VW_TILE;
constexpr int kNW = kBlock / kWave;
static_assert(kSide * kSide == kBlock && SCG_VW_SMOOTH_PIXELS == kBlock, "one pixel per thread");

thread_local ErrorText g_err = {};

struct WarpLayout {
    size_t hw, y, dyd, partial, coef, total;      // offsets and total in BYTES: the fp64 regions first
    int tiles_x, tiles_y;
};

bool warp_layout(int64_t nv, int64_t H, int64_t W, WarpLayout* l) {
    if (nv < 1 || nv > SCG_VW_MAX_VIEWS || H < SCG_VW_MIN_DIM || W < SCG_VW_MIN_DIM || H > SCG_VW_MAX_DIM || W > SCG_VW_MAX_DIM) return false;
    l->hw = (size_t)H * (size_t)W;
    l->tiles_x = (int)((W + kSide - 1) / kSide);
    l->tiles_y = (int)((H + kSide - 1) / kSide);
    l->y = 0;
    l->dyd = l->y + (size_t)nv * 3 * l->hw * sizeof(double);
    l->partial = l->dyd + (size_t)nv * 3 * l->hw * sizeof(double);
    l->coef = l->partial + (size_t)l->tiles_x * l->tiles_y * sizeof(double);
    l->total = l->coef + 12 * l->hw * sizeof(float);
    return true;
}

struct WarpArgs {
    int nv, H, W, tiles_x, tiles;
    const float* img;           // (3,H,W)
    const float* depth;         // (H,W)
    const uint8_t* mask;
    const float* colors;        // (nv,3,H,W)
    const float* records;       // (nv,12)
    const float* upstream;
    float* loss;
    float* loss_map;
    int8_t* winner;
    uint8_t* in_bounds;
    double* y;                  // scratch (nv,3,H,W), fp64
    double* dyd;                // scratch (nv,3,H,W), fp64
    float* coef;                // scratch (4,3,H,W): A, A', B, C
    double* partial;            // scratch (tiles), fp64
    float* d_img;
    float* d_depth;
};

__device__ __forceinline__ bool tile_pixel(const WarpArgs& a, int& px, int& py) {
    const int tile = blockIdx.x;
    const int ty = tile / a.tiles_x, tx = tile - ty * a.tiles_x;
    px = tx * kSide + (threadIdx.x & (kSide - 1));
    py = ty * kSide + (threadIdx.x >> 4);
    return px < a.W && py < a.H;
}

__global__ __launch_bounds__(kBlock) void vw_warp_kernel(WarpArgs a) {
    const int v = blockIdx.y;
    int px, py;
    if (v >= a.nv || !tile_pixel(a, px, py)) return;
    const float* __restrict__ r = a.records + (size_t)v * SCG_VW_RECORD_FLOATS;
    const int H = a.H, W = a.W;
    const size_t hw = (size_t)H * W, q = (size_t)py * W + px;
    const double fx = (double)px, fy = (double)py, d = (double)a.depth[q];
    const double ax = (double)r[0] * fx + (double)r[1] * fy + (double)r[2];
    const double ay = (double)r[3] * fx + (double)r[4] * fy + (double)r[5];
    const double az = (double)r[6] * fx + (double)r[7] * fy + (double)r[8];
    const double X = d * ax + (double)r[9], Y = d * ay + (double)r[10], Z = d * az + (double)r[11];
    const double Zp = Z + 1e-8;
    const double x = X / Zp, y = Y / Zp;
    const double nx = 2.0 * x / (double)(W - 1) - 1.0;
    const double ny = 2.0 * y / (double)(H - 1) - 1.0;
    a.in_bounds[(size_t)v * hw + q] = (fabs(nx) <= 1.0 && fabs(ny) <= 1.0) ? 1 : 0;

    // torch's grid_sample(bilinear, zeros, align_corners=False): value and derivative with respect to the tap position
    const double ix = ((nx + 1.0) * (double)W - 1.0) / 2.0;
    const double iy = ((ny + 1.0) * (double)H - 1.0) / 2.0;
    double val[3] = {0.0, 0.0, 0.0}, dvx[3] = {0.0, 0.0, 0.0}, dvy[3] = {0.0, 0.0, 0.0};
    const double xf = floor(ix), yf = floor(iy);
    // a NaN samples zero; a floor beyond int32 is outside every image: decided on the float, the cast would be undefined
    if (ix == ix && iy == iy && fabs(xf) < 2147483648.0 && fabs(yf) < 2147483648.0) {
        const double x1 = xf + 1.0, y1 = yf + 1.0;
        const double wx[2] = {x1 - ix, ix - xf}, wy[2] = {y1 - iy, iy - yf};
        const int x0 = (int)xf, y0 = (int)yf;
        const float* __restrict__ src = a.colors + (size_t)v * 3 * hw;
#pragma unroll
        for (int k = 0; k < 4; ++k) {              // nw, ne, sw, se
            const int64_t tx = (int64_t)x0 + (k & 1), ty = (int64_t)y0 + (k >> 1);
            if (tx >= 0 && tx < W && ty >= 0 && ty < H) {
                const size_t p = (size_t)ty * W + (size_t)tx;
                const double w = wx[k & 1] * wy[k >> 1];
                const double sx = (k & 1) ? wy[k >> 1] : -wy[k >> 1];
                const double sy = (k >> 1) ? wx[k & 1] : -wx[k & 1];
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const double t = (double)src[(size_t)c * hw + p];
                    val[c] = val[c] + t * w;
                    dvx[c] = dvx[c] + t * sx;
                    dvy[c] = dvy[c] + t * sy;
                }
            }
        }
    }
    // d(tap position)/d(depth): dx/dd = (a_x (Z + 1e-8) - X a_z) / (Z + 1e-8)^2, then 2 / (W - 1) and W / 2
    const double zz = Zp * Zp;
    const double dixdd = (ax * Zp - X * az) / zz * (2.0 / (double)(W - 1)) * ((double)W / 2.0);
    const double diydd = (ay * Zp - Y * az) / zz * (2.0 / (double)(H - 1)) * ((double)H / 2.0);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const size_t e = ((size_t)v * 3 + c) * hw + q;
        a.y[e] = val[c];
        a.dyd[e] = dvx[c] * dixdd + dvy[c] * diydd;
    }
}

// ReflectionPad2d(2) for n >= 3 and -2 <= i <= n + 1
__device__ __forceinline__ int reflect(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * (n - 1) - i : i); }

constexpr double kC1 = 0.01 * 0.01, kC2 = 0.03 * 0.03;

__global__ __launch_bounds__(kBlock) void vw_ssim_kernel(WarpArgs a) {
    __shared__ double s_red[kNW];
    int px, py;
    const bool active = tile_pixel(a, px, py);
    const int H = a.H, W = a.W;
    const size_t hw = (size_t)H * W;
    double lossv = 0.0;
    if (active) {
        const size_t p = (size_t)py * W + px;
        int col[5], row[5];
#pragma unroll
        for (int k = 0; k < 5; ++k) { col[k] = reflect(px + k - 2, W); row[k] = reflect(py + k - 2, H); }
        double best = 0.0;
        float bc[12], cc[12];
        int w = -1;
#pragma unroll
        for (int k = 0; k < 12; ++k) bc[k] = 0.0f;
        for (int v = 0; v < a.nv; ++v) {
            double s;
            if (a.in_bounds[(size_t)v * hw + p]) {
                double acc = 0.0;
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const float* __restrict__ xi = a.img + (size_t)c * hw;
                    const double* __restrict__ yi = a.y + ((size_t)v * 3 + c) * hw;
                    double sx = 0.0, sy = 0.0, sxx = 0.0, syy = 0.0, sxy = 0.0;
#pragma unroll
                    for (int j = 0; j < 5; ++j)
#pragma unroll
                        for (int i = 0; i < 5; ++i) {
                            const size_t e = (size_t)row[j] * W + col[i];
                            const double xv = xi[e], yv = yi[e];
                            sx = sx + xv; sy = sy + yv; sxx = sxx + xv * xv; syy = syy + yv * yv; sxy = sxy + xv * yv;
                        }
                    const double mx = sx / 25.0, my = sy / 25.0;
                    const double vx = sxx / 25.0 - mx * mx, vy = syy / 25.0 - my * my, vxy = sxy / 25.0 - mx * my;
                    const double n1 = 2.0 * mx * my + kC1, n2 = 2.0 * vxy + kC2;
                    const double d1 = mx * mx + my * my + kC1, d2 = vx + vy + kC2;
                    const double n = n1 * n2, dd = d1 * d2;
                    const double r = n / dd;
                    const double raw = (1.0 - r) / 2.0;
                    acc = acc + fmin(fmax(raw, 0.0), 1.0) + (raw != raw ? raw : 0.0);               // clamp keeps a NaN
                    const bool open = raw >= 0.0 && raw <= 1.0;                                     // torch's clamp backward: inclusive
                    cc[c] = open ? (float)(-(mx * (n2 - n1) - r * my * (d2 - d1)) / dd) : 0.0f;     // A
                    cc[3 + c] = open ? (float)(-(my * (n2 - n1) - r * mx * (d2 - d1)) / dd) : 0.0f; // A'
                    cc[6 + c] = open ? (float)(r * d1 / dd) : 0.0f;                                 // B = B'
                    cc[9 + c] = open ? (float)(-n1 / dd) : 0.0f;                                    // C
                }
                s = acc / 3.0;
            } else {
                s = 1000.0;
#pragma unroll
                for (int k = 0; k < 12; ++k) cc[k] = 0.0f;
            }
            if (v == 0 || s < best || (s != s && best == best)) {       // the lowest index attaining the minimum; a NaN wins (torch.min)
                best = s;
                w = v;
#pragma unroll
                for (int k = 0; k < 12; ++k) bc[k] = cc[k];
            }
        }
        const bool none = best >= 1000.0 || !a.mask[p];
        if (none) w = -1;
        lossv = none ? 0.0 : best;
        a.loss_map[p] = (float)lossv;
        a.winner[p] = (int8_t)w;
#pragma unroll
        for (int k = 0; k < 12; ++k) a.coef[(size_t)k * hw + p] = none ? 0.0f : bc[k];
    }
    const double t = wg_reduce<kNW>(lossv, s_red, Sum());
    if (threadIdx.x == 0) a.partial[blockIdx.x] = t;
}

// the partial sums in a fixed order: thread t takes t, t + 256, ...; then the tree and the fold of reduce.h
__global__ __launch_bounds__(kBlock) void vw_fold_kernel(const double* __restrict__ partial, int n, double denom, float* __restrict__ out) {
    __shared__ double s_red[kNW];
    double t = 0.0;
    for (int k = threadIdx.x; k < n; k += kBlock) t = t + partial[k];
    t = wg_reduce<kNW>(t, s_red, Sum());
    if (threadIdx.x == 0) out[0] = (float)(t / denom);
}

// how many positions of the padded 5-window centred at p reflect onto q (|p - q| <= 2, 0 <= p < n)
__device__ __forceinline__ int fold_count(int p, int q, int n) {
    int k = 1;                                                       // q itself: |p - q| <= 2 by construction
    if (q >= 1 && q <= 2 && p + q <= 2) ++k;                         // the padded position -q
    if (q >= n - 3 && q <= n - 2 && 2 * (n - 1) - q - p <= 2) ++k;   // the padded position 2 (n - 1) - q
    return k;
}

__global__ __launch_bounds__(kBlock) void vw_backward_kernel(WarpArgs a) {
    int qx, qy;
    if (!tile_pixel(a, qx, qy)) return;
    const int H = a.H, W = a.W;
    const size_t hw = (size_t)H * W, q = (size_t)qy * W + qx;
    const int x0 = max(qx - 2, 0), x1 = min(qx + 2, W - 1), y0 = max(qy - 2, 0), y1 = min(qy + 2, H - 1);
    double xq[3], gx[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int c = 0; c < 3; ++c) xq[c] = a.img[(size_t)c * hw + q];
    double gd = 0.0;
    for (int v = 0; v < a.nv; ++v) {
        double yq[3], gy[3] = {0.0, 0.0, 0.0};
#pragma unroll
        for (int c = 0; c < 3; ++c) yq[c] = a.y[((size_t)v * 3 + c) * hw + q];
        for (int py = y0; py <= y1; ++py) {
            const int ky = fold_count(py, qy, H);
            for (int px = x0; px <= x1; ++px) {
                const size_t p = (size_t)py * W + px;
                if (a.winner[p] != v) continue;
                const double cnt = (double)(ky * fold_count(px, qx, W));
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const double A = a.coef[(size_t)c * hw + p], Ap = a.coef[(size_t)(3 + c) * hw + p];
                    const double B = a.coef[(size_t)(6 + c) * hw + p], C = a.coef[(size_t)(9 + c) * hw + p];
                    gy[c] = gy[c] + cnt * (A + B * yq[c] + C * xq[c]);
                    gx[c] = gx[c] + cnt * (Ap + B * xq[c] + C * yq[c]);
                }
            }
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) gd = gd + gy[c] * a.dyd[((size_t)v * 3 + c) * hw + q];
    }
    const double scale = (double)a.upstream[0] / ((double)hw * 75.0);
#pragma unroll
    for (int c = 0; c < 3; ++c) a.d_img[(size_t)c * hw + q] = (float)(gx[c] * scale);
    a.d_depth[q] = (float)(gd * scale);
}

// ---- the smoothness loss --------------------------------------------------------------------------------------------------------
struct SmoothArgs {
    int H, W, C, groups;
    const float* depth;
    const float* guide;
    const float* upstream;
    double* partial;            // (2, groups), fp64
    float* loss;
    float* d_depth;
};

// exp(-mean over C of |g[e] - g[e + step]|); 1 without a guide
__device__ __forceinline__ float edge_weight(const SmoothArgs& a, size_t hw, size_t e, size_t step) {
    if (a.C == 0) return 1.0f;
    float s = 0.0f;
    for (int c = 0; c < a.C; ++c) s = s + fabsf(a.guide[(size_t)c * hw + e] - a.guide[(size_t)c * hw + e + step]);
    if (a.C > 1) s = s / (float)a.C;
    return expf(-s);
}

__device__ __forceinline__ float sign_of(float v) { return (float)((v > 0.0f) - (v < 0.0f)); }

__global__ __launch_bounds__(kBlock) void vw_smooth_kernel(SmoothArgs a) {
    __shared__ double s_a[kNW], s_b[kNW];
    const size_t hw = (size_t)a.H * a.W, e = (size_t)blockIdx.x * kBlock + threadIdx.x;
    double tx = 0.0, ty = 0.0;
    if (e < hw) {
        const int i = (int)(e / a.W), j = (int)(e - (size_t)i * a.W);
        const float d = a.depth[e];
        if (j + 1 < a.W) tx = fabsf(d - a.depth[e + 1]) * edge_weight(a, hw, e, 1);
        if (i + 1 < a.H) ty = fabsf(d - a.depth[e + a.W]) * edge_weight(a, hw, e, (size_t)a.W);
    }
    wave_publish(tx, ty, s_a, s_b, Sum(), Sum());
    __syncthreads();
    if (threadIdx.x == 0) {
        a.partial[blockIdx.x] = wg_fold<kNW>(s_a, Sum());
        a.partial[(size_t)a.groups + blockIdx.x] = wg_fold<kNW>(s_b, Sum());
    }
}

__global__ __launch_bounds__(kBlock) void vw_smooth_fold_kernel(SmoothArgs a) {
    __shared__ double s_a[kNW], s_b[kNW];
    double tx = 0.0, ty = 0.0;
    for (int k = threadIdx.x; k < a.groups; k += kBlock) { tx = tx + a.partial[k]; ty = ty + a.partial[(size_t)a.groups + k]; }
    wave_publish(tx, ty, s_a, s_b, Sum(), Sum());
    __syncthreads();
    if (threadIdx.x == 0) {
        const double nx = (double)((int64_t)a.H * (a.W - 1)), ny = (double)((int64_t)(a.H - 1) * a.W);
        a.loss[0] = (float)(wg_fold<kNW>(s_a, Sum()) / nx + wg_fold<kNW>(s_b, Sum()) / ny);      // an empty mean is 0 / 0 = NaN, as torch's
    }
}

__global__ __launch_bounds__(kBlock) void vw_smooth_backward_kernel(SmoothArgs a) {
    const size_t hw = (size_t)a.H * a.W, e = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (e >= hw) return;
    const int i = (int)(e / a.W), j = (int)(e - (size_t)i * a.W);
    const float d = a.depth[e], up = a.upstream[0];
    float gx = 0.0f, gy = 0.0f;
    if (j + 1 < a.W) gx = gx + sign_of(d - a.depth[e + 1]) * edge_weight(a, hw, e, 1);
    if (j > 0) gx = gx - sign_of(a.depth[e - 1] - d) * edge_weight(a, hw, e - 1, 1);
    if (i + 1 < a.H) gy = gy + sign_of(d - a.depth[e + a.W]) * edge_weight(a, hw, e, (size_t)a.W);
    if (i > 0) gy = gy - sign_of(a.depth[e - a.W] - d) * edge_weight(a, hw, e - a.W, (size_t)a.W);
    float g = 0.0f;
    if (a.W > 1) g = g + gx * (up / (float)((int64_t)a.H * (a.W - 1)));
    if (a.H > 1) g = g + gy * (up / (float)((int64_t)(a.H - 1) * a.W));
    a.d_depth[e] = g;
}

int check_warp_sizes(const char* who, int32_t nv, int32_t H, int32_t W, WarpLayout* l) {
    if (nv < 1 || nv > SCG_VW_MAX_VIEWS) return g_err.fail(SCG_E_RANGE, "%s: nv = %d is outside 1..%d", who, nv, SCG_VW_MAX_VIEWS);
    if (H < SCG_VW_MIN_DIM || W < SCG_VW_MIN_DIM || H > SCG_VW_MAX_DIM || W > SCG_VW_MAX_DIM)
        return g_err.fail(SCG_E_RANGE, "%s: %d x %d pixels (H, W must be %d..%d: the 5x5 window reflects by 2)", who, W, H, SCG_VW_MIN_DIM,
                       SCG_VW_MAX_DIM);
    warp_layout(nv, H, W, l);
    return 0;
}

int check_smooth_sizes(const char* who, int32_t H, int32_t W, int32_t C) {
    if (H < 1 || W < 1 || H > SCG_VW_MAX_DIM || W > SCG_VW_MAX_DIM)
        return g_err.fail(SCG_E_RANGE, "%s: %d x %d pixels (H, W must be 1..%d)", who, W, H, SCG_VW_MAX_DIM);
    if (C < 0 || C > SCG_VW_MAX_GUIDE_CHANNELS) return g_err.fail(SCG_E_RANGE, "%s: C = %d is outside 0..%d", who, C, SCG_VW_MAX_GUIDE_CHANNELS);
    return 0;
}

int smooth_groups(int64_t H, int64_t W) { return (int)((H * W + kBlock - 1) / kBlock); }

}  // namespace
}  // namespace scg

using namespace scg;

extern "C" {

const char* scg_vw_last_error(void) { return g_err.text; }
int32_t scg_vw_abi_version(void) { return SCG_VW_ABI_VERSION; }

size_t scg_vw_warp_scratch_bytes(int32_t nv, int32_t H, int32_t W) {
    WarpLayout l;
    return warp_layout(nv, H, W, &l) ? l.total : 0;
}

int scg_vw_warp_forward(int32_t nv, int32_t H, int32_t W, const float* virtual_img, const float* virtual_depth, const uint8_t* vir_mask,
                        const float* img_colors, const float* records, float* loss, float* loss_map, int8_t* winner,
                        uint8_t* in_bounds, void* scratch, size_t scratch_bytes, void* stream) {
    const char* who = "scg_vw_warp_forward";
    WarpLayout l;
    if (int rc = check_warp_sizes(who, nv, H, W, &l)) return rc;
    if (int rc = g_err.check_ptr(who, virtual_img, "virtual_img", 4)) return rc;
    if (int rc = g_err.check_ptr(who, virtual_depth, "virtual_depth", 4)) return rc;
    if (int rc = g_err.check_ptr(who, vir_mask, "vir_mask", 1)) return rc;
    if (int rc = g_err.check_ptr(who, img_colors, "img_colors", 4)) return rc;
    if (int rc = g_err.check_ptr(who, records, "records", 4)) return rc;
    if (int rc = g_err.check_ptr(who, loss, "loss", 4)) return rc;
    if (int rc = g_err.check_ptr(who, loss_map, "loss_map", 4)) return rc;
    if (int rc = g_err.check_ptr(who, winner, "winner", 1)) return rc;
    if (int rc = g_err.check_ptr(who, in_bounds, "in_bounds", 1)) return rc;
    if (!scratch) return g_err.fail(SCG_E_NULL, "%s: scratch is NULL", who);
    if (scratch_bytes < l.total) return g_err.fail(SCG_E_SCRATCH, "%s: scratch of %zu bytes < %zu", who, scratch_bytes, l.total);
    if (reinterpret_cast<uintptr_t>(scratch) % 16) return g_err.fail(SCG_E_ALIGN, "%s: scratch is not 16-byte aligned", who);

    WarpArgs a = {};
    a.nv = nv; a.H = H; a.W = W; a.tiles_x = l.tiles_x; a.tiles = l.tiles_x * l.tiles_y;
    a.img = virtual_img; a.depth = virtual_depth; a.mask = vir_mask; a.colors = img_colors; a.records = records;
    a.loss = loss; a.loss_map = loss_map; a.winner = winner; a.in_bounds = in_bounds;
    char* s = static_cast<char*>(scratch);
    a.y = reinterpret_cast<double*>(s + l.y); a.dyd = reinterpret_cast<double*>(s + l.dyd);
    a.partial = reinterpret_cast<double*>(s + l.partial); a.coef = reinterpret_cast<float*>(s + l.coef);
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(vw_warp_kernel, dim3((unsigned)a.tiles, (unsigned)nv), dim3(kBlock), 0, st, a);
    if (int rc = g_err.check_hip(hipGetLastError(), "vw_warp")) return rc;
    hipLaunchKernelGGL(vw_ssim_kernel, dim3((unsigned)a.tiles), dim3(kBlock), 0, st, a);
    if (int rc = g_err.check_hip(hipGetLastError(), "vw_ssim")) return rc;
    hipLaunchKernelGGL(vw_fold_kernel, dim3(1), dim3(kBlock), 0, st, (const double*)a.partial, a.tiles, (double)l.hw, loss);
    return g_err.check_hip(hipGetLastError(), "vw_fold");
}

int scg_vw_warp_backward(int32_t nv, int32_t H, int32_t W, const float* virtual_img, const float* upstream, const int8_t* winner,
                         const void* scratch, size_t scratch_bytes, float* d_img, float* d_depth, void* stream) {
    const char* who = "scg_vw_warp_backward";
    WarpLayout l;
    if (int rc = check_warp_sizes(who, nv, H, W, &l)) return rc;
    if (int rc = g_err.check_ptr(who, virtual_img, "virtual_img", 4)) return rc;
    if (int rc = g_err.check_ptr(who, upstream, "upstream", 4)) return rc;
    if (int rc = g_err.check_ptr(who, winner, "winner", 1)) return rc;
    if (int rc = g_err.check_ptr(who, d_img, "d_img", 4)) return rc;
    if (int rc = g_err.check_ptr(who, d_depth, "d_depth", 4)) return rc;
    if (!scratch) return g_err.fail(SCG_E_NULL, "%s: scratch is NULL", who);
    if (scratch_bytes < l.total) return g_err.fail(SCG_E_SCRATCH, "%s: scratch of %zu bytes < %zu", who, scratch_bytes, l.total);
    if (reinterpret_cast<uintptr_t>(scratch) % 16) return g_err.fail(SCG_E_ALIGN, "%s: scratch is not 16-byte aligned", who);

    WarpArgs a = {};
    a.nv = nv; a.H = H; a.W = W; a.tiles_x = l.tiles_x; a.tiles = l.tiles_x * l.tiles_y;
    a.img = virtual_img; a.upstream = upstream; a.winner = const_cast<int8_t*>(winner);
    char* s = static_cast<char*>(const_cast<void*>(scratch));
    a.y = reinterpret_cast<double*>(s + l.y); a.dyd = reinterpret_cast<double*>(s + l.dyd);
    a.partial = reinterpret_cast<double*>(s + l.partial); a.coef = reinterpret_cast<float*>(s + l.coef);
    a.d_img = d_img; a.d_depth = d_depth;
    hipLaunchKernelGGL(vw_backward_kernel, dim3((unsigned)a.tiles), dim3(kBlock), 0, static_cast<hipStream_t>(stream), a);
    return g_err.check_hip(hipGetLastError(), "vw_backward");
}

size_t scg_vw_smooth_scratch_bytes(int32_t H, int32_t W) {
    if (H < 1 || W < 1 || H > SCG_VW_MAX_DIM || W > SCG_VW_MAX_DIM) return 0;
    return (size_t)smooth_groups(H, W) * 2 * sizeof(double);
}

int scg_vw_smooth_forward(int32_t H, int32_t W, int32_t C, const float* depth, const float* guide, float* loss, void* scratch,
                          size_t scratch_bytes, void* stream) {
    const char* who = "scg_vw_smooth_forward";
    if (int rc = check_smooth_sizes(who, H, W, C)) return rc;
    if (int rc = g_err.check_ptr(who, depth, "depth", 4)) return rc;
    if (C == 0 && guide) return g_err.fail(SCG_E_EXCLUSIVE, "%s: a guide with C = 0", who);
    if (C > 0) if (int rc = g_err.check_ptr(who, guide, "guide", 4)) return rc;
    if (int rc = g_err.check_ptr(who, loss, "loss", 4)) return rc;
    if (int rc = g_err.check_ptr(who, scratch, "scratch", 8)) return rc;
    const size_t need = scg_vw_smooth_scratch_bytes(H, W);
    if (scratch_bytes < need) return g_err.fail(SCG_E_SCRATCH, "%s: scratch of %zu bytes < %zu", who, scratch_bytes, need);
    SmoothArgs a = {};
    a.H = H; a.W = W; a.C = C; a.groups = smooth_groups(H, W);
    a.depth = depth; a.guide = guide; a.partial = static_cast<double*>(scratch); a.loss = loss;
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(vw_smooth_kernel, dim3((unsigned)a.groups), dim3(kBlock), 0, st, a);
    if (int rc = g_err.check_hip(hipGetLastError(), "vw_smooth")) return rc;
    hipLaunchKernelGGL(vw_smooth_fold_kernel, dim3(1), dim3(kBlock), 0, st, a);
    return g_err.check_hip(hipGetLastError(), "vw_smooth_fold");
}

int scg_vw_smooth_backward(int32_t H, int32_t W, int32_t C, const float* depth, const float* guide, const float* upstream,
                           float* d_depth, void* stream) {
    const char* who = "scg_vw_smooth_backward";
    if (int rc = check_smooth_sizes(who, H, W, C)) return rc;
    if (int rc = g_err.check_ptr(who, depth, "depth", 4)) return rc;
    if (C == 0 && guide) return g_err.fail(SCG_E_EXCLUSIVE, "%s: a guide with C = 0", who);
    if (C > 0) if (int rc = g_err.check_ptr(who, guide, "guide", 4)) return rc;
    if (int rc = g_err.check_ptr(who, upstream, "upstream", 4)) return rc;
    if (int rc = g_err.check_ptr(who, d_depth, "d_depth", 4)) return rc;
    SmoothArgs a = {};
    a.H = H; a.W = W; a.C = C; a.groups = smooth_groups(H, W);
    a.depth = depth; a.guide = guide; a.upstream = upstream; a.d_depth = d_depth;
    hipLaunchKernelGGL(vw_smooth_backward_kernel, dim3((unsigned)a.groups), dim3(kBlock), 0, static_cast<hipStream_t>(stream), a);
    return g_err.check_hip(hipGetLastError(), "vw_smooth_backward");
}

}  // extern "C"

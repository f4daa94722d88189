// lpips.hip — libscg_lp.so: the LPIPS metric with VGG16 features (include/lp/scg_lpips.h states the rule, the orders and the layouts).
//
//   lp_first_kernel   the first layer (cin = 3, K = 27) on the vector pipe: the z-score, the zero padding in the z domain, an fmaf
//                     chain in k order, bias, ReLU.  A thread is one pixel and sixteen output channels; weights in LDS.
//   lp_conv_kernel    every other layer as an implicit GEMM on v_mfma_f32_32x32x2_f32.  A workgroup of four waves (2 x 2) owns
//                     128 pixels x 64 NT channels; a wave 64 pixels x 32 NT channels = 2 x NT accumulator tiles.  Per chunk of
//                     32 k both operand tiles go global -> registers -> LDS ([row][32 + 4] floats: 16-byte stores, and
//                     ds_read_b128 without a bank conflict, MI355X LDS table), the next chunk's loads in flight behind the MFMAs.
//                     A chunk's 32 products are one MFMA chain from +0; the chunks' sums are added in chunk order on the vector
//                     pipe (a sum of 144 numbers of 32 products each carries a fifth of the error of one chain of 4608).
//                     A chunk lies inside one of the nine positions (cin is a multiple of 64), so a row's 32 k are contiguous in
//                     the channels-last activation, and in the [cout][9 cin] weights.  POOL: the loader takes the maximum of the
//                     four unpooled pixels instead.  Rows beyond M and positions outside the image load zeros.
//   lp_head_kernel    a wave per pixel, the channels over its lanes: both norms, the quotients, the weighted squared difference,
//                     the optional normalised maps; per workgroup one fp64 partial sum.  blockIdx.y is the tap.
//   lp_fold_kernel    one workgroup folds each tap's partial sums in a fixed order, divides, and sums the five means.
//
// No atomics, no allocation, no host read.  Every sum starts at +0 and every step is one fma or one add: a product with a zero
// operand leaves it as it is, so a pixel's value does not depend on its neighbours in the tile.
#include "../../include/lp/scg_lpips.h"
#include "host_error.h"
#include "reduce.h"

#pragma clang fp contract(off)

namespace scg {
namespace {

constexpr int kTM = SCG_LP_TILE_M;
constexpr int kBK = 32;                    // k per chunk
constexpr int kLd = kBK + 4;               // LDS row stride in floats
constexpr int kHeadPix = SCG_LP_HEAD_PIXELS;
constexpr int kNW = kBlock / kWave;
constexpr int kFirstPix = 64;              // pixels per workgroup of the first layer
constexpr int kSmallGrid = SCG_LP_SMALL_GRID;      // at most this many 128-channel workgroups: the layer runs with 64-channel ones
static_assert(kTM == 128 && kBlock == 256 && kHeadPix % kNW == 0, "the tiling below is written for these");

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kCin[SCG_LP_LAYERS] = {3, 64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512};
constexpr int kCout[SCG_LP_LAYERS] = {64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512, 512};
constexpr bool kPoolIn[SCG_LP_LAYERS] = {false, false, true, false, true, false, false, true, false, false, true, false, false};
constexpr int kTapC[SCG_LP_TAPS] = {64, 128, 256, 512, 512};

thread_local ErrorText g_err = {};

// torch's relu: a NaN stays, -0 and everything below become +0
__device__ __forceinline__ float relu_keep_nan(float v) { return (v > 0.f || v != v) ? v : 0.f; }

// ---- the first layer ---------------------------------------------------------------------------------------------------------
struct FirstArgs {
    int n, h, w, M;
    const float* img0;          // image 0; image i >= 1 is img1 when given, else img0 + i * image_stride
    const float* img1;
    size_t image_stride, pixel_stride, channel_stride;      // in floats
    const float* wt;            // [64][27]
    const float* bias;
    float* out;                 // (n, h, w, 64)
    int relu, zscore;
};

__global__ __launch_bounds__(kBlock) void lp_first_kernel(FirstArgs a) {
    __shared__ float s_w[27 * 64];          // [k][cout]
    __shared__ float s_b[64];
    for (int i = threadIdx.x; i < 27 * 64; i += kBlock) s_w[(i % 27) * 64 + i / 27] = a.wt[i];
    if (threadIdx.x < 64) s_b[threadIdx.x] = a.bias[threadIdx.x];
    __syncthreads();
    const int m = blockIdx.x * kFirstPix + (threadIdx.x >> 2);
    if (m >= a.M) return;
    const int cq = (threadIdx.x & 3) * 16;
    const int hw = a.h * a.w;
    const int img = m / hw, rem = m - img * hw, y = rem / a.w, x = rem - y * a.w;
    const float* __restrict__ src = (img >= 1 && a.img1) ? a.img1 : a.img0 + (size_t)img * a.image_stride;
    const float mean[3] = {-.030f, -.088f, -.188f}, sd[3] = {.458f, .448f, .450f};
    float v[27];
#pragma unroll
    for (int t = 0; t < 9; ++t) {
        const int yy = y + t / 3 - 1, xx = x + t % 3 - 1;
        const bool in = yy >= 0 && yy < a.h && xx >= 0 && xx < a.w;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float p = 0.f;
            if (in) {
                p = src[((size_t)yy * a.w + xx) * a.pixel_stride + (size_t)c * a.channel_stride];
                if (a.zscore) p = (p - mean[c]) / sd[c];
            }
            v[t * 3 + c] = p;
        }
    }
    float* __restrict__ o = a.out + (size_t)m * 64 + cq;
#pragma unroll
    for (int u4 = 0; u4 < 4; ++u4) {
        float r[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int co = cq + u4 * 4 + e;
            float s = 0.f;
#pragma unroll
            for (int k = 0; k < 27; ++k) s = fmaf(v[k], s_w[k * 64 + co], s);
            s = s + s_b[co];
            r[e] = a.relu ? relu_keep_nan(s) : s;
        }
        *reinterpret_cast<float4*>(o + u4 * 4) = make_float4(r[0], r[1], r[2], r[3]);
    }
}

// ---- the implicit GEMM -------------------------------------------------------------------------------------------------------
struct ConvArgs {
    int cin, cout, h, w;        // h, w: the convolution's own size (the pooled size under POOL)
    int hin, win;               // the input tensor's size
    int M;                      // n * h * w
    const float* in;
    const float* wt;            // [cout][9 cin]
    const float* bias;
    float* out;                 // (n, h, w, cout)
    int relu;
};

// torch's max pool: a NaN on either side wins (branch-free)
__device__ __forceinline__ float pool_max(float a, float b) { return (a == a && b == b) ? fmaxf(a, b) : __builtin_nanf(""); }
__device__ __forceinline__ f32x4 max4(f32x4 a, f32x4 b) {
    f32x4 r;
#pragma unroll
    for (int e = 0; e < 4; ++e) r[e] = pool_max(a[e], b[e]);
    return r;
}

template <int NT, bool POOL>
__global__ __launch_bounds__(kBlock) void lp_conv_kernel(ConvArgs a) {
    constexpr int TN = 64 * NT;
    __shared__ __attribute__((aligned(16))) float s_a[kTM * kLd];
    __shared__ __attribute__((aligned(16))) float s_b[TN * kLd];
    const int nb = a.cout / TN;
    const int nt = blockIdx.x % nb, mt = blockIdx.x / nb;       // the channel tiles of one pixel tile run next to each other
    const int m0 = mt * kTM, n0 = nt * TN;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int kq = (tid & 7) * 4, lr = tid >> 3;                // the loader's k offset inside a chunk and its first row
    const int K = 9 * a.cin, nchunks = K / kBK;
    const int hw = a.h * a.w;

    int py[4], px[4], pimg[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int m = m0 + lr + 32 * j;
        const int img = m / hw, rem = m - img * hw;
        pimg[j] = img;
        py[j] = m < a.M ? rem / a.w : -4;                       // a row beyond M: every position is outside
        px[j] = rem - (rem / a.w) * a.w;
    }

    f32x4 ra[4], rb[2 * NT];

    const f32x16 kZero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    f32x16 acc[2][NT];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int t = 0; t < NT; ++t) acc[i][t] = kZero16;

    const int frag = (lane & 31) * kLd + (lane >> 5) * 4;
    const float* fa0 = s_a + (wm * 64) * kLd + frag;
    const float* fb0 = s_b + (wn * 32 * NT) * kLd + frag;

    for (int chunk = -1; chunk < nchunks; ++chunk) {           // trip -1 only loads
        if (chunk >= 0) {
            __syncthreads();                                    // the previous chunk's reads are done
#pragma unroll
            for (int j = 0; j < 4; ++j) *reinterpret_cast<f32x4*>(s_a + (lr + 32 * j) * kLd + kq) = ra[j];
#pragma unroll
            for (int j = 0; j < 2 * NT; ++j) *reinterpret_cast<f32x4*>(s_b + (lr + 32 * j) * kLd + kq) = rb[j];
            __syncthreads();
        }
        if (chunk + 1 < nchunks) {                              // the next chunk's loads, in flight behind the MFMAs
            const int k0 = (chunk + 1) * kBK, pos = k0 / a.cin, c0 = k0 - pos * a.cin + kq;
            const int dy = pos / 3 - 1, dx = pos % 3 - 1;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int yy = py[j] + dy, xx = px[j] + dx;
                f32x4 v = {0.f, 0.f, 0.f, 0.f};
                if (yy >= 0 && yy < a.h && xx >= 0 && xx < a.w) {
                    if (POOL) {
                        const float* p = a.in + (((size_t)pimg[j] * a.hin + 2 * yy) * a.win + 2 * xx) * a.cin + c0;
                        const size_t row = (size_t)a.win * a.cin;
                        v = max4(max4(*reinterpret_cast<const f32x4*>(p), *reinterpret_cast<const f32x4*>(p + a.cin)),
                                 max4(*reinterpret_cast<const f32x4*>(p + row), *reinterpret_cast<const f32x4*>(p + row + a.cin)));
                    } else {
                        v = *reinterpret_cast<const f32x4*>(a.in + (((size_t)pimg[j] * a.h + yy) * a.w + xx) * a.cin + c0);
                    }
                }
                ra[j] = v;
            }
#pragma unroll
            for (int j = 0; j < 2 * NT; ++j)
                rb[j] = *reinterpret_cast<const f32x4*>(a.wt + (size_t)(n0 + lr + 32 * j) * K + k0 + kq);
        }
        if (chunk < 0) continue;
        f32x16 part[2][NT];                                     // this chunk's sums: one fma chain each, from +0
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            f32x4 fa[2], fb[NT];
#pragma unroll
            for (int i = 0; i < 2; ++i) fa[i] = *reinterpret_cast<const f32x4*>(fa0 + i * 32 * kLd + q * 8);
#pragma unroll
            for (int t = 0; t < NT; ++t) fb[t] = *reinterpret_cast<const f32x4*>(fb0 + t * 32 * kLd + q * 8);
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int t = 0; t < NT; ++t)
#pragma unroll
                    for (int i = 0; i < 2; ++i)
                        part[i][t] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[i][j], fb[t][j], (q | j) ? part[i][t] : kZero16, 0, 0, 0);
        }
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int t = 0; t < NT; ++t) acc[i][t] = acc[i][t] + part[i][t];      // the chunks' sums, added in chunk order
    }

    // D: column = lane & 31 (the channel), row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5) (the pixel)
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int co = n0 + wn * 32 * NT + t * 32 + (lane & 31);
        const float b = a.bias[co];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = m0 + wm * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                if (m < a.M) {
                    const float s = acc[i][t][r] + b;
                    a.out[(size_t)m * a.cout + co] = a.relu ? relu_keep_nan(s) : s;
                }
            }
    }
}

int launch_first(const FirstArgs& a, hipStream_t st) {
    hipLaunchKernelGGL(lp_first_kernel, dim3((unsigned)((a.M + kFirstPix - 1) / kFirstPix)), dim3(kBlock), 0, st, a);
    return g_err.check_hip(hipGetLastError(), "lp_first");
}

// n images of (hin, win, cin), pooled first when `pool`
int launch_conv(int n, int cin, int cout, int hin, int win, bool pool, const float* in, const float* wt, const float* bias,
                float* out, bool relu, hipStream_t st) {
    ConvArgs a = {};
    a.cin = cin; a.cout = cout; a.hin = hin; a.win = win;
    a.h = pool ? hin / 2 : hin; a.w = pool ? win / 2 : win;
    a.M = n * a.h * a.w;
    a.in = in; a.wt = wt; a.bias = bias; a.out = out; a.relu = relu ? 1 : 0;
    const int mtiles = (a.M + kTM - 1) / kTM;
    // 64-channel tiles where 128-channel ones would leave most compute units without a workgroup: twice the workgroups of half
    // the work.  Which tile computes an output element does not enter its sum: the bits are the same either way.
    if (cout == 64 || mtiles * (cout / 128) <= kSmallGrid) {
        const dim3 grid((unsigned)mtiles * (unsigned)(cout / 64));
        if (pool) hipLaunchKernelGGL((lp_conv_kernel<1, true>), grid, dim3(kBlock), 0, st, a);
        else hipLaunchKernelGGL((lp_conv_kernel<1, false>), grid, dim3(kBlock), 0, st, a);
    } else {
        const dim3 grid((unsigned)mtiles * (unsigned)(cout / 128));
        if (pool) hipLaunchKernelGGL((lp_conv_kernel<2, true>), grid, dim3(kBlock), 0, st, a);
        else hipLaunchKernelGGL((lp_conv_kernel<2, false>), grid, dim3(kBlock), 0, st, a);
    }
    return g_err.check_hip(hipGetLastError(), "lp_conv");
}

// ---- the head ----------------------------------------------------------------------------------------------------------------
struct HeadArgs {
    const float* tap[SCG_LP_TAPS];          // (2, P, C)
    const float* lin[SCG_LP_TAPS];
    float* feat[SCG_LP_TAPS];               // (2, P, C) or nullptr
    int C[SCG_LP_TAPS], P[SCG_LP_TAPS];
    double* partial;                        // [tap][pb]
    int pb;
    float* value;
    float* terms;
};

__global__ __launch_bounds__(kBlock) void lp_head_kernel(HeadArgs a) {
    __shared__ double s_red[kNW];
    const int t = blockIdx.y, P = a.P[t], C = a.C[t];
    const int first = blockIdx.x * kHeadPix;
    if (first >= P) return;
    const float* __restrict__ fx = a.tap[t];
    const float* __restrict__ fy = fx + (size_t)P * C;
    const float* __restrict__ lin = a.lin[t];
    float* ox = a.feat[t];
    float* oy = ox ? ox + (size_t)P * C : nullptr;
    const int lane = lane_id();
    double wsum = 0.0;
    for (int i = 0; i < kHeadPix / kNW; ++i) {
        const int p = first + wave_id() * (kHeadPix / kNW) + i;
        if (p >= P) break;                                   // the same for the whole wave
        float xv[8], yv[8];
        double sx = 0.0, sy = 0.0;
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            xv[u] = yv[u] = 0.f;
            if (u * 64 < C) {
                xv[u] = fx[(size_t)p * C + u * 64 + lane];
                yv[u] = fy[(size_t)p * C + u * 64 + lane];
                sx = sx + (double)xv[u] * (double)xv[u];
                sy = sy + (double)yv[u] * (double)yv[u];
            }
        }
        sx = __shfl(wave_reduce(sx, Sum()), 0, kWave);
        sy = __shfl(wave_reduce(sy, Sum()), 0, kWave);
        const double dx = sqrt(sx) + 1e-10, dy = sqrt(sy) + 1e-10;
        double d = 0.0;
#pragma unroll
        for (int u = 0; u < 8; ++u)
            if (u * 64 < C) {
                const double nx = (double)xv[u] / dx, ny = (double)yv[u] / dy, df = nx - ny;
                d = d + (double)lin[u * 64 + lane] * (df * df);
                if (ox) {
                    ox[(size_t)p * C + u * 64 + lane] = (float)nx;
                    oy[(size_t)p * C + u * 64 + lane] = (float)ny;
                }
            }
        wsum = wsum + wave_reduce(d, Sum());                 // lane 0's is the wave's
    }
    if (lane == 0) s_red[wave_id()] = wsum;                  // a wave without a pixel leaves 0
    __syncthreads();
    if (threadIdx.x == 0) a.partial[(size_t)t * a.pb + blockIdx.x] = wg_fold<kNW>(s_red, Sum());
}

__global__ __launch_bounds__(kBlock) void lp_fold_kernel(HeadArgs a) {
    __shared__ double s_red[kNW];
    double total = 0.0;
    for (int t = 0; t < SCG_LP_TAPS; ++t) {
        const int nblk = (a.P[t] + kHeadPix - 1) / kHeadPix;
        double s = 0.0;
        for (int i = threadIdx.x; i < nblk; i += kBlock) s = s + a.partial[(size_t)t * a.pb + i];
        s = wg_reduce<kNW>(s, s_red, Sum());
        const double mean = s / (double)a.P[t];
        if (threadIdx.x == 0) a.terms[t] = (float)mean;
        total = total + mean;
    }
    if (threadIdx.x == 0) a.value[0] = (float)total;
}

struct Layout {
    int h[SCG_LP_TAPS], w[SCG_LP_TAPS];
    size_t tap[SCG_LP_TAPS], A, B, partial, total;      // offsets in BYTES
    size_t feat[SCG_LP_TAPS], feat_floats;              // offsets in floats
    int pb;
};

bool layout(int64_t H, int64_t W, Layout* l) {
    if (H < SCG_LP_MIN_DIM || W < SCG_LP_MIN_DIM || H > SCG_LP_MAX_DIM || W > SCG_LP_MAX_DIM || H * W > SCG_LP_MAX_PIXELS) return false;
    size_t P[SCG_LP_TAPS];
    for (int t = 0; t < SCG_LP_TAPS; ++t) {
        l->h[t] = t ? l->h[t - 1] / 2 : (int)H;
        l->w[t] = t ? l->w[t - 1] / 2 : (int)W;
        P[t] = (size_t)l->h[t] * l->w[t];
    }
    size_t off = 0, f = 0;
    auto take = [&](size_t floats) { const size_t at = off; off += floats * sizeof(float); return at; };
    l->tap[0] = take(2 * P[0] * 64);
    l->A = take(2 * P[0] * 64);
    l->tap[1] = take(2 * P[1] * 128);
    l->tap[2] = take(2 * P[2] * 256);
    l->B = take(2 * P[2] * 256);
    l->tap[3] = take(2 * P[3] * 512);
    l->tap[4] = take(2 * P[4] * 512);
    l->pb = (int)((P[0] + kHeadPix - 1) / kHeadPix);
    l->partial = off;
    l->total = off + (size_t)SCG_LP_TAPS * l->pb * sizeof(double);
    for (int t = 0; t < SCG_LP_TAPS; ++t) { l->feat[t] = f; f += 2 * P[t] * kTapC[t]; }
    l->feat_floats = f;
    return true;
}


// the head and the fold on the taps in scratch
int launch_head(const Layout& l, char* s, const float* params, float* value, float* terms, float* features, hipStream_t st) {
    size_t off = 0;
    for (int i = 0; i < SCG_LP_LAYERS; ++i) off += (size_t)9 * kCin[i] * kCout[i] + kCout[i];
    HeadArgs a = {};
    for (int t = 0; t < SCG_LP_TAPS; ++t) {
        a.tap[t] = reinterpret_cast<const float*>(s + l.tap[t]);
        a.lin[t] = params + off;
        off += kTapC[t];
        a.feat[t] = features ? features + l.feat[t] : nullptr;
        a.C[t] = kTapC[t];
        a.P[t] = l.h[t] * l.w[t];
    }
    a.partial = reinterpret_cast<double*>(s + l.partial); a.pb = l.pb; a.value = value; a.terms = terms;
    hipLaunchKernelGGL(lp_head_kernel, dim3((unsigned)l.pb, SCG_LP_TAPS), dim3(kBlock), 0, st, a);
    if (int rc = g_err.check_hip(hipGetLastError(), "lp_head")) return rc;
    hipLaunchKernelGGL(lp_fold_kernel, dim3(1), dim3(kBlock), 0, st, a);
    return g_err.check_hip(hipGetLastError(), "lp_fold");
}

}  // namespace
}  // namespace scg

using namespace scg;

extern "C" {

const char* scg_lp_last_error(void) { return g_err.text; }
int32_t scg_lp_abi_version(void) { return SCG_LP_ABI_VERSION; }

size_t scg_lp_scratch_bytes(int32_t H, int32_t W) {
    Layout l;
    return layout(H, W, &l) ? l.total : 0;
}

size_t scg_lp_feature_floats(int32_t H, int32_t W) {
    Layout l;
    return layout(H, W, &l) ? l.feat_floats : 0;
}

int scg_lp_conv3x3(int32_t n, int32_t cin, int32_t cout, int32_t h, int32_t w, const float* in, const float* weights,
                   const float* bias, float* out, int32_t flags, void* stream) {
    const char* who = "scg_lp_conv3x3";
    bool pair = false;
    for (int l = 0; l < SCG_LP_LAYERS; ++l) pair |= (cin == kCin[l] && cout == kCout[l]);
    if (!pair) return g_err.fail(SCG_E_RANGE, "%s: (cin, cout) = (%d, %d) is not a layer of the network", who, cin, cout);
    if (flags & ~(SCG_LP_RELU | SCG_LP_POOL | SCG_LP_ZSCORE)) return g_err.fail(SCG_E_RANGE, "%s: unknown flags %d", who, flags);
    const bool pool = flags & SCG_LP_POOL, zs = flags & SCG_LP_ZSCORE;
    if (cin == 3 ? pool : zs)
        return g_err.fail(SCG_E_EXCLUSIVE, "%s: the z-score belongs to cin = 3, the pool to cin >= 64", who);
    const int lo = pool ? 2 : 1;
    if (n < 1 || n > SCG_LP_MAX_BATCH || h < lo || w < lo || h > SCG_LP_MAX_DIM || w > SCG_LP_MAX_DIM ||
        (int64_t)h * w > SCG_LP_MAX_PIXELS)
        return g_err.fail(SCG_E_RANGE, "%s: n = %d, h = %d, w = %d out of range", who, n, h, w);
    if (int rc = g_err.check_ptr(who, in, "in", 16)) return rc;
    if (int rc = g_err.check_ptr(who, weights, "weights", 16)) return rc;
    if (int rc = g_err.check_ptr(who, bias, "bias", 16)) return rc;
    if (int rc = g_err.check_ptr(who, out, "out", 16)) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (cin == 3) {
        FirstArgs a = {};
        a.n = n; a.h = h; a.w = w; a.M = n * h * w;
        a.img0 = in; a.img1 = nullptr; a.image_stride = (size_t)h * w * 3; a.pixel_stride = 3; a.channel_stride = 1;
        a.wt = weights; a.bias = bias; a.out = out; a.relu = (flags & SCG_LP_RELU) ? 1 : 0; a.zscore = zs ? 1 : 0;
        return launch_first(a, st);
    }
    return launch_conv(n, cin, cout, h, w, pool, in, weights, bias, out, flags & SCG_LP_RELU, st);
}

int scg_lp_forward(int32_t H, int32_t W, const float* x, const float* y, const float* params, float* value, float* terms,
                   float* features, void* scratch, size_t scratch_bytes, void* stream) {
    const char* who = "scg_lp_forward";
    Layout l;
    if (!layout(H, W, &l))
        return g_err.fail(SCG_E_RANGE, "%s: H = %d, W = %d: both must be in [%d, %d] and H * W <= %d", who, H, W, SCG_LP_MIN_DIM,
                       SCG_LP_MAX_DIM, SCG_LP_MAX_PIXELS);
    if (int rc = g_err.check_ptr(who, x, "x", 4)) return rc;
    if (int rc = g_err.check_ptr(who, y, "y", 4)) return rc;
    if (int rc = g_err.check_ptr(who, params, "params", 16)) return rc;
    if (int rc = g_err.check_ptr(who, value, "value", 4)) return rc;
    if (int rc = g_err.check_ptr(who, terms, "terms", 4)) return rc;
    if (features) if (int rc = g_err.check_ptr(who, features, "features", 16)) return rc;
    if (!scratch) return g_err.fail(SCG_E_NULL, "%s: scratch is NULL", who);
    if (scratch_bytes < l.total) return g_err.fail(SCG_E_SCRATCH, "%s: scratch of %zu bytes < %zu", who, scratch_bytes, l.total);
    if (reinterpret_cast<uintptr_t>(scratch) % 16) return g_err.fail(SCG_E_ALIGN, "%s: scratch is not 16-byte aligned", who);

    hipStream_t st = static_cast<hipStream_t>(stream);
    char* s = static_cast<char*>(scratch);
    float* tap[SCG_LP_TAPS];
    for (int t = 0; t < SCG_LP_TAPS; ++t) tap[t] = reinterpret_cast<float*>(s + l.tap[t]);
    float* A = reinterpret_cast<float*>(s + l.A);
    float* B = reinterpret_cast<float*>(s + l.B);
    const float* wt[SCG_LP_LAYERS];
    const float* bias[SCG_LP_LAYERS];
    size_t off = 0;
    for (int i = 0; i < SCG_LP_LAYERS; ++i) { wt[i] = params + off; off += (size_t)9 * kCin[i] * kCout[i]; }
    for (int i = 0; i < SCG_LP_LAYERS; ++i) { bias[i] = params + off; off += kCout[i]; }
    // where each layer reads and writes: the taps are kept, A and B carry the layers between them
    float* const dst[SCG_LP_LAYERS] = {A, tap[0], A, tap[1], A, B, tap[2], A, B, tap[3], A, B, tap[4]};
    const int level[SCG_LP_LAYERS] = {0, 0, 1, 1, 2, 2, 2, 3, 3, 3, 4, 4, 4};      // the resolution a layer works at

    FirstArgs f = {};
    f.n = 2; f.h = H; f.w = W; f.M = 2 * H * W;
    f.img0 = x; f.img1 = y; f.image_stride = 0; f.pixel_stride = 1; f.channel_stride = (size_t)H * W;
    f.wt = wt[0]; f.bias = bias[0]; f.out = dst[0]; f.relu = 1; f.zscore = 1;
    if (int rc = launch_first(f, st)) return rc;
    for (int i = 1; i < SCG_LP_LAYERS; ++i) {
        const int src = kPoolIn[i] ? level[i] - 1 : level[i];
        if (int rc = launch_conv(2, kCin[i], kCout[i], l.h[src], l.w[src], kPoolIn[i], dst[i - 1], wt[i], bias[i], dst[i], true, st))
            return rc;
    }
    return launch_head(l, s, params, value, terms, features, st);
}

int scg_lp_head(int32_t H, int32_t W, const float* params, float* value, float* terms, float* features, void* scratch,
                size_t scratch_bytes, void* stream) {
    const char* who = "scg_lp_head";
    Layout l;
    if (!layout(H, W, &l))
        return g_err.fail(SCG_E_RANGE, "%s: H = %d, W = %d: both must be in [%d, %d] and H * W <= %d", who, H, W, SCG_LP_MIN_DIM,
                       SCG_LP_MAX_DIM, SCG_LP_MAX_PIXELS);
    if (int rc = g_err.check_ptr(who, params, "params", 16)) return rc;
    if (int rc = g_err.check_ptr(who, value, "value", 4)) return rc;
    if (int rc = g_err.check_ptr(who, terms, "terms", 4)) return rc;
    if (features) if (int rc = g_err.check_ptr(who, features, "features", 16)) return rc;
    if (!scratch) return g_err.fail(SCG_E_NULL, "%s: scratch is NULL", who);
    if (scratch_bytes < l.total) return g_err.fail(SCG_E_SCRATCH, "%s: scratch of %zu bytes < %zu", who, scratch_bytes, l.total);
    if (reinterpret_cast<uintptr_t>(scratch) % 16) return g_err.fail(SCG_E_ALIGN, "%s: scratch is not 16-byte aligned", who);
    return launch_head(l, static_cast<char*>(scratch), params, value, terms, features, static_cast<hipStream_t>(stream));
}

}  // extern "C"

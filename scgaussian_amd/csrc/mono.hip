// mono.hip — the reference's scene setup, GaussianModel.create_from_mono (include/scg_mono.h).
//
//   scene/gaussian_model.py:293-310   per view: image / 255, mask, intr, w2c                        -> mono_images_kernel (+ host)
//   scene/gaussian_model.py:318-339   per ordered pair: uv, two grid_samples, the rays, the depths  -> mono_matches_kernel
//   init_stage.py from_view_gs        per ordered pair: partner uv, valid, count, weights           -> mono_pairs_kernel
//
// The rule decides a match from that match and its view's constants alone, so the match kernel is one thread per element of the
// arena.  A workgroup serves one segment (ScgMonoGroup), so the segment's and the view's records have one address for all its
// threads (blockIdx.x only) and are fetched with scalar loads, as in geocheck.hip; what a thread itself loads is its match pixel,
// its uniform number and the taps.  The one thing that crosses matches is a pair's count: one workgroup per segment reduces it in a
// fixed order (reduce.h).  No atomics.
//
// Every index and offset read from a table is checked against the sizes of ScgMono before it addresses anything: a record that
// points outside is skipped.
//
// Compiled with -ffp-contract=off: tests/mono_refs.py restates the arithmetic below operation by operation (the sampler in fp32,
// the ray chain in fp64); a fused multiply-add would round differently.
#include <math.h>

#include "scg_common.h"
#include "reduce.h"
#include "../../include/scg_mono.h"

namespace scg {

constexpr int kMonoImageTrips = 4;               // elements per thread of the image kernel, kBlock apart
static_assert(sizeof(ScgMonoView) == 272, "two offsets, H, W, near, far and 30 doubles");
static_assert(sizeof(ScgMonoSegment) == 16 && sizeof(ScgMonoGroup) == 8, "table records");

// the view's pixel range lies inside the image arena (and its mask inside the mask arena)
__device__ __forceinline__ bool view_ok(const ScgMonoView& v, int64_t image_pixels, int64_t mask_pixels) {
    if (v.H < 1 || v.W < 1) return false;
    const int64_t n = (int64_t)v.H * v.W;
    if (v.image_off < 0 || v.image_off > image_pixels - n) return false;
    if (v.mask_off != -1 && (v.mask_off < 0 || v.mask_off > mask_pixels - n)) return false;
    return true;
}

__device__ __forceinline__ bool segment_ok(const ScgMonoSegment& s, int N, int V) {
    return s.count >= 0 && s.offset >= 0 && s.offset <= N - s.count && (unsigned)s.view < (unsigned)V;
}

__global__ __launch_bounds__(kBlock) void mono_images_kernel(const uint8_t* __restrict__ bytes, const ScgMonoView* __restrict__ views,
                                                             int64_t image_pixels, float* __restrict__ out) {
    const ScgMonoView& v = views[blockIdx.y];
    if (!view_ok(v, image_pixels, INT64_MAX)) return;
    const int64_t n = (int64_t)v.H * v.W * 3, base = v.image_off * 3;
    const int64_t first = (int64_t)blockIdx.x * (kBlock * kMonoImageTrips) + threadIdx.x;
#pragma unroll
    for (int k = 0; k < kMonoImageTrips; ++k) {
        const int64_t e = first + (int64_t)k * kBlock;
        if (e < n) out[base + e] = __fdiv_rn((float)bytes[base + e], 255.0f);
    }
}

// torch's grid_sample at one normalised coordinate pair: the weights and the four taps' coordinates.  false: samples nothing.
struct Taps { int x0, y0; float nw, ne, sw, se; };

__device__ __forceinline__ bool mono_taps(float gx, float gy, int H, int W, Taps& t) {
    const float ix = ((gx + 1.0f) * (float)W - 1.0f) / 2.0f;
    const float iy = ((gy + 1.0f) * (float)H - 1.0f) / 2.0f;
    if (ix != ix || iy != iy) return false;
    const float xf = floorf(ix), yf = floorf(iy);
    // a floor beyond int32 is outside every image: decided on the float, the cast would be undefined
    if (!(fabsf(xf) < 2147483648.0f && fabsf(yf) < 2147483648.0f)) return false;
    const float x1 = xf + 1.0f, y1 = yf + 1.0f;
    t.x0 = (int)xf;
    t.y0 = (int)yf;
    t.nw = (x1 - ix) * (y1 - iy);
    t.ne = (ix - xf) * (y1 - iy);
    t.sw = (x1 - ix) * (iy - yf);
    t.se = (ix - xf) * (iy - yf);
    return true;
}

__global__ __launch_bounds__(kBlock) void mono_matches_kernel(ScgMono a) {
    const ScgMonoGroup grp = a.groups[blockIdx.x];
    if ((unsigned)grp.segment >= (unsigned)a.nseg) return;
    const ScgMonoSegment seg = a.segments[grp.segment];
    if (!segment_ok(seg, a.N, a.V) || grp.first < 0) return;
    const ScgMonoView& v = a.views[seg.view];
    if (!view_ok(v, a.image_pixels, a.mask_pixels)) return;
    const int64_t k = (int64_t)grp.first + threadIdx.x;
    if (k >= seg.count) return;
    const size_t e = (size_t)seg.offset + (size_t)k;
    const int H = v.H, W = v.W;

    const float mx = a.match_pixel[2 * e], my = a.match_pixel[2 * e + 1];
    const float ux = mx * (float)W, uy = my * (float)H;
    a.uv[2 * e] = ux;
    a.uv[2 * e + 1] = uy;

    // ---- the two grid_samples ------------------------------------------------------------------------------------------------
    const float gx = mx * 2.0f - 1.0f, gy = my * 2.0f - 1.0f;
    float c0 = 0.0f, c1 = 0.0f, c2 = 0.0f, bm = 0.0f;
    Taps t;
    if (mono_taps(gx, gy, H, W, t)) {
        const float* __restrict__ img = a.image_color + v.image_off * 3;
        const float* __restrict__ msk = v.mask_off >= 0 ? a.masks + v.mask_off : nullptr;
#pragma unroll
        for (int q = 0; q < 4; ++q) {              // nw, ne, sw, se
            const int64_t x = (int64_t)t.x0 + (q & 1), y = (int64_t)t.y0 + (q >> 1);
            const float w = q == 0 ? t.nw : (q == 1 ? t.ne : (q == 2 ? t.sw : t.se));
            if (x >= 0 && x < W && y >= 0 && y < H) {
                const size_t p = (size_t)y * W + (size_t)x;
                c0 = c0 + img[3 * p] * w;
                c1 = c1 + img[3 * p + 1] * w;
                c2 = c2 + img[3 * p + 2] * w;
                bm = bm + (msk ? msk[p] : 1.0f) * w;
            }
        }
    }
    a.color[3 * e] = c0;
    a.color[3 * e + 1] = c1;
    a.color[3 * e + 2] = c2;
    a.blender_mask[e] = bm;

    // ---- the rays, fp64 ------------------------------------------------------------------------------------------------------
    const double u = (double)ux, w = (double)uy;
    const double px = v.Kinv[0] * u + v.Kinv[1] * w + v.Kinv[2];
    const double py = v.Kinv[3] * u + v.Kinv[4] * w + v.Kinv[5];
    const double pz = v.Kinv[6] * u + v.Kinv[7] * w + v.Kinv[8];
    const double nrm = sqrt(px * px + py * py + pz * pz) + 1e-8;
    const double dx = px / nrm, dy = py / nrm, dz = pz / nrm;
    const double rx = v.Rc2w[0] * dx + v.Rc2w[1] * dy + v.Rc2w[2] * dz;
    const double ry = v.Rc2w[3] * dx + v.Rc2w[4] * dy + v.Rc2w[5] * dz;
    const double rz = v.Rc2w[6] * dx + v.Rc2w[7] * dy + v.Rc2w[8] * dz;
    const double qx = v.Rw2c[0] * rx + v.Rw2c[1] * ry + v.Rw2c[2] * rz;
    const double qy = v.Rw2c[3] * rx + v.Rw2c[4] * ry + v.Rw2c[5] * rz;
    const double qz = v.Rw2c[6] * rx + v.Rw2c[7] * ry + v.Rw2c[8] * rz;
    a.rays_o[3 * e] = (float)v.origin[0];
    a.rays_o[3 * e + 1] = (float)v.origin[1];
    a.rays_o[3 * e + 2] = (float)v.origin[2];
    a.rays_d[3 * e] = (float)rx;
    a.rays_d[3 * e + 1] = (float)ry;
    a.rays_d[3 * e + 2] = (float)rz;
    a.cam_rays_d[3 * e] = (float)qx;
    a.cam_rays_d[3 * e + 1] = (float)qy;
    a.cam_rays_d[3 * e + 2] = (float)qz;
    a.cam_z[e] = (float)qz;

    // ---- the initial depth ---------------------------------------------------------------------------------------------------
    const float span = v.far_z - v.near_z;
    a.z[e] = a.u[e] * span + v.near_z;
}

__global__ __launch_bounds__(kBlock) void mono_pairs_kernel(ScgMono a) {
    __shared__ int s_red[kBlock / kWave];
    const int s = blockIdx.x;
    const ScgMonoSegment seg = a.segments[s];
    if (!segment_ok(seg, a.N, a.V) || (unsigned)seg.partner >= (unsigned)a.nseg) return;       // uniform: before any barrier
    const ScgMonoSegment back = a.segments[seg.partner];
    if (!segment_ok(back, a.N, a.V) || back.count != seg.count) return;
    int mine = 0;
    for (int k = threadIdx.x; k < seg.count; k += kBlock) {
        const size_t e = (size_t)seg.offset + k, p = (size_t)back.offset + k;
        a.uv_t[2 * e] = a.uv[2 * p];
        a.uv_t[2 * e + 1] = a.uv[2 * p + 1];
        const float prod = a.blender_mask[e] * a.blender_mask[p];
        const float valid = prod > 0.0f ? 1.0f : 0.0f;
        a.valid[e] = valid;
        mine += prod > 0.0f ? 1 : 0;
    }
    const int count = wg_reduce<kBlock / kWave>(mine, s_red, Sum());
    if (threadIdx.x == 0) a.counts[s] = count;
    const float fc = (float)count;
    for (int k = threadIdx.x; k < seg.count; k += kBlock) {
        const size_t e = (size_t)seg.offset + k;
        a.wgt[e] = count > 0 ? a.valid[e] / fc : 0.0f;           // this thread's own store of the first loop
    }
}

static int mono_validate(const ScgMono* a, const char* who) {
    if (!a) return fail(SCG_E_NULL, "%s: the argument struct is NULL", who);
    if (a->struct_bytes != (int32_t)sizeof(ScgMono))
        return fail(SCG_E_RANGE, "%s: struct_bytes = %d, the library's ScgMono has %zu", who, a->struct_bytes, sizeof(ScgMono));
    if (a->V < 1 || a->V > SCG_MONO_MAX_VIEWS || a->nseg < 1 || a->nseg > SCG_MONO_MAX_SEGMENTS || a->N < 1 || a->ngroups < 1 ||
        a->ngroups >= (1 << 24))
        return fail(SCG_E_RANGE, "%s: V = %d, nseg = %d, N = %d or ngroups = %d out of range", who, a->V, a->nseg, a->N, a->ngroups);
    if (a->max_view_pixels < 1 || a->max_view_pixels > a->image_pixels || a->max_view_pixels >= (1ll << 31) || a->mask_pixels < 0)
        return fail(SCG_E_RANGE, "%s: image_pixels = %lld, max_view_pixels = %lld or mask_pixels = %lld out of range", who,
                    (long long)a->image_pixels, (long long)a->max_view_pixels, (long long)a->mask_pixels);
    const void* ptrs[] = {a->views, a->segments, a->groups, a->image_bytes, a->match_pixel, a->u, a->image_color, a->uv, a->color,
                          a->blender_mask, a->rays_o, a->rays_d, a->cam_rays_d, a->cam_z, a->z, a->uv_t, a->valid, a->wgt, a->counts};
    for (const void* p : ptrs)
        if (!p) return fail(SCG_E_NULL, "%s pointer is NULL", who);
    if (a->mask_pixels > 0 && !a->masks) return fail(SCG_E_NULL, "%s: masks is NULL with mask_pixels = %lld", who, (long long)a->mask_pixels);
    if (reinterpret_cast<uintptr_t>(a->views) % 8) return fail(SCG_E_ALIGN, "%s: views not 8-byte aligned", who);
    for (const void* p : ptrs)
        if (p != a->image_bytes && reinterpret_cast<uintptr_t>(p) % 4) return fail(SCG_E_ALIGN, "%s: a table or an fp32 array is not 4-byte aligned", who);
    if (reinterpret_cast<uintptr_t>(a->masks) % 4) return fail(SCG_E_ALIGN, "%s: masks not 4-byte aligned", who);
    return 0;
}

}  // namespace scg

using namespace scg;

extern "C" {

size_t scg_mono_struct_bytes(int32_t which) {
    switch (which) {
        case 0: return sizeof(ScgMono);
        case 1: return sizeof(ScgMonoView);
        case 2: return sizeof(ScgMonoSegment);
        case 3: return sizeof(ScgMonoGroup);
        default: return 0;
    }
}

int32_t scg_mono_block(void) { return kBlock; }

int scg_mono_images(const ScgMono* a, void* stream) {
    if (int rc = mono_validate(a, "mono_images")) return rc;
    const int64_t per = (int64_t)kBlock * kMonoImageTrips;
    const int64_t trips = (a->max_view_pixels * 3 + per - 1) / per;          // < 2^31 * 3 / 1024
    hipLaunchKernelGGL(mono_images_kernel, dim3((unsigned)trips, (unsigned)a->V), dim3(kBlock), 0, reinterpret_cast<hipStream_t>(stream),
                       a->image_bytes, a->views, a->image_pixels, a->image_color);
    return check_hip(hipGetLastError(), "mono_images_kernel");
}

int scg_mono_matches(const ScgMono* a, void* stream) {
    if (int rc = mono_validate(a, "mono_matches")) return rc;
    hipLaunchKernelGGL(mono_matches_kernel, dim3((unsigned)a->ngroups), dim3(kBlock), 0, reinterpret_cast<hipStream_t>(stream), *a);
    return check_hip(hipGetLastError(), "mono_matches_kernel");
}

int scg_mono_pairs(const ScgMono* a, void* stream) {
    if (int rc = mono_validate(a, "mono_pairs")) return rc;
    hipLaunchKernelGGL(mono_pairs_kernel, dim3((unsigned)a->nseg), dim3(kBlock), 0, reinterpret_cast<hipStream_t>(stream), *a);
    return check_hip(hipGetLastError(), "mono_pairs_kernel");
}

}  // extern "C"

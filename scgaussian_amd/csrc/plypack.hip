// plypack.hip — libscg_io.so: the bodies of the scene files packed and unpacked on the GPU (include/io/scg_ply.h).
//
// GaussianModel.save_ply / load_ply (scene/gaussian_model.py:565-609, :653-756) and storePly (scene/dataset_readers.py:127-142)
// are a re-layout: every output byte is decided from one Gaussian alone, the SH block is transposed between coefficient-major
// (memory) and channel-major (file).  A workgroup owns a TILE of kRows consecutive rows and stages it through LDS, so that both
// sides of the copy are contiguous in global memory: the tensor side is `rows x width` consecutive dwords of each tensor, the
// record side `rows x stride` consecutive dwords of the body.  Every global access is a lane-contiguous dword; nothing is atomic,
// nothing is read by the host, no workgroup waits on another.  Rows are indexed in 64 bits.
//
// LDS layout: the tile lies in LDS as it lies in the file, row r at dword r * stride.  The strides are 69 and 62 dwords (11 and 55
// in the colour tiles); the one walk with a row per lane (the position and colour of a row) runs over the odd ones, and an odd dword
// stride is coprime with the 32 banks of ds_read_b32 / ds_write_b32, so the 32 lanes of a half wave fall on 32 banks (CDNA HIP
// programming guide §2 "Bank structure" and Guideline 4: break power-of-two row strides).  The transposing copies walk LDS with
// the stride of the permutation (15 or 3 dwords inside a row): odd again.
//
// Compiled with -ffp-contract=off: x = rayo + rayd * zval is a product and a sum, each rounded, as torch and numpy round them; the
// colour is the chain of single fp32 operations of include/io/scg_ply.h.  Everything else moves as uint32_t.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/io/scg_ply.h"
#include "host_align.h"
#include "host_error.h"
#include "sh_eval.h"

#pragma clang fp contract(off)

namespace scg {
namespace {

constexpr int kRows = SCG_PLY_TILE_ROWS;
constexpr int kBlock = 256;
constexpr int kRay = SCG_PLY_RAY_FLOATS, kBg = SCG_PLY_BG_FLOATS, kColor = SCG_PLY_COLOR_BYTES;
constexpr int kRest = 45;                              // floats of a features_rest row: 15 coefficients x 3 channels
// destination columns of a record (the order of construct_list_of_attributes)
constexpr int kColDc = 6, kColRest = 9, kColOpacity = 54, kColScale = 55, kColRot = 58, kColZval = 62, kColRayo = 63, kColRayd = 66;
static_assert(kRows % 4 == 0 && (kRows * kColor) % 4 == 0, "a tile of colour records is a whole number of dwords");

thread_local ErrorText g_err = {};

ScgPlyLayout layout_of(int32_t nr, int32_t nb) {
    ScgPlyLayout l;
    l.ray_offset = 0;
    l.ray_bytes = (uint64_t)nr * kRay * 4;
    l.bg_offset = align_to<256>(l.ray_offset + l.ray_bytes);
    l.bg_bytes = (uint64_t)nb * kBg * 4;
    l.color_offset = align_to<256>(l.bg_offset + l.bg_bytes);
    l.color_bytes = align_to<4>(((uint64_t)nr + (uint64_t)nb) * kColor);
    l.total = align_to<256>(l.color_offset + l.color_bytes);
    return l;
}

int tiles_of(int64_t rows) { return (int)((rows + kRows - 1) / kRows); }

// ---- device side ---------------------------------------------------------------------------------------------------------------
// The byte numpy's array cast float32 -> uint8 gives on x86-64.  The hardware's float-to-int conversion saturates; the range test
// keeps it away from every value where saturating and wrapping differ, and sends NaN (every comparison false) to 0.
__device__ __forceinline__ uint32_t color_byte(float v) {
    if (!(fabsf(v) < 2147483648.0f)) return 0u;
    return (uint32_t)(int32_t)v & 255u;
}

// `n` rows of a tensor of W dwords per row, from row `first` on, into columns [col, col + W) of the LDS tile.  TRANSPOSE: the row
// is (15, 3) coefficient-major and goes to (3, 15) channel-major.
template <int W, bool TRANSPOSE>
__device__ __forceinline__ void tensor_to_tile(uint32_t* tile, int stride, int col, const float* __restrict__ src, size_t first,
                                               int n) {
    const uint32_t* s = reinterpret_cast<const uint32_t*>(src) + first * W;
    for (int i = threadIdx.x; i < n * W; i += kBlock) {
        const int r = i / W, k = i - r * W;
        const int c = TRANSPOSE ? (k % 3) * 15 + k / 3 : k;
        tile[r * stride + col + c] = s[i];
    }
}

// The inverse: the tensor's column k of row r comes from dword table[col + c] of the record.
template <int W, bool TRANSPOSE>
__device__ __forceinline__ void tile_to_tensor(const uint32_t* tile, int stride, const int32_t* table, int col,
                                               const float* dst_const, size_t first, int n) {
    uint32_t* d = reinterpret_cast<uint32_t*>(const_cast<float*>(dst_const)) + first * W;
    for (int i = threadIdx.x; i < n * W; i += kBlock) {
        const int r = i / W, k = i - r * W;
        const int c = TRANSPOSE ? (k % 3) * 15 + k / 3 : k;
        d[i] = tile[r * stride + table[col + c]];
    }
}

__device__ __forceinline__ void tile_out(const uint32_t* tile, uint32_t* __restrict__ dst, int ndw, int pad_dw) {
    for (int i = threadIdx.x; i < ndw; i += kBlock) dst[i] = tile[i];
    if ((int)threadIdx.x < pad_dw) dst[ndw + threadIdx.x] = 0u;      // the gap up to the next body (last tile of a body only)
}

// x = rayo + rayd * zval of one staged row.  Everything is read before anything is written: `out` may overlap the inputs.
__device__ __forceinline__ void ray_position(uint32_t* row, int zval, int rayo, int rayd, int out) {
    const float z = __uint_as_float(row[zval]);
    float x[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float prod = __uint_as_float(row[rayd + c]) * z;
        x[c] = __uint_as_float(row[rayo + c]) + prod;
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) row[out + c] = __float_as_uint(x[c]);
}

struct PackArgs {
    ScgModel m;
    uint32_t* ray;             // the three bodies
    uint32_t* bg;
    uint32_t* color;
    int ray_tiles, bg_tiles, color_tiles;
    int ray_pad, bg_pad, color_pad;      // dwords of zeros behind each body
    const float* campos;       // colour-view kernel only
};

__device__ __forceinline__ void pack_ray_tile(const PackArgs& a, int t, uint32_t* tile) {
    const ScgModelSet& s = a.m.ray;
    const size_t first = (size_t)t * kRows;
    const int n = (int)min((size_t)kRows, (size_t)s.count - first);
    tensor_to_tile<3, false>(tile, kRay, kColDc, s.features_dc, first, n);
    tensor_to_tile<kRest, true>(tile, kRay, kColRest, s.features_rest, first, n);
    tensor_to_tile<1, false>(tile, kRay, kColOpacity, s.opacity, first, n);
    tensor_to_tile<3, false>(tile, kRay, kColScale, s.scaling, first, n);
    tensor_to_tile<4, false>(tile, kRay, kColRot, s.rotation, first, n);
    tensor_to_tile<1, false>(tile, kRay, kColZval, s.zval, first, n);
    tensor_to_tile<3, false>(tile, kRay, kColRayo, s.rayo, first, n);
    tensor_to_tile<3, false>(tile, kRay, kColRayd, s.rayd, first, n);
    __syncthreads();
    if ((int)threadIdx.x < n) {                                    // a row per lane: stride 69
        uint32_t* row = tile + threadIdx.x * kRay;
        ray_position(row, kColZval, kColRayo, kColRayd, 0);
        row[3] = row[4] = row[5] = 0u;
    }
    __syncthreads();
    tile_out(tile, a.ray + first * kRay, n * kRay, t == a.ray_tiles - 1 ? a.ray_pad : 0);
}

__device__ __forceinline__ void pack_bg_tile(const PackArgs& a, int t, uint32_t* tile) {
    const ScgModelSet& s = a.m.bg;
    const size_t first = (size_t)t * kRows;
    const int n = (int)min((size_t)kRows, (size_t)s.count - first);
    tensor_to_tile<3, false>(tile, kBg, 0, s.xyz, first, n);
    tensor_to_tile<3, false>(tile, kBg, kColDc, s.features_dc, first, n);
    tensor_to_tile<kRest, true>(tile, kBg, kColRest, s.features_rest, first, n);
    tensor_to_tile<1, false>(tile, kBg, kColOpacity, s.opacity, first, n);
    tensor_to_tile<3, false>(tile, kBg, kColScale, s.scaling, first, n);
    tensor_to_tile<4, false>(tile, kBg, kColRot, s.rotation, first, n);
    for (int i = threadIdx.x; i < 3 * n; i += kBlock) tile[(i / 3) * kBg + 3 + i % 3] = 0u;
    __syncthreads();
    tile_out(tile, a.bg + first * kBg, n * kBg, t == a.bg_tiles - 1 ? a.bg_pad : 0);
}

// A tile of the colour body: rows [first, first + n) of ray-bound rows followed by background rows, so a tile may hold both.
// Staged row (stride kIn): 0 zval | 1-3 rayo (background: xyz) | 4-6 rayd | 7-9 f_dc | 10-54 f_rest (view-dependent colour only).
// The row's lane then overwrites dwords 0-2 with the position and 3 with the three colour bytes, and the body's dwords are
// gathered from there byte by byte.  DEG < 0: colour = f_dc * 255.
template <int DEG>
__device__ __forceinline__ void pack_color_tile(const PackArgs& a, int t, uint32_t* tile) {
    constexpr int kIn = DEG < 0 ? 11 : 55;
    const size_t nr = (size_t)a.m.ray.count, P = nr + (size_t)a.m.bg.count;
    const size_t first = (size_t)t * kRows;
    const int n = (int)min((size_t)kRows, P - first);
    const int n_ray = first >= nr ? 0 : (int)min((size_t)n, nr - first);
    const int n_bg = n - n_ray;
    if (n_ray) {
        const ScgModelSet& s = a.m.ray;
        tensor_to_tile<1, false>(tile, kIn, 0, s.zval, first, n_ray);
        tensor_to_tile<3, false>(tile, kIn, 1, s.rayo, first, n_ray);
        tensor_to_tile<3, false>(tile, kIn, 4, s.rayd, first, n_ray);
        tensor_to_tile<3, false>(tile, kIn, 7, s.features_dc, first, n_ray);
        if (DEG > 0) tensor_to_tile<kRest, false>(tile, kIn, 10, s.features_rest, first, n_ray);
    }
    if (n_bg) {
        const ScgModelSet& s = a.m.bg;
        const size_t bfirst = first + n_ray - nr;
        uint32_t* part = tile + n_ray * kIn;
        tensor_to_tile<3, false>(part, kIn, 1, s.xyz, bfirst, n_bg);
        tensor_to_tile<3, false>(part, kIn, 7, s.features_dc, bfirst, n_bg);
        if (DEG > 0) tensor_to_tile<kRest, false>(part, kIn, 10, s.features_rest, bfirst, n_bg);
    }
    __syncthreads();
    if ((int)threadIdx.x < n) {                                    // a row per lane: stride 11 or 55
        uint32_t* row = tile + threadIdx.x * kIn;
        if ((int)threadIdx.x < n_ray) ray_position(row, 0, 1, 4, 0);
        else { row[0] = row[1]; row[1] = row[2]; row[2] = row[3]; }         // bit copies
        float v[3];
        if constexpr (DEG < 0) {
#pragma unroll
            for (int c = 0; c < 3; ++c) v[c] = __uint_as_float(row[7 + c]) * 255.0f;
        } else {
            constexpr int K = 3 * (DEG + 1) * (DEG + 1);
            float sh[K];
#pragma unroll
            for (int k = 0; k < K; ++k) sh[k] = __uint_as_float(row[7 + k]);
            const float dx = __uint_as_float(row[0]) - a.campos[0];
            const float dy = __uint_as_float(row[1]) - a.campos[1];
            const float dz = __uint_as_float(row[2]) - a.campos[2];
            const float len = sqrtf((dx * dx + dy * dy) + dz * dz);
            float rgb[3];
            eval_sh<DEG>(sh, dx / len, dy / len, dz / len, rgb);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float r = rgb[c] + 0.5f;
                v[c] = (r < 0.0f ? 0.0f : r) * 255.0f;             // clamp_min keeps NaN; its byte is 0 either way
            }
        }
        row[3] = color_byte(v[0]) | (color_byte(v[1]) << 8) | (color_byte(v[2]) << 16);
    }
    __syncthreads();
    const int nbytes = n * kColor, ndw = (nbytes + 3) >> 2;
    uint32_t* dst = a.color + (size_t)t * (kRows * kColor / 4);
    for (int d = threadIdx.x; d < ndw; d += kBlock) {
        uint32_t word = 0u;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int at = 4 * d + b;
            if (at < nbytes) {
                const int r = at / kColor, o = at - r * kColor;
                uint32_t byte = 0u;
                if (o < 12) byte = (tile[r * kIn + (o >> 2)] >> (8 * (o & 3))) & 255u;
                else if (o >= 24) byte = (tile[r * kIn + 3] >> (8 * (o - 24))) & 255u;
                word |= byte << (8 * b);
            }
        }
        dst[d] = word;
    }
    if (t == a.color_tiles - 1 && (int)threadIdx.x < a.color_pad) dst[ndw + threadIdx.x] = 0u;
}

__global__ void __launch_bounds__(kBlock) ply_pack_kernel(const PackArgs a) {
    __shared__ uint32_t tile[kRows * kRay];
    int t = blockIdx.x;
    if (t < a.ray_tiles) return pack_ray_tile(a, t, tile);
    t -= a.ray_tiles;
    if (t < a.bg_tiles) return pack_bg_tile(a, t, tile);
    pack_color_tile<-1>(a, t - a.bg_tiles, tile);
}

template <int DEG>
__global__ void __launch_bounds__(kBlock) ply_color_view_kernel(const PackArgs a) {
    __shared__ uint32_t tile[kRows * 55];
    pack_color_tile<DEG>(a, blockIdx.x, tile);
}

// upload: rows * stride dwords, then the table.  Dynamic LDS: kRows * stride dwords of records, then the table.
template <bool BG>
__global__ void __launch_bounds__(kBlock) ply_unpack_kernel(const uint32_t* __restrict__ upload, size_t rows, int stride,
                                                             const ScgModelSet s) {
    extern __shared__ uint32_t lds[];
    constexpr int kCols = BG ? kBg : kRay;
    int32_t* table = reinterpret_cast<int32_t*>(lds + kRows * stride);
    const size_t first = (size_t)blockIdx.x * kRows;
    const int n = (int)min((size_t)kRows, rows - first);
    // (the host validated its own copy of the table; this one is clamped, so that a copy that differs cannot leave the record)
    if ((int)threadIdx.x < kCols) table[threadIdx.x] = min(max((int32_t)upload[rows * stride + threadIdx.x], 0), stride - 1);
    const uint32_t* src = upload + first * stride;
    for (int i = threadIdx.x; i < n * stride; i += kBlock) lds[i] = src[i];
    __syncthreads();
    if (BG) tile_to_tensor<3, false>(lds, stride, table, 0, s.xyz, first, n);
    tile_to_tensor<3, false>(lds, stride, table, kColDc, s.features_dc, first, n);
    tile_to_tensor<kRest, true>(lds, stride, table, kColRest, s.features_rest, first, n);
    tile_to_tensor<1, false>(lds, stride, table, kColOpacity, s.opacity, first, n);
    tile_to_tensor<3, false>(lds, stride, table, kColScale, s.scaling, first, n);
    tile_to_tensor<4, false>(lds, stride, table, kColRot, s.rotation, first, n);
    if (!BG) {
        tile_to_tensor<1, false>(lds, stride, table, kColZval, s.zval, first, n);
        tile_to_tensor<3, false>(lds, stride, table, kColRayo, s.rayo, first, n);
        tile_to_tensor<3, false>(lds, stride, table, kColRayd, s.rayd, first, n);
    }
}

// ---- validation ----------------------------------------------------------------------------------------------------------------
int check_set(const char* who, const ScgModelSet& s, bool ray) {
    if (s.count < 0) return g_err.fail(SCG_E_RANGE, "%s: a set of %d Gaussians", who, s.count);
    if (s.count == 0) return 0;
    const bool have = s.features_dc && s.features_rest && s.opacity && s.scaling && s.rotation &&
                      (ray ? (s.zval && s.rayo && s.rayd) : s.xyz != nullptr);
    if (!have) return g_err.fail(SCG_E_NULL, "%s: a tensor of the %s set is NULL", who, ray ? "ray-bound" : "background");
    return 0;
}

int check_model(const char* who, const ScgModel* m) {
    if (!m) return g_err.fail(SCG_E_NULL, "%s: model is NULL", who);
    if (int rc = check_set(who, m->ray, true)) return rc;
    return check_set(who, m->bg, false);
}

int check_buffer(const char* who, const void* buffer, size_t bytes, uint64_t need) {
    if (!buffer) return g_err.fail(SCG_E_NULL, "%s: buffer is NULL", who);
    if (bytes < need) return g_err.fail(SCG_E_SCRATCH, "%s: buffer of %zu bytes < %llu", who, bytes, (unsigned long long)need);
    if (reinterpret_cast<uintptr_t>(buffer) % 16) return g_err.fail(SCG_E_ALIGN, "%s: buffer not 16-byte aligned", who);
    return 0;
}

}  // namespace
}  // namespace scg

using namespace scg;

extern "C" {

const char* scg_io_last_error(void) { return g_err.text; }
int32_t scg_io_abi_version(void) { return SCG_IO_ABI_VERSION; }
size_t scg_ply_layout_bytes(void) { return sizeof(ScgPlyLayout); }

int scg_ply_layout(int32_t nr, int32_t nb, ScgPlyLayout* out) {
    if (!out) return g_err.fail(SCG_E_NULL, "scg_ply_layout: out is NULL");
    if (nr < 0 || nb < 0) return g_err.fail(SCG_E_RANGE, "scg_ply_layout: %d ray-bound and %d background Gaussians", nr, nb);
    *out = layout_of(nr, nb);
    return 0;
}

int scg_ply_pack(const ScgModel* model, void* buffer, size_t buffer_bytes, void* stream) {
    if (int rc = check_model("scg_ply_pack", model)) return rc;
    const int32_t nr = model->ray.count, nb = model->bg.count;
    if (nr == 0 && nb == 0) return 0;
    const ScgPlyLayout l = layout_of(nr, nb);
    if (int rc = check_buffer("scg_ply_pack", buffer, buffer_bytes, l.total)) return rc;
    PackArgs a;
    a.m = *model;
    char* base = static_cast<char*>(buffer);
    a.ray = reinterpret_cast<uint32_t*>(base + l.ray_offset);
    a.bg = reinterpret_cast<uint32_t*>(base + l.bg_offset);
    a.color = reinterpret_cast<uint32_t*>(base + l.color_offset);
    a.ray_tiles = tiles_of(nr);
    a.bg_tiles = tiles_of(nb);
    a.color_tiles = tiles_of((int64_t)nr + nb);
    a.ray_pad = (int)((l.bg_offset - (l.ray_offset + l.ray_bytes)) / 4);
    a.bg_pad = (int)((l.color_offset - (l.bg_offset + l.bg_bytes)) / 4);
    a.color_pad = (int)((l.total - (l.color_offset + l.color_bytes)) / 4);
    a.campos = nullptr;
    const int64_t blocks = (int64_t)a.ray_tiles + a.bg_tiles + a.color_tiles;
    if (blocks > 0x7fffffff) return g_err.fail(SCG_E_RANGE, "scg_ply_pack: %lld tiles are more than one launch takes", (long long)blocks);
    hipLaunchKernelGGL(ply_pack_kernel, dim3((unsigned)blocks), dim3(kBlock), 0, static_cast<hipStream_t>(stream), a);
    return g_err.check_hip(hipGetLastError(), "scg_ply_pack");
}

int scg_ply_pack_color_view(const ScgModel* model, int32_t sh_degree, const float* campos, void* buffer, size_t buffer_bytes,
                            void* stream) {
    if (int rc = check_model("scg_ply_pack_color_view", model)) return rc;
    if (sh_degree < 0 || sh_degree > 3) return g_err.fail(SCG_E_RANGE, "scg_ply_pack_color_view: SH degree %d is not 0..3", sh_degree);
    if (!campos) return g_err.fail(SCG_E_NULL, "scg_ply_pack_color_view: campos is NULL");
    const int64_t P = (int64_t)model->ray.count + model->bg.count;
    if (P == 0) return 0;
    const uint64_t bytes = ((uint64_t)P * kColor + 3u) & ~(uint64_t)3u;
    if (int rc = check_buffer("scg_ply_pack_color_view", buffer, buffer_bytes, bytes)) return rc;
    PackArgs a;
    a.m = *model;
    a.ray = a.bg = nullptr;
    a.color = static_cast<uint32_t*>(buffer);
    a.ray_tiles = a.bg_tiles = 0;
    a.color_tiles = tiles_of(P);
    a.ray_pad = a.bg_pad = a.color_pad = 0;
    a.campos = campos;
    const dim3 grid((unsigned)a.color_tiles), block(kBlock);
    hipStream_t st = static_cast<hipStream_t>(stream);
    switch (sh_degree) {
        case 0: hipLaunchKernelGGL(ply_color_view_kernel<0>, grid, block, 0, st, a); break;
        case 1: hipLaunchKernelGGL(ply_color_view_kernel<1>, grid, block, 0, st, a); break;
        case 2: hipLaunchKernelGGL(ply_color_view_kernel<2>, grid, block, 0, st, a); break;
        default: hipLaunchKernelGGL(ply_color_view_kernel<3>, grid, block, 0, st, a); break;
    }
    return g_err.check_hip(hipGetLastError(), "scg_ply_pack_color_view");
}

int scg_ply_unpack(const void* upload, size_t body_bytes, const int32_t* table_host, int32_t rows, int32_t stride, int32_t bg,
                   const ScgModel* model, void* stream) {
    const char* who = "scg_ply_unpack";
    if (!upload || !table_host) return g_err.fail(SCG_E_NULL, "%s: %s is NULL", who, upload ? "table_host" : "upload");
    if (int rc = check_model(who, model)) return rc;
    if (rows < 0) return g_err.fail(SCG_E_RANGE, "%s: %d rows", who, rows);
    if (stride < 1 || stride > SCG_PLY_MAX_STRIDE)
        return g_err.fail(SCG_E_RANGE, "%s: a record of %d dwords is outside 1..%d", who, stride, SCG_PLY_MAX_STRIDE);
    if (body_bytes != (size_t)rows * (size_t)stride * 4)
        return g_err.fail(SCG_E_SCRATCH, "%s: a body of %zu bytes is not %d rows of %d dwords", who, body_bytes, rows, stride);
    const int cols = bg ? kBg : kRay;
    for (int d = 0; d < cols; ++d)
        if (table_host[d] < 0 || table_host[d] >= stride)
            return g_err.fail(SCG_E_RANGE, "%s: table[%d] = %d is outside the record of %d dwords", who, d, table_host[d], stride);
    if (reinterpret_cast<uintptr_t>(upload) % 16) return g_err.fail(SCG_E_ALIGN, "%s: upload not 16-byte aligned", who);
    const ScgModelSet& s = bg ? model->bg : model->ray;
    if (s.count != rows) return g_err.fail(SCG_E_RANGE, "%s: the model's set holds %d rows, the file %d", who, s.count, rows);
    if (rows == 0) return 0;
    const dim3 grid((unsigned)tiles_of(rows)), block(kBlock);
    const size_t lds = ((size_t)kRows * stride + cols) * 4;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const uint32_t* up = static_cast<const uint32_t*>(upload);
    if (bg) hipLaunchKernelGGL(ply_unpack_kernel<true>, grid, block, lds, st, up, (size_t)rows, (int)stride, s);
    else hipLaunchKernelGGL(ply_unpack_kernel<false>, grid, block, lds, st, up, (size_t)rows, (int)stride, s);
    return g_err.check_hip(hipGetLastError(), who);
}

}  // extern "C"

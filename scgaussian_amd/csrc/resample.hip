// resample.hip — libscg_img.so: Pillow's bicubic Image.resize of 8-bit images on the GPU, byte for byte (include/img/scg_resample.h).
//
// PILtoTorch (utils/general_utils.py:22-28) downsizes every camera image on one host core: for a 4032 x 3024 photograph at -r 8 a
// 33-tap filter over 12 M pixels.  For 8-bit images Pillow's resampler is integer arithmetic — coefficients with 22 fractional bits,
// a horizontal pass rounded to bytes, a vertical pass rounded to bytes — so two kernels equal it exactly.  The tables (window and
// coefficients per output index) depend on double arithmetic in a fixed order and are built by the caller on the host.
//
// Horizontal pass (win -> wout), src (n, hin, win, C) tight -> mid (n, hin, pitch):
//   a source row starts at any byte phase and a pixel is 3 bytes, so there is no lane-per-pixel dword view of it.  A workgroup owns
//   a STRIP of kStrip output columns over kStripRows source rows.  Its slice of the tables (kStrip x ksize ints) is loaded into LDS
//   once and reused down the rows: at -r 8 the whole table (66 KB) is larger than a source row (12 KB), so a workgroup per row would
//   move more coefficient bytes than pixels.  The source span of the strip is read `rt` rows at a time as ALIGNED dwords, lane-contiguous
//   (CDNA HIP programming guide §1 "Coalescing"), into LDS; the byte phase of each row is carried into the LDS byte address.  A lane owns one
//   output column (all channels) of four rows in 32 at a time; the coefficient reads of a wave walk LDS with the odd stride ksize (every
//   ksize is 2 * ceil(support) + 1), so the 32 columns fall on 32 banks and the two rows of a wave share the address.  The output
//   bytes are gathered in LDS and leave as whole dwords: the strip starts at byte 32 * C * strip, and the pitch is a multiple of 16.
// Vertical pass (hin -> hout), mid (or src when the width is unchanged) -> out (n, hout, wout, C) tight [+ float (n, C, hout, wout)]:
//   a lane owns 4 consecutive bytes of an output row; the row's window and coefficients are the same for the whole workgroup
//   (blockIdx.y), so they arrive as uniform loads.  The loop reads one dword per source row into four int32 accumulators.  The
//   tight output row starts at byte (image * hout + y) * wout * C: a lane stores a dword where its address is aligned and bytes
//   elsewhere (every row when wout * C is a multiple of 4, the usual case).  hout == hin: one tap of 2^22, a copy.
//
// Offsets are 64-bit (twenty 36 MB images exceed 2^31 bytes).  No atomics, no host read, no workgroup waits on another.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/img/scg_resample.h"
#include "host_align.h"
#include "host_error.h"

namespace scg {
namespace {

constexpr int kBlock = 256;
constexpr int kWave = 64;
constexpr int kStrip = SCG_RESAMPLE_STRIP;
constexpr int kStripRows = SCG_RESAMPLE_STRIP_ROWS;
constexpr int kRowSubs = kBlock / kStrip;              // rows of a staged chunk the lanes of a workgroup stand on
constexpr int kRowsPerLane = 4;                        // ... each lane computing this many of them at a time
constexpr int kVTile = SCG_RESAMPLE_VTILE;
constexpr int kPitchAlign = SCG_RESAMPLE_PITCH_ALIGN;
constexpr int kHalf = 1 << 21, kOne = 1 << 22, kShift = 22;
constexpr size_t kLdsBudget = 40 * 1024;               // per workgroup, so that four fit a compute unit; a long span takes what kRowSubs rows need
static_assert(kBlock % kStrip == 0 && kStrip <= kWave && (kStrip * 3) % 4 == 0, "a strip of either pixel size is whole dwords");
static_assert(kVTile == 4 * kBlock, "4 bytes per lane");

thread_local ErrorText g_err = {};

size_t pitch_of(int32_t wout, int32_t channels) { return align_up((size_t)wout * channels, kPitchAlign); }

// ---- device side ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t to_byte(int acc) {
    const int v = acc >> kShift;                        // arithmetic: a negative accumulator gives a negative value, hence 0
    return (uint32_t)min(max(v, 0), 255);
}

struct HArgs {
    const uint8_t* src;
    uint8_t* mid;
    const int32_t* bounds;
    const int32_t* coeffs;
    int hin, win, wout, ksize;
    int pitch;           // bytes of a row of mid
    int lp;              // dwords of LDS per staged source row
    int rt;              // source rows staged at a time, a multiple of kRowSubs
};

// dynamic LDS: coef[kStrip * ksize] | wmin[kStrip] | wcnt[kStrip] | tile[rt * lp] | otile[rt * kStrip * C / 4]
template <int C>
__global__ void __launch_bounds__(kBlock) resample_h_kernel(const HArgs a) {
    extern __shared__ uint32_t lds[];
    constexpr int kOutDw = kStrip * C / 4;
    int32_t* coef = reinterpret_cast<int32_t*>(lds);
    int* wmin = reinterpret_cast<int*>(lds + kStrip * a.ksize);
    int* wcnt = wmin + kStrip;
    uint32_t* tile = reinterpret_cast<uint32_t*>(wcnt + kStrip);
    uint32_t* otile = tile + (size_t)a.rt * a.lp;

    const int tid = threadIdx.x;
    const int j0 = blockIdx.x * kStrip;
    const int ncol = min(kStrip, a.wout - j0);
    const int row0 = blockIdx.y * kStripRows;
    const int nrows = min(kStripRows, a.hin - row0);
    const size_t img = blockIdx.z;

    // the strip's windows, clamped into the source row and into ksize coefficients, and its coefficients
    if (tid < kStrip) {
        const int j = min(j0 + tid, a.wout - 1);
        const int xmin = min(max(a.bounds[2 * j], 0), a.win - 1);
        wmin[tid] = xmin;
        wcnt[tid] = min(max(a.bounds[2 * j + 1], 0), min(a.ksize, a.win - xmin));
    }
    for (int i = tid; i < ncol * a.ksize; i += kBlock) coef[i] = a.coeffs[(size_t)j0 * a.ksize + i];
    __syncthreads();
    int x0 = a.win, x1 = 0;
    for (int c = 0; c < ncol; ++c) {                    // uniform LDS reads
        x0 = min(x0, wmin[c]);
        x1 = max(x1, wmin[c] + wcnt[c]);
    }
    // (for the tables of these sizes the span fits the staged row; any others are cut to it)
    x1 = min(x1, x0 + (a.lp * 4 - 3) / C);
    const int span_bytes = (x1 - x0) * C;

    const int col = tid % kStrip, rsub = tid / kStrip;
    const int xm = wmin[col] - x0;
    const int cnt = max(min(wcnt[col], x1 - wmin[col]), 0);
    const int32_t* kc = coef + col * a.ksize;
    const int wave = tid / kWave, lane = tid % kWave;

    const size_t row_bytes = (size_t)a.win * C;
    const uintptr_t base = reinterpret_cast<uintptr_t>(a.src) + (img * a.hin + row0) * row_bytes + (size_t)x0 * C;
    const int strip_b0 = j0 * C;                        // a multiple of 32: dword-aligned in mid
    const int out_dw = (min(kStrip * C, a.wout * C - strip_b0) + 3) >> 2;
    uint8_t* mid_rows = a.mid + (img * a.hin + row0) * (size_t)a.pitch + strip_b0;

    for (int c0 = 0; c0 < nrows; c0 += a.rt) {
        const int rn = min(a.rt, nrows - c0);
        // stage: the aligned dwords that hold the span of each row, a row per wave at a time
        for (int rr = wave; rr < rn; rr += kBlock / kWave) {
            const uintptr_t at = base + (size_t)(c0 + rr) * row_bytes;
            const uint32_t* from = reinterpret_cast<const uint32_t*>(at & ~(uintptr_t)3);
            const int nd = ((int)(at & 3) + span_bytes + 3) >> 2;
            for (int d = lane; d < nd; d += kWave) tile[rr * a.lp + d] = from[d];
        }
        __syncthreads();
        // kRowsPerLane rows of the chunk at a time per lane: one coefficient read serves them all, and their accumulator
        // chains are independent (a row beyond the chunk repeats the last one and is not stored)
        for (int rr = rsub; rr < rn; rr += kRowSubs * kRowsPerLane) {
            const uint8_t* sb[kRowsPerLane];
            int acc[kRowsPerLane][C];
#pragma unroll
            for (int q = 0; q < kRowsPerLane; ++q) {
                const int r = min(rr + q * kRowSubs, rn - 1);
                const int phase = (int)((base + (size_t)(c0 + r) * row_bytes) & 3);
                sb[q] = reinterpret_cast<const uint8_t*>(tile + r * a.lp) + phase + xm * C;
#pragma unroll
                for (int c = 0; c < C; ++c) acc[q][c] = kHalf;
            }
#pragma unroll 2
            for (int t = 0; t < cnt; ++t) {
                const int k = kc[t];
#pragma unroll
                for (int q = 0; q < kRowsPerLane; ++q)
#pragma unroll
                    for (int c = 0; c < C; ++c) acc[q][c] += (int)sb[q][t * C + c] * k;
            }
#pragma unroll
            for (int q = 0; q < kRowsPerLane; ++q) {
                const int r = rr + q * kRowSubs;
                if (r < rn) {
                    uint8_t* ob = reinterpret_cast<uint8_t*>(otile + r * kOutDw) + col * C;
#pragma unroll
                    for (int c = 0; c < C; ++c) ob[c] = col < ncol ? (uint8_t)to_byte(acc[q][c]) : (uint8_t)0;
                }
            }
        }
        __syncthreads();
        for (int i = tid; i < rn * kOutDw; i += kBlock) {
            const int rr = i / kOutDw, d = i - rr * kOutDw;
            if (d < out_dw) reinterpret_cast<uint32_t*>(mid_rows + (size_t)(c0 + rr) * a.pitch)[d] = otile[i];
        }
        // (the next chunk's staging writes `tile`, which nobody reads after the barrier above; `otile` is rewritten only after
        // the next barrier)
    }
}

struct VArgs {
    const uint8_t* in;       // (n, hin, pitch)
    uint8_t* out;            // (n, hout, wout * C)
    float* out_float;        // (n, C, hout, wout) or NULL
    const int32_t* bounds;   // NULL: hout == hin, a copy
    const int32_t* coeffs;
    int hin, hout, wout, ksize;
    size_t pitch;
};

template <int C, bool DWORD_IN>
__global__ void __launch_bounds__(kBlock) resample_v_kernel(const VArgs a) {
    const int y = blockIdx.y;
    const size_t img = blockIdx.z;
    const int RB = a.wout * C;
    const int b0 = 4 * (int)(blockIdx.x * kBlock + threadIdx.x);
    if (b0 >= RB) return;
    int ymin = y, cnt = 1;
    const int32_t* kc = nullptr;
    if (a.bounds) {                                     // uniform: the same row for the whole workgroup
        ymin = min(max(a.bounds[2 * y], 0), a.hin - 1);
        cnt = min(max(a.bounds[2 * y + 1], 0), min(a.ksize, a.hin - ymin));
        kc = a.coeffs + (size_t)y * a.ksize;
    }
    const uint8_t* p = a.in + (img * a.hin + ymin) * a.pitch + b0;
    int acc[4] = {kHalf, kHalf, kHalf, kHalf};
    for (int t = 0; t < cnt; ++t) {
        const int k = kc ? kc[t] : kOne;
        uint32_t v;
        if (DWORD_IN) {
            v = *reinterpret_cast<const uint32_t*>(p);
        } else {
            v = p[0];
#pragma unroll
            for (int i = 1; i < 4; ++i)
                if (b0 + i < RB) v |= (uint32_t)p[i] << (8 * i);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[i] += (int)((v >> (8 * i)) & 255u) * k;
        p += a.pitch;
    }
    uint32_t o[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) o[i] = to_byte(acc[i]);
    uint8_t* q = a.out + (img * a.hout + y) * (size_t)RB + b0;
    if ((reinterpret_cast<uintptr_t>(q) & 3) == 0 && b0 + 4 <= RB) {
        *reinterpret_cast<uint32_t*>(q) = o[0] | (o[1] << 8) | (o[2] << 16) | (o[3] << 24);
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (b0 + i < RB) q[i] = (uint8_t)o[i];
    }
    if (a.out_float) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int j = b0 + i;
            if (j < RB) {
                const int x = j / C, c = j - x * C;
                a.out_float[((img * C + c) * a.hout + y) * (size_t)a.wout + x] = __fdiv_rn((float)o[i], 255.0f);
            }
        }
    }
}

bool size_ok(int32_t v) { return v >= 1 && v <= SCG_RESAMPLE_MAX_SIZE; }

}  // namespace
}  // namespace scg

using namespace scg;

extern "C" {

const char* scg_img_last_error(void) { return g_err.text; }
int32_t scg_img_abi_version(void) { return SCG_IMG_ABI_VERSION; }

size_t scg_resample_pitch(int32_t wout, int32_t channels) {
    if (!size_ok(wout) || (channels != 1 && channels != 3)) return 0;
    return pitch_of(wout, channels);
}

size_t scg_resample_mid_bytes(int32_t n, int32_t hin, int32_t win, int32_t channels, int32_t wout) {
    if (!size_ok(n) || !size_ok(hin) || !size_ok(win) || !size_ok(wout) || (channels != 1 && channels != 3)) return 0;
    return win == wout ? 0 : (size_t)n * hin * pitch_of(wout, channels);
}

int scg_resample_u8(const uint8_t* src, int32_t n, int32_t hin, int32_t win, int32_t channels, int32_t hout, int32_t wout,
                    const int32_t* hbounds, const int32_t* hcoeffs, int32_t hksize,
                    const int32_t* vbounds, const int32_t* vcoeffs, int32_t vksize,
                    void* mid, size_t mid_bytes, uint8_t* out, size_t out_bytes, float* out_float, size_t out_float_bytes,
                    void* stream) {
    const char* who = "scg_resample_u8";
    if (!src || !out) return g_err.fail(SCG_E_NULL, "%s: %s is NULL", who, src ? "out" : "src");
    if (!size_ok(n) || !size_ok(hin) || !size_ok(win) || !size_ok(hout) || !size_ok(wout))
        return g_err.fail(SCG_E_RANGE, "%s: %d images of %d x %d to %d x %d: every size must be 1..%d", who, n, win, hin, wout, hout,
                    SCG_RESAMPLE_MAX_SIZE);
    if (channels != 1 && channels != 3) return g_err.fail(SCG_E_RANGE, "%s: %d channels, not 1 or 3", who, channels);
    const bool horizontal = wout != win, vertical = hout != hin;
    if (horizontal) {
        if (!hbounds || !hcoeffs) return g_err.fail(SCG_E_NULL, "%s: the width changes and its tables are NULL", who);
        if (hksize < 1 || hksize > SCG_RESAMPLE_MAX_KSIZE)
            return g_err.fail(SCG_E_RANGE, "%s: hksize %d is outside 1..%d", who, hksize, SCG_RESAMPLE_MAX_KSIZE);
    }
    if (vertical) {
        if (!vbounds || !vcoeffs) return g_err.fail(SCG_E_NULL, "%s: the height changes and its tables are NULL", who);
        if (vksize < 1 || vksize > SCG_RESAMPLE_MAX_KSIZE)
            return g_err.fail(SCG_E_RANGE, "%s: vksize %d is outside 1..%d", who, vksize, SCG_RESAMPLE_MAX_KSIZE);
    }
    const size_t pitch = pitch_of(wout, channels);
    if (horizontal) {
        const size_t need = (size_t)n * hin * pitch;
        if (!mid) return g_err.fail(SCG_E_NULL, "%s: the width changes and mid is NULL", who);
        if (mid_bytes < need) return g_err.fail(SCG_E_SCRATCH, "%s: mid of %zu bytes < %zu", who, mid_bytes, need);
        if (reinterpret_cast<uintptr_t>(mid) % kPitchAlign) return g_err.fail(SCG_E_ALIGN, "%s: mid not %d-byte aligned", who, kPitchAlign);
    }
    const size_t out_need = (size_t)n * hout * wout * channels;
    if (out_bytes < out_need) return g_err.fail(SCG_E_SCRATCH, "%s: out of %zu bytes < %zu", who, out_bytes, out_need);
    if (out_float) {
        if (out_float_bytes < out_need * 4)
            return g_err.fail(SCG_E_SCRATCH, "%s: out_float of %zu bytes < %zu", who, out_float_bytes, out_need * 4);
        if (reinterpret_cast<uintptr_t>(out_float) % 4) return g_err.fail(SCG_E_ALIGN, "%s: out_float not 4-byte aligned", who);
    }
    hipStream_t st = static_cast<hipStream_t>(stream);

    if (horizontal) {
        HArgs h;
        h.src = src;
        h.mid = static_cast<uint8_t*>(mid);
        h.bounds = hbounds;
        h.coeffs = hcoeffs;
        h.hin = hin;
        h.win = win;
        h.wout = wout;
        h.ksize = hksize;
        h.pitch = (int)pitch;
        // the widest source span of a strip: the first windows of its columns lie within (kStrip - 1) * scale + 1 of each other
        // and a window holds at most ksize samples; 3 more bytes for the phase of the row, a dword to round up
        const double scale = (double)win / (double)wout;
        const long span_px = (long)((kStrip - 1) * scale) + 2 + hksize;
        h.lp = (int)((span_px * channels + 3 + 3) / 4 + 1);
        const size_t fixed = ((size_t)kStrip * hksize + 2 * kStrip) * 4;
        const size_t per_row = ((size_t)h.lp + kStrip * channels / 4) * 4;
        size_t rt = fixed < kLdsBudget ? (kLdsBudget - fixed) / per_row : 0;
        constexpr size_t kFull = kRowSubs * kRowsPerLane;        // rows one sweep of the lanes covers with every lane busy
        rt = rt >= kFull ? rt / kFull * kFull : rt / kRowSubs * kRowSubs;
        if (rt < (size_t)kRowSubs) rt = kRowSubs;
        if (rt > (size_t)kStripRows) rt = kStripRows;
        h.rt = (int)rt;
        const size_t lds = fixed + rt * per_row;
        if (lds > 64 * 1024) return g_err.fail(SCG_E_RANGE, "%s: a strip of %d -> %d needs %zu bytes of LDS", who, win, wout, lds);
        const dim3 grid((unsigned)((wout + kStrip - 1) / kStrip), (unsigned)((hin + kStripRows - 1) / kStripRows), (unsigned)n);
        if (channels == 3) hipLaunchKernelGGL(resample_h_kernel<3>, grid, dim3(kBlock), lds, st, h);
        else hipLaunchKernelGGL(resample_h_kernel<1>, grid, dim3(kBlock), lds, st, h);
        if (int rc = g_err.check_hip(hipGetLastError(), who)) return rc;
    }

    VArgs v;
    v.in = horizontal ? static_cast<const uint8_t*>(mid) : src;
    v.out = out;
    v.out_float = out_float;
    v.bounds = vertical ? vbounds : nullptr;
    v.coeffs = vertical ? vcoeffs : nullptr;
    v.hin = hin;
    v.hout = hout;
    v.wout = wout;
    v.ksize = vertical ? vksize : 1;
    v.pitch = horizontal ? pitch : (size_t)win * channels;
    const bool dword_in = v.pitch % 4 == 0 && reinterpret_cast<uintptr_t>(v.in) % 4 == 0;
    const int row_bytes = wout * channels;
    const dim3 grid((unsigned)((row_bytes + kVTile - 1) / kVTile), (unsigned)hout, (unsigned)n);
    if (channels == 3) {
        if (dword_in) hipLaunchKernelGGL((resample_v_kernel<3, true>), grid, dim3(kBlock), 0, st, v);
        else hipLaunchKernelGGL((resample_v_kernel<3, false>), grid, dim3(kBlock), 0, st, v);
    } else {
        if (dword_in) hipLaunchKernelGGL((resample_v_kernel<1, true>), grid, dim3(kBlock), 0, st, v);
        else hipLaunchKernelGGL((resample_v_kernel<1, false>), grid, dim3(kBlock), 0, st, v);
    }
    return g_err.check_hip(hipGetLastError(), who);
}

}  // extern "C"

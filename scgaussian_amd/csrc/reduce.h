// reduce.h — the fixed-order workgroup reduction of the image-side kernels (loss.hip, dtumask.hip, evalview.hip, depthviz.hip).
// The order contract, stated once: within a wave a __shfl_down tree over the offsets 32, 16, 8, 4, 2, 1 in that order; then the
// waves' values folded left to right in wave order, starting from wave 0's: ((w0 op w1) op w2) op ...  No float atomics anywhere.
// The "bitwise reproducible" claims in those files' headers rest on exactly this and on nothing else.
// (geometry.hip, binning.hip and blend.hip take their integer wave trees from here as well.  matchloss.hip keeps a written-out copy
// of the same tree, folded from a literal 0.f: see the note at its site.)
#pragma once

#include "scg_common.h"

namespace scg {

// torch.min / torch.max: a NaN on either side wins
__device__ __forceinline__ float nan_min(float a, float b) { return a != a ? a : (b != b ? b : (b < a ? b : a)); }
__device__ __forceinline__ float nan_max(float a, float b) { return a != a ? a : (b != b ? b : (b > a ? b : a)); }

struct Sum { template <typename T> __device__ __forceinline__ T operator()(T a, T b) const { return a + b; } };
struct Max { __device__ __forceinline__ uint32_t operator()(uint32_t a, uint32_t b) const { return max(a, b); } };
struct NanMin { __device__ __forceinline__ float operator()(float a, float b) const { return nan_min(a, b); } };
struct NanMax { __device__ __forceinline__ float operator()(float a, float b) const { return nan_max(a, b); } };

// the tree; the result is valid in lane 0
template <typename T, typename Op>
__device__ __forceinline__ T wave_reduce(T v, Op op) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = op(v, (T)__shfl_down(v, off, kWave));
    return v;
}

// The fold over the words the NW waves left in s_red, behind the barrier that follows their stores.
template <int NW, typename T, typename Op>
__device__ __forceinline__ T wg_fold(const T* s_red, Op op) {
    T t = s_red[0];
#pragma unroll
    for (int k = 1; k < NW; ++k) t = op(t, s_red[k]);
    return t;
}

// Tree, lane 0's word, barrier, fold: every thread of the workgroup of NW waves calls it, every thread gets the result.  A second
// barrier ends it, so s_red (NW words) may be written again straight after the call.
template <int NW, typename T, typename Op>
__device__ __forceinline__ T wg_reduce(T v, T* s_red, Op op) {
    v = wave_reduce(v, op);
    if (lane_id() == 0) s_red[wave_id()] = v;
    __syncthreads();
    const T t = wg_fold<NW>(s_red, op);
    __syncthreads();
    return t;
}

// The first half for TWO values that share one barrier (min and max, numerator and denominator): both trees in one loop, lane 0's
// two words.  The caller's __syncthreads() and its wg_fold of each array follow, on every thread or on thread 0 alone.
template <typename T, typename OpA, typename OpB>
__device__ __forceinline__ void wave_publish(T a, T b, T* s_a, T* s_b, OpA op_a, OpB op_b) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { a = op_a(a, (T)__shfl_down(a, off, kWave)); b = op_b(b, (T)__shfl_down(b, off, kWave)); }
    if (lane_id() == 0) { s_a[wave_id()] = a; s_b[wave_id()] = b; }
}

}  // namespace scg

// compact.h — the integer steps of a stable stream compaction "classify / count per workgroup / one-workgroup scan / scatter at
// base + rank" (densify.hip, seed.hip).  K counters ride together: flag k of a thread is bit k of `flags`, the counts of workgroup g
// are counts[g * K .. g * K + K).  No atomics, a fixed order: the same input gives the same bits.
#pragma once

#include "scg_common.h"

namespace scg {

// tot[k]: the threads of the workgroup that set flag k; rank[k]: those of them in front of this thread, in thread order.  Ballot +
// popcount per wave, the waves' counts through K words of LDS each.  Every thread of the workgroup calls it, once per kernel; it
// holds one barrier, so what the workgroup wrote to LDS before the call is visible after it.
template <int K, int kThreads>
__device__ __forceinline__ void block_counts(uint32_t flags, uint32_t rank[K], uint32_t tot[K]) {
    constexpr int kWaves = kThreads / kWave;
    __shared__ uint32_t s_w[kWaves][K];
    const int lane = lane_id(), w = wave_id();
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const unsigned long long b = __ballot((flags >> k) & 1u);
        rank[k] = (uint32_t)__popcll(b & ((1ull << lane) - 1ull));
        if (lane == 0) s_w[w][k] = (uint32_t)__popcll(b);
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k) {
        uint32_t before = 0, all = 0;
        for (int j = 0; j < kWaves; ++j) {
            const uint32_t u = s_w[j][k];
            if (j < w) before += u;
            all += u;
        }
        rank[k] += before;
        tot[k] = all;
    }
}

// The carry scan: counts (groups x K) become exclusive bases in place, in workgroup order, and total[k] the sum of column k.  Every
// thread of ONE workgroup calls it; the workgroup walks the groups kThreads at a time and carries the sums along.
template <int K, int kThreads>
__device__ __forceinline__ void carry_scan(uint32_t* counts, int groups, uint32_t total[K]) {
    constexpr int kWaves = kThreads / kWave;
    __shared__ uint32_t s_w[kWaves][K];
    const int lane = lane_id(), w = wave_id();
#pragma unroll
    for (int k = 0; k < K; ++k) total[k] = 0;
    for (int base = 0; base < groups; base += kThreads) {
        const int g = base + (int)threadIdx.x;
        uint32_t v[K], inc[K];
#pragma unroll
        for (int k = 0; k < K; ++k) {
            v[k] = g < groups ? counts[(int64_t)g * K + k] : 0u;
            uint32_t x = v[k];
            for (int off = 1; off < kWave; off <<= 1) {
                const uint32_t y = (uint32_t)__shfl_up((int)x, off, kWave);
                if (lane >= off) x += y;
            }
            inc[k] = x;
            if (lane == kWave - 1) s_w[w][k] = x;
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < K; ++k) {
            uint32_t before = 0, all = 0;
            for (int j = 0; j < kWaves; ++j) {
                const uint32_t u = s_w[j][k];
                if (j < w) before += u;
                all += u;
            }
            if (g < groups) counts[(int64_t)g * K + k] = total[k] + before + inc[k] - v[k];
            total[k] += all;
        }
        __syncthreads();
    }
}

}  // namespace scg

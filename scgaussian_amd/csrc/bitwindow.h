// bitwindow.h — what the two file packers (pngpack.hip, jpegpack.hip) share on the device: every thread of a workgroup forms a run of
// code words, an exclusive scan of the threads' bit counts says where each run begins, and the bits are ORed into a zeroed window of
// the stream in LDS.  Integer arithmetic only, a fixed order: the same input gives the same bits.
#pragma once

#include "scg_common.h"

namespace scg {

// The workgroup-exclusive sum of one word per thread: `before` the sum of v over the threads in front of this one, `total` over all.
// A __shfl_up ladder inside the wave, the wave's sum through s_waves (kThreads / kWave words of LDS, the CALLER'S: two scans over
// distinct arrays need no barrier between them), ONE barrier behind the store, then every thread walks the waves' words.  Every
// thread of the workgroup calls it; s_waves is free again behind the workgroup's next barrier.
template <int kThreads>
__device__ __forceinline__ void block_exclusive_sum(uint32_t v, uint32_t* s_waves, uint32_t& before, uint32_t& total) {
    const int lane = lane_id(), w = wave_id();
    uint32_t inc = v;
    for (int o = 1; o < kWave; o <<= 1) {
        const uint32_t y = (uint32_t)__shfl_up((int)inc, o, kWave);
        if (lane >= o) inc += y;
    }
    if (lane == kWave - 1) s_waves[w] = inc;
    __syncthreads();
    before = total = 0u;
    for (int j = 0; j < kThreads / kWave; ++j) {
        if (j < w) before += s_waves[j];
        total += s_waves[j];
    }
    before += inc - v;
}

// 64 bits of the stream that begin at its word w, `first` in word w and `second` in word w + 1, ORed into the LDS window `win` that
// holds the words [wlo, whi): a half outside the window is dropped, so a code word that straddles two windows lands in both when it
// is put once per window.  The bit order inside a word is the caller's (PNG: first bit lowest; JPEG: first bit highest).
__device__ __forceinline__ void window_or(uint32_t* win, uint32_t wlo, uint32_t whi, uint32_t w, uint32_t first, uint32_t second) {
    if (first && w >= wlo && w < whi) atomicOr(&win[w - wlo], first);
    if (second && w + 1u >= wlo && w + 1u < whi) atomicOr(&win[w + 1u - wlo], second);
}

}  // namespace scg

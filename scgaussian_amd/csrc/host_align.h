// host_align.h — the host code's rounding of sizes and its pointer alignment tests.
#pragma once

#include <stddef.h>
#include <stdint.h>

namespace scg {

inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }            // any a > 0

template <uint64_t N>
inline uint64_t align_to(uint64_t v) {                                                // N a power of two
    static_assert(N && !(N & (N - 1)), "a power of two");
    return (v + (N - 1)) & ~(N - 1);
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
inline bool aligned64(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 63u) == 0; }

}  // namespace scg

// probe_timeline.h — the per-wave timeline probe: in the probe build (build.py build_probe_timeline_variant) every wave of the
// geometry, scatter, forward-blend and blend-backward kernels reads the 100 MHz wall clock at the boundaries of its phases
// and logs them behind the n_tiles cost words of ScgFrame.tile_cost_out; tools/probes/*_timeline.py read the log
// (tools/probes/_timeline_log.py holds the same layout, tests/test_probe_timeline_cpu.py holds the two together).
// The only file that tests the build's macro: in the product build SCG_PROBE(...) and SCG_TP(k) expand to nothing and GeoProbe
// is empty — the product's device code does not know the probe exists.
#pragma once

#include "scg_common.h"

namespace scg {

// ---- the log, in 32-bit words behind tile_cost_out[n_tiles]: four regions of fixed-size records, one record per wave -------
constexpr int kTlScatterRecord = 8;             // words of a record of tile_scatter_kernel
constexpr int kTlGeometryRecord = 8;            // ... of geometry_hist_kernel
constexpr int kTlBlendRecord = 8;               // ... of tile_blend_forward_kernel, and of the sort's second record per workgroup
constexpr int kTlBackwardRecord = 4;            // ... of blend_backward_kernel
constexpr int kTlScatterAt = 0;                 // the scatter region: 8 224 records
constexpr int kTlGeometryAt = 65792;            // the geometry region: 4 096 records
constexpr int kTlBlendAt = 65792 + 32768;       // the forward-blend region: four quadrant waves + the sort's record per tile
constexpr int kTlTilePad = 8;                   // the per-tile regions are sized for n_tiles + 8 (>= the launch order's slots)
constexpr int kTlBlendWordsPerTile = 40;
constexpr int kTlBackwardWordsPerTile = 16;     // the backward region: four quadrant waves per tile
constexpr int kTlTailWords = 64;
// the last word of a record says who wrote it (a log is only as long as the caller made it: the scripts keep what is signed)
constexpr uint32_t kTlSigScatter = 0xC0FFEEu;
constexpr uint32_t kTlSigGeometry = 0xC0FFEE00u;     // | chunks the wave took (low 8 bits)
constexpr uint32_t kTlSigBlend = 0xB1E9D000u;
constexpr uint32_t kTlSigSort = 0x50B70000u;
constexpr uint32_t kTlSigBackward = 0xBAC00000u;     // | 4 tile + quadrant

// A wave's record: record `index` of a region of the log behind cost_out[n_tiles] (scatter, geometry: workgroup * waves +
// wave; blend: workgroup * 4 + quadrant, the sort's second record at SCG_TL_SORT_INDEX; backward: workgroup).  Expressions, not
// functions: the probe build's address arithmetic then stands in the kernel's own block, where the compiler has always seen it.
#define SCG_TL_SCATTER_RECORD(cost_out, n_tiles, index) ((cost_out) + (n_tiles) + scg::kTlScatterAt + (index) * scg::kTlScatterRecord)
#define SCG_TL_GEOMETRY_RECORD(cost_out, n_tiles, index) ((cost_out) + (n_tiles) + scg::kTlGeometryAt + (index) * scg::kTlGeometryRecord)
#define SCG_TL_BLEND_RECORD(cost_out, n_tiles, index) ((cost_out) + (n_tiles) + scg::kTlBlendAt + (index) * scg::kTlBlendRecord)
#define SCG_TL_BACKWARD_RECORD(cost_out, n_tiles, index) ((cost_out) + (n_tiles) + scg::kTlBlendAt + (size_t)((n_tiles) + scg::kTlTilePad) * scg::kTlBlendWordsPerTile + (index) * scg::kTlBackwardRecord)
#define SCG_TL_SORT_INDEX(n_tiles, workgroup) ((size_t)scg::tile_order_slots(n_tiles) * 4 + (workgroup))
// words of the whole log (what a caller allocates behind the n_tiles cost words for every probe of the build to have its region)
#define SCG_TL_LOG_WORDS(n_tiles) (scg::kTlBlendAt + (size_t)((n_tiles) + scg::kTlTilePad) * scg::kTlBlendWordsPerTile + (size_t)((n_tiles) + scg::kTlTilePad) * scg::kTlBackwardWordsPerTile + scg::kTlTailWords)

#if defined(__HIPCC__)
// ---- what the kernels write the probe with --------------------------------------------------------------------------
// SCG_PROBE(statements or members): compiled in the probe build, nothing in the product build.  kProbeTimeline: the same as
// a value.  SCG_TP(k) (tile_sort.h sort_tile_bucket): clock k of a tile's sort, kept in the sort's LDS (TileSortLds::probe).
// GeoProbe: what geometry_forward_one is handed by its two callers, in both builds — the wave's phase clocks (tools/probes/
// geometry_timeline.py): [0..3] time in the cull / covariance chain | in `between` | waiting for the SH record | in the rest of
// the chunk, summed over the wave's chunks; [4] the last clock read.  Empty in the product build: the parameter vanishes.
#ifdef SCG_PROBE_TIMELINE
#define SCG_PROBE(...) __VA_ARGS__
constexpr bool kProbeTimeline = true;
typedef uint32_t GeoProbe[5];
#else
#define SCG_PROBE(...)
constexpr bool kProbeTimeline = false;
struct GeoProbe {};
#endif
#define SCG_TP(k) SCG_PROBE(if (threadIdx.x == 0) L.probe[k] = scg::probe_clock();)

__device__ __forceinline__ uint32_t probe_clock() { return (uint32_t)wall_clock64(); }      // s_memrealtime, 100 MHz

#endif  // __HIPCC__

}  // namespace scg

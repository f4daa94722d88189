// matchpoint.hip — libscg_mp.so: the init stage's snapshot packed on the GPU (include/mp/scg_matchpoint.h).
//
// GaussianModel.save_ply_at_matchpoint (scene/gaussian_model.py:611-642) loops over the ordered view pairs in Python: per pair an
// index_put into the view's image, per view two synchronising copies and a min / max, at the end two concatenations and a tuple
// per match.  Every match is decided from that match alone and every pixel from its winning match and two scalars of its view, so
// here it is four launches whatever the number of views and pairs, into ONE buffer the caller copies to the host once:
//
//   mp_clear_kernel     the winner map (one int32 per pixel of all views) to -1; workgroup 0 also zeroes the gaps between the
//                       buffer's regions
//   mp_matches_kernel   one thread per match, a workgroup per kGroup = 256 consecutive matches of the arena = four record tiles,
//                       so that a workgroup's part of the body begins on a dword.  xyz and the colour bytes go to LDS, a row per
//                       lane (stride 5 dwords: odd, so the lanes of a half wave fall on distinct banks), and leave as the file's
//                       bytes in lane-contiguous dwords, the last one padded with zeros.  A match with a finite uv puts its arena
//                       index into its view's winner map with an integer atomicMax: the latest in arena order wins, whatever
//                       order the threads run in.  A workgroup that lies inside one segment (all but those at a segment's ends)
//                       reads that segment's view record once, through scalar loads; in the others a match finds its segment in
//                       the LDS copy of the table (csrc/seed.hip).  Why not a workgroup per segment slice: a slice begins at any
//                       byte phase of the body, so its first and last dwords would be shared with its neighbours, and 42
//                       segments of three matches would be 42 workgroups.
//   mp_resolve_kernel   one thread per pixel, a workgroup inside one view (found from blockIdx.x alone: scalar loads): the depth
//                       plane from the winner map, and the workgroup's (min, max) in the fixed order of reduce.h
//   mp_quantise_kernel  a workgroup inside one view: it folds the view's partials itself, then four pixels per thread: normalise,
//                       quantise (pixel_rules.h), one dword; the view's first workgroup writes (min, max)
//
// No float atomics, no host read, no allocation.  Min and max are exact in any order once zeros are ordered by sign and a NaN wins
// (ordered_min / ordered_max below).  Compiled with -ffp-contract=off: the position is a product and a sum.
#include "../../include/mp/scg_matchpoint.h"
#include "host_align.h"
#include "host_error.h"
#include "pixel_rules.h"
#include "reduce.h"

#pragma clang fp contract(off)

namespace scg {
namespace {

constexpr int kGroup = SCG_MP_MATCH_GROUP;
constexpr int kRec = SCG_MP_RECORD_BYTES;
constexpr int kRow = 5;                                  // LDS dwords of a staged match: x y z rgb, and one to make the stride odd
constexpr int kMaxClearGroups = 1024;
static_assert(kGroup == kBlock && kGroup % SCG_MP_TILE_RECORDS == 0 && (SCG_MP_TILE_RECORDS * kRec) % 4 == 0,
              "a workgroup's records are whole tiles and a tile is a whole number of dwords");
static_assert(SCG_MP_RESOLVE_PIXELS == kBlock && SCG_MP_QUANT_PIXELS == 4 * kBlock, "one and four pixels per thread");

thread_local ErrorText g_err = {};

// The layout and the view table from the sizes; who == nullptr: no message.  Host only.
int layout_of(const char* who, int64_t N, int64_t V, const int32_t* hw, ScgMpLayout* l, ScgMpView* views) {
    if (N < 0 || N > SCG_MP_MAX_MATCHES) return who ? g_err.fail(SCG_E_RANGE, "%s: N = %lld is outside 0..2^31 - 1", who, (long long)N) : SCG_E_RANGE;
    if (V < 1 || V > SCG_MP_MAX_VIEWS) return who ? g_err.fail(SCG_E_RANGE, "%s: V = %lld is outside 1..%d", who, (long long)V, SCG_MP_MAX_VIEWS) : SCG_E_RANGE;
    if (!hw) return who ? g_err.fail(SCG_E_NULL, "%s: hw is NULL", who) : SCG_E_NULL;
    uint64_t pixels = 0, bytes = 0, rg = 0, qg = 0;
    for (int64_t v = 0; v < V; ++v) {
        const int32_t H = hw[2 * v], W = hw[2 * v + 1];
        if (H < 1 || W < 1 || H > SCG_MP_MAX_DIM || W > SCG_MP_MAX_DIM)
            return who ? g_err.fail(SCG_E_RANGE, "%s: view %lld of %d x %d pixels (H, W must be 1..%d)", who, (long long)v, W, H, SCG_MP_MAX_DIM)
                       : SCG_E_RANGE;
        const uint64_t n = (uint64_t)H * (uint64_t)W;
        if (bytes + align_to<4>(n) > SCG_MP_MAX_PIXELS)
            return who ? g_err.fail(SCG_E_RANGE, "%s: the views hold more than 2^31 - 1 pixels", who) : SCG_E_RANGE;
        if (views) {
            views[v].H = H;
            views[v].W = W;
            views[v].first_pixel = (int32_t)pixels;
            views[v].first_byte = (int32_t)bytes;
            views[v].resolve_group = (int32_t)rg;
            views[v].quant_group = (int32_t)qg;
        }
        pixels += n;
        bytes += align_to<4>(n);
        rg += (n + SCG_MP_RESOLVE_PIXELS - 1) / SCG_MP_RESOLVE_PIXELS;
        qg += (n + SCG_MP_QUANT_PIXELS - 1) / SCG_MP_QUANT_PIXELS;
    }
    l->body_offset = 0;
    l->body_bytes = align_to<4>((uint64_t)N * kRec);
    l->depth_offset = align_to<256>(l->body_offset + l->body_bytes);
    l->depth_bytes = pixels * 4;
    l->byte_offset = align_to<256>(l->depth_offset + l->depth_bytes);
    l->byte_bytes = bytes;
    l->range_offset = align_to<256>(l->byte_offset + l->byte_bytes);
    l->range_bytes = (uint64_t)V * 8;
    l->total = align_to<256>(l->range_offset + l->range_bytes);
    l->pixels = pixels;
    l->resolve_groups = rg;
    l->quant_groups = qg;
    return 0;
}

size_t workspace_of(const ScgMpLayout& l) { return (size_t)(l.pixels * 4 + l.resolve_groups * 8); }

// ---- device side ---------------------------------------------------------------------------------------------------------------
struct MpArgs {
    int N, V, nseg;
    int pixels, byte_total, resolve_groups;
    const ScgSeedSegment* seg;
    const ScgMpView* views;
    const float* rays_o;
    const float* rays_d;
    const float* z;
    const float* color;
    const float* uv;
    const float* cam_z;
    uint32_t* body;
    float* depth;
    uint32_t* bytes;            // the byte planes, as dwords
    float* ranges;
    int32_t* winner;
    float* partial;             // (min, max) per workgroup of the resolve kernel
    uint32_t* gap[4];           // the gaps behind the four regions ...
    int gap_dw[4];              // ... and their dwords (each < 64)
};

// the byte numpy's array cast float32 -> uint8 gives on x86-64 (include/io/scg_ply.h; csrc/plypack.hip states the same rule)
__device__ __forceinline__ uint32_t color_byte(float v) {
    if (!(fabsf(v) < 2147483648.0f)) return 0u;
    return (uint32_t)(int32_t)v & 255u;
}

// min / max with a NaN winning (torch.min / torch.max) and -0.0 below +0.0: associative and commutative, so any order gives one result
__device__ __forceinline__ bool below(float a, float b) { return a < b || (a == b && signbit(a) && !signbit(b)); }
__device__ __forceinline__ float ordered_min(float a, float b) { return a != a ? a : (b != b ? b : (below(b, a) ? b : a)); }
__device__ __forceinline__ float ordered_max(float a, float b) { return a != a ? a : (b != b ? b : (below(a, b) ? b : a)); }
struct OrderedMin { __device__ __forceinline__ float operator()(float a, float b) const { return ordered_min(a, b); } };
struct OrderedMax { __device__ __forceinline__ float operator()(float a, float b) const { return ordered_max(a, b); } };

__global__ __launch_bounds__(kBlock) void mp_clear_kernel(MpArgs a) {
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x; p < a.pixels; p += stride) a.winner[p] = -1;
    if (blockIdx.x == 0) {
        const int g = threadIdx.x >> 6, k = threadIdx.x & 63;            // a wave per gap
        if (k < a.gap_dw[g]) a.gap[g][k] = 0u;
    }
}

// the segment of match i: the last one whose offset is <= i (the table is sorted and tiles [0, N); empty segments are never chosen
// in front of the one that follows them)
__device__ __forceinline__ int segment_of(const int32_t* s_off, int nseg, int64_t i) {
    int lo = 0, hi = nseg - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (s_off[mid] <= i) lo = mid; else hi = mid - 1;
    }
    return lo;
}

__global__ __launch_bounds__(kBlock) void mp_matches_kernel(MpArgs a) {
    __shared__ int32_t s_off[SCG_MP_MAX_SEGMENTS];
    __shared__ int32_t s_view[SCG_MP_MAX_SEGMENTS];
    __shared__ uint32_t tile[kGroup * kRow];
    const int tid = threadIdx.x;
    for (int s = tid; s < a.nseg; s += kBlock) {
        s_off[s] = a.seg[s].offset;
        s_view[s] = a.seg[s].view;
    }
    const int64_t first = (int64_t)blockIdx.x * kGroup;
    const int64_t i = first + tid;
    const int n = (int)min((int64_t)kGroup, (int64_t)a.N - first);
    if (tid < n) {
        const float z = a.z[i];
        uint32_t* row = tile + tid * kRow;
        uint32_t rgb = 0u;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float prod = a.rays_d[i * 3 + c] * z;
            row[c] = __float_as_uint(a.rays_o[i * 3 + c] + prod);
            rgb |= color_byte(a.color[i * 3 + c] * 255.0f) << (8 * c);
        }
        row[3] = rgb;
    }
    __syncthreads();
    // Where the workgroup's first and last match lie in one segment (all but the workgroups at a segment's ends, at 2 000 matches
    // per pair) the view is the workgroup's: one record, one address, scalar loads.  Elsewhere every match looks its segment up.
    const int s_first = segment_of(s_off, a.nseg, first), s_last = segment_of(s_off, a.nseg, first + n - 1);
    const bool one = s_first == s_last;
    const int uview = __builtin_amdgcn_readfirstlane(s_view[s_first]);
    ScgMpView uw = {};
    if (one && uview >= 0 && uview < a.V) uw = a.views[uview];
    if (tid < n) {
        const float u = a.uv[i * 2], v = a.uv[i * 2 + 1];
        if (isfinite(u) && isfinite(v)) {
            const int view = one ? uview : s_view[segment_of(s_off, a.nseg, i)];
            if (view >= 0 && view < a.V) {
                const ScgMpView w = one ? uw : a.views[view];
                if (w.H >= 1 && w.W >= 1 && w.H <= SCG_MP_MAX_DIM && w.W <= SCG_MP_MAX_DIM) {
                    const int64_t r = (int64_t)fminf(fmaxf(v, 0.0f), (float)(w.H - 1));      // clamp on the float, then truncate
                    const int64_t c = (int64_t)fminf(fmaxf(u, 0.0f), (float)(w.W - 1));
                    const int64_t p = (int64_t)w.first_pixel + r * w.W + c;
                    if (r >= 0 && r < w.H && c >= 0 && c < w.W && p >= 0 && p < a.pixels) atomicMax(&a.winner[p], (int32_t)i);
                }
            }
        }
    }
    // the workgroup's records as the file holds them: dword d of its part gathers bytes 4 d .. 4 d + 3
    const int nbytes = n * kRec, ndw = (nbytes + 3) >> 2;
    uint32_t* dst = a.body + (size_t)blockIdx.x * (kGroup * kRec / 4);
    for (int d = tid; d < ndw; d += kBlock) {
        uint32_t word = 0u;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int at = 4 * d + b;
            if (at < nbytes) {
                const int r = at / kRec, o = at - r * kRec;
                uint32_t byte = 0u;
                if (o < 12) byte = (tile[r * kRow + (o >> 2)] >> (8 * (o & 3))) & 255u;
                else if (o >= 24) byte = (tile[r * kRow + 3] >> (8 * (o - 24))) & 255u;
                word |= byte << (8 * b);
            }
        }
        dst[d] = word;
    }
}

// The view whose workgroups hold `g`: the last record whose first group is <= g.  Uniform in the workgroup.  FIELD: 0 the resolve
// kernel's groups, 1 the quantise kernel's.
template <int FIELD>
__device__ __forceinline__ int view_of_group(const ScgMpView* views, int V, int g) {
    int lo = 0, hi = V - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        const int at = FIELD ? views[mid].quant_group : views[mid].resolve_group;
        if (at <= g) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// Is the record one whose planes lie inside the buffers?  (The host validated its own copy; this is the device copy.)
__device__ __forceinline__ bool view_inside(const ScgMpView& w, const MpArgs& a) {
    if (w.H < 1 || w.W < 1 || w.H > SCG_MP_MAX_DIM || w.W > SCG_MP_MAX_DIM) return false;
    const int64_t hw = (int64_t)w.H * w.W;
    return w.first_pixel >= 0 && (int64_t)w.first_pixel + hw <= a.pixels && w.first_byte >= 0 && (w.first_byte & 3) == 0 &&
           (int64_t)w.first_byte + ((hw + 3) & ~(int64_t)3) <= a.byte_total;
}

__global__ __launch_bounds__(kBlock) void mp_resolve_kernel(MpArgs a) {
    __shared__ float s_mn[kBlock / kWave], s_mx[kBlock / kWave];
    const int g = blockIdx.x;
    const ScgMpView w = a.views[view_of_group<0>(a.views, a.V, g)];
    if (!view_inside(w, a) || g < w.resolve_group) return;               // uniform: before any barrier
    const int64_t hw = (int64_t)w.H * w.W;
    const int64_t local = (int64_t)(g - w.resolve_group) * kBlock + threadIdx.x;
    const bool active = local < hw;
    float d = 0.0f;
    if (active) {
        const int64_t p = (int64_t)w.first_pixel + local;
        const int32_t wi = a.winner[p];
        d = (wi >= 0 && wi < a.N) ? a.z[wi] * a.cam_z[wi] : 0.0f;
        a.depth[p] = d;
    }
    wave_publish(active ? d : INFINITY, active ? d : -INFINITY, s_mn, s_mx, OrderedMin(), OrderedMax());
    __syncthreads();
    if (threadIdx.x == 0) {
        a.partial[2 * (int64_t)g] = wg_fold<kBlock / kWave>(s_mn, OrderedMin());
        a.partial[2 * (int64_t)g + 1] = wg_fold<kBlock / kWave>(s_mx, OrderedMax());
    }
}

__global__ __launch_bounds__(kBlock) void mp_quantise_kernel(MpArgs a) {
    __shared__ float s_mn[kBlock / kWave], s_mx[kBlock / kWave];
    const int g = blockIdx.x;
    const int view = view_of_group<1>(a.views, a.V, g);
    const ScgMpView w = a.views[view];
    if (!view_inside(w, a) || g < w.quant_group) return;                 // uniform: before any barrier
    const int64_t hw = (int64_t)w.H * w.W;
    const int64_t parts = (hw + kBlock - 1) / kBlock;
    if (w.resolve_group < 0 || (int64_t)w.resolve_group + parts > a.resolve_groups) return;
    float mn = INFINITY, mx = -INFINITY;
    for (int64_t k = threadIdx.x; k < parts; k += kBlock) {
        mn = ordered_min(mn, a.partial[2 * (w.resolve_group + k)]);
        mx = ordered_max(mx, a.partial[2 * (w.resolve_group + k) + 1]);
    }
    wave_publish(mn, mx, s_mn, s_mx, OrderedMin(), OrderedMax());
    __syncthreads();
    mn = wg_fold<kBlock / kWave>(s_mn, OrderedMin());
    mx = wg_fold<kBlock / kWave>(s_mx, OrderedMax());
    if (g == w.quant_group && threadIdx.x == 0) {
        a.ranges[2 * view] = mn;
        a.ranges[2 * view + 1] = mx;
    }
    const float range = mx - mn;
    const int64_t local = (int64_t)(g - w.quant_group) * SCG_MP_QUANT_PIXELS + 4 * (int64_t)threadIdx.x;
    if (local >= hw) return;
    const float* src = a.depth + w.first_pixel + local;
    uint32_t word = 0u;
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (local + k < hw) word |= quantise(__fdiv_rn(src[k] - mn, range)) << (8 * k);
    a.bytes[((int64_t)w.first_byte + local) >> 2] = word;               // the plane's padding bytes are the zeros of the last word
}

}  // namespace
}  // namespace scg

using namespace scg;

extern "C" {

const char* scg_mp_last_error(void) { return g_err.text; }
int32_t scg_mp_abi_version(void) { return SCG_MP_ABI_VERSION; }

size_t scg_mp_struct_bytes(int32_t which) {
    switch (which) {
        case 0: return sizeof(ScgMpLayout);
        case 1: return sizeof(ScgMpView);
        case 2: return sizeof(ScgMpPack);
        default: return 0;
    }
}

int scg_mp_layout(int32_t N, int32_t V, const int32_t* hw, ScgMpLayout* out, ScgMpView* views_out) {
    if (!out) return g_err.fail(SCG_E_NULL, "scg_mp_layout: out is NULL");
    ScgMpLayout l;
    if (int rc = layout_of("scg_mp_layout", N, V, hw, &l, views_out)) return rc;
    *out = l;
    return 0;
}

size_t scg_mp_workspace_bytes(int32_t V, const int32_t* hw) {
    ScgMpLayout l;
    return layout_of(nullptr, 0, V, hw, &l, nullptr) ? 0 : workspace_of(l);
}

int scg_mp_pack(const ScgMpPack* p, void* buffer, size_t buffer_bytes, void* workspace, size_t workspace_bytes, void* stream) {
    const char* who = "scg_mp_pack";
    if (!p) return g_err.fail(SCG_E_NULL, "%s: args is NULL", who);
    if (p->struct_bytes != (int32_t)sizeof(ScgMpPack))
        return g_err.fail(SCG_E_RANGE, "%s: struct_bytes = %d, the library's ScgMpPack has %zu", who, p->struct_bytes, sizeof(ScgMpPack));
    if (p->N < 1) return g_err.fail(SCG_E_RANGE, "%s: N = %d: a snapshot needs at least one match", who, p->N);
    if (p->V < 1 || p->V > SCG_MP_MAX_VIEWS) return g_err.fail(SCG_E_RANGE, "%s: V = %d is outside 1..%d", who, p->V, SCG_MP_MAX_VIEWS);
    if (p->nseg < 1 || p->nseg > SCG_MP_MAX_SEGMENTS)
        return g_err.fail(SCG_E_RANGE, "%s: nseg = %d is outside 1..%d", who, p->nseg, SCG_MP_MAX_SEGMENTS);
    if (!p->segments || !p->segments_dev) return g_err.fail(SCG_E_NULL, "%s: a segment table is NULL", who);
    if (!p->views || !p->views_dev) return g_err.fail(SCG_E_NULL, "%s: a view table is NULL", who);
    const int N = p->N, V = p->V;
    int64_t at = 0;
    for (int s = 0; s < p->nseg; ++s) {
        const ScgSeedSegment& g = p->segments[s];
        if (g.view < 0 || g.view >= V) return g_err.fail(SCG_E_RANGE, "%s: segment %d has view %d outside [0, %d)", who, s, g.view, V);
        if (g.count < 0 || g.offset < 0) return g_err.fail(SCG_E_RANGE, "%s: segment %d has offset %d, count %d", who, s, g.offset, g.count);
        if (g.offset != at)
            return g_err.fail(SCG_E_RANGE, "%s: segment %d starts at %d, the one before it ends at %lld", who, s, g.offset, (long long)at);
        at += g.count;
        if (at > N) return g_err.fail(SCG_E_RANGE, "%s: segment %d runs past N = %d", who, s, N);
    }
    if (at != N) return g_err.fail(SCG_E_RANGE, "%s: the segments cover %lld of N = %d matches", who, (long long)at, N);
    // the view table: the one the layout gives for its own H and W, record by record
    int32_t hw[2 * SCG_MP_MAX_VIEWS];
    for (int v = 0; v < V; ++v) {
        hw[2 * v] = p->views[v].H;
        hw[2 * v + 1] = p->views[v].W;
    }
    ScgMpLayout l;
    static thread_local ScgMpView want[SCG_MP_MAX_VIEWS];
    if (int rc = layout_of(who, N, V, hw, &l, want)) return rc;
    for (int v = 0; v < V; ++v) {
        const ScgMpView &x = p->views[v], &y = want[v];
        if (x.first_pixel != y.first_pixel || x.first_byte != y.first_byte || x.resolve_group != y.resolve_group ||
            x.quant_group != y.quant_group)
            return g_err.fail(SCG_E_RANGE, "%s: view %d is (pixel %d, byte %d, groups %d, %d), the layout gives (%d, %d, %d, %d)", who, v,
                           x.first_pixel, x.first_byte, x.resolve_group, x.quant_group, y.first_pixel, y.first_byte, y.resolve_group,
                           y.quant_group);
    }
    if (!buffer) return g_err.fail(SCG_E_NULL, "%s: buffer is NULL", who);
    if (buffer_bytes < l.total) return g_err.fail(SCG_E_SCRATCH, "%s: buffer of %zu bytes < %llu", who, buffer_bytes, (unsigned long long)l.total);
    if (reinterpret_cast<uintptr_t>(buffer) % 16) return g_err.fail(SCG_E_ALIGN, "%s: buffer not 16-byte aligned", who);
    if (!workspace) return g_err.fail(SCG_E_NULL, "%s: workspace is NULL", who);
    if (workspace_bytes < workspace_of(l))
        return g_err.fail(SCG_E_SCRATCH, "%s: workspace of %zu bytes < %zu", who, workspace_bytes, workspace_of(l));
    if (reinterpret_cast<uintptr_t>(workspace) % 4) return g_err.fail(SCG_E_ALIGN, "%s: workspace not 4-byte aligned", who);
    if (!p->rays_o || !p->rays_d || !p->z || !p->color || !p->uv || !p->cam_z) return g_err.fail(SCG_E_NULL, "%s: an input tensor is NULL", who);
    for (const float* t : {p->rays_o, p->rays_d, p->z, p->color, p->uv, p->cam_z})
        if (reinterpret_cast<uintptr_t>(t) % 4) return g_err.fail(SCG_E_ALIGN, "%s: an input tensor is not 4-byte aligned", who);

    MpArgs a;
    a.N = N; a.V = V; a.nseg = p->nseg;
    a.pixels = (int)l.pixels; a.byte_total = (int)l.byte_bytes; a.resolve_groups = (int)l.resolve_groups;
    a.seg = p->segments_dev; a.views = p->views_dev;
    a.rays_o = p->rays_o; a.rays_d = p->rays_d; a.z = p->z; a.color = p->color; a.uv = p->uv; a.cam_z = p->cam_z;
    char* base = static_cast<char*>(buffer);
    a.body = reinterpret_cast<uint32_t*>(base + l.body_offset);
    a.depth = reinterpret_cast<float*>(base + l.depth_offset);
    a.bytes = reinterpret_cast<uint32_t*>(base + l.byte_offset);
    a.ranges = reinterpret_cast<float*>(base + l.range_offset);
    a.winner = static_cast<int32_t*>(workspace);
    a.partial = reinterpret_cast<float*>(a.winner + l.pixels);
    const uint64_t ends[4] = {l.body_offset + l.body_bytes, l.depth_offset + l.depth_bytes, l.byte_offset + l.byte_bytes,
                              l.range_offset + l.range_bytes};
    const uint64_t next[4] = {l.depth_offset, l.byte_offset, l.range_offset, l.total};
    for (int k = 0; k < 4; ++k) {
        a.gap[k] = reinterpret_cast<uint32_t*>(base + ends[k]);
        a.gap_dw[k] = (int)((next[k] - ends[k]) / 4);
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    int64_t clear = ((int64_t)l.pixels + 4 * kBlock - 1) / (4 * kBlock);
    clear = clear > kMaxClearGroups ? kMaxClearGroups : (clear < 1 ? 1 : clear);
    hipLaunchKernelGGL(mp_clear_kernel, dim3((unsigned)clear), dim3(kBlock), 0, st, a);
    if (int rc = g_err.check_hip(hipGetLastError(), "mp_clear")) return rc;
    hipLaunchKernelGGL(mp_matches_kernel, dim3((unsigned)(((int64_t)N + kGroup - 1) / kGroup)), dim3(kBlock), 0, st, a);
    if (int rc = g_err.check_hip(hipGetLastError(), "mp_matches")) return rc;
    hipLaunchKernelGGL(mp_resolve_kernel, dim3((unsigned)l.resolve_groups), dim3(kBlock), 0, st, a);
    if (int rc = g_err.check_hip(hipGetLastError(), "mp_resolve")) return rc;
    hipLaunchKernelGGL(mp_quantise_kernel, dim3((unsigned)l.quant_groups), dim3(kBlock), 0, st, a);
    return g_err.check_hip(hipGetLastError(), "mp_quantise");
}

}  // extern "C"

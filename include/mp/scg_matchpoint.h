/* scg_matchpoint.h — C ABI of libscg_mp.so: the init stage's snapshot, GaussianModel.save_ply_at_matchpoint
 * (scene/gaussian_model.py:611-642, called by scene.save_init, train.py:97), packed on the GPU (csrc/matchpoint.hip, gfx950).
 *
 * A fourth library next to libscg_raster.so, libscg_io.so and libscg_img.so: its entry points are declared here and in no other
 * header.  Conventions as there: plain C, `void* stream` is a hipStream_t (NULL = the default stream), every launch is asynchronous
 * on it, return value 0 = ok, < 0 = invalid argument (the SCG_E_* codes of scg_raster.h), > 0 = a hipError_t; the message of the
 * last failure of the calling thread is scg_mp_last_error().  Every argument is validated before anything touches a device.  The
 * caller owns all buffers; nothing is allocated, nothing is read back.
 *
 * The rule, all in fp32, for matches in arena order (views in dictionary order, per view its pairs in dictionary order):
 *   point cloud   EVERY match, no threshold: xyz = rays_o + rays_d * z (a product and a sum, each rounded; never fused), normals 0,
 *                 colour byte B(color * 255) (one rounded product).  B is the byte rule of include/io/scg_ply.h: the low 8 bits of
 *                 int32(trunc(v)) for a finite |v| < 2^31, 0 for everything else.  The record is storePly's: x y z nx ny nz (float)
 *                 red green blue (uchar), 27 bytes, little-endian.
 *   sparse depth  of a view, H x W, 0 where nothing lands: depth = z * cam_z (one rounded product; cam_z = cam_rays_d.z) at
 *                 row = int(clamp(uv.y, 0, H - 1)), col = int(clamp(uv.x, 0, W - 1)): the clamp acts on the float, the cast
 *                 truncates.  Where several matches of one view hit a pixel the match LATEST in arena order wins (an integer
 *                 atomicMax of the arena index, as the seeding step's).  A match whose uv is NOT FINITE is in the point cloud but
 *                 writes no depth — the rule csrc/seed.hip chose for the same line of the reference; the reference itself would
 *                 clamp an infinity to the edge and leaves the cast of a NaN undefined.  A finite uv of any size (2^33) is clamped.
 *   byte plane    of a view: q((d - min) / (max - min)) with the view's own min and max over the plane (two rounded differences,
 *                 one correctly rounded division), q = torchvision's save_image quantiser (csrc/pixel_rules.h), q(NaN) = 0.  A NaN
 *                 in the plane makes min and max NaN (torch.min / torch.max) and the plane black; so does a constant plane
 *                 (0 / 0).  Among zeros of both signs min is -0.0 and max +0.0, whatever order the threads run in.
 */
#ifndef SCG_MATCHPOINT_H
#define SCG_MATCHPOINT_H

#include "../scg_raster.h"

#define SCG_MP_ABI_VERSION 1
#define SCG_MP_RECORD_BYTES 27        /* bytes of a point-cloud record */
#define SCG_MP_TILE_RECORDS 64        /* records of one tile of the body: 432 dwords */
#define SCG_MP_MATCH_GROUP 256        /* matches per workgroup of the match kernel: four tiles, so a workgroup's first byte is a dword's */
#define SCG_MP_RESOLVE_PIXELS 256     /* pixels per workgroup of the resolve kernel */
#define SCG_MP_QUANT_PIXELS 1024      /* pixels per workgroup of the quantise kernel: four per thread, one dword */
#define SCG_MP_MAX_SEGMENTS 1024      /* ordered view pairs: the match kernel holds the table in LDS */
#define SCG_MP_MAX_VIEWS 1024
#define SCG_MP_MAX_DIM 65535          /* H and W of a view */
#define SCG_MP_MAX_MATCHES 2147483647 /* N < 2^31 */
#define SCG_MP_MAX_PIXELS 2147483647  /* pixels of all views together, each plane padded to four: < 2^31 */

#ifdef __cplusplus
extern "C" {
#endif

SCG_API const char* scg_mp_last_error(void);
SCG_API int32_t scg_mp_abi_version(void);
SCG_API size_t scg_mp_struct_bytes(int32_t which);      /* sizeof in the library: 0 ScgMpLayout, 1 ScgMpView, 2 ScgMpPack; else 0 */

/* The ONE output buffer.  Offsets are multiples of 256.  body_bytes is 27 N rounded up to 4; depth_bytes 4 * pixels (the planes of
 * the views one behind the other, view v at pixel views[v].first_pixel); byte_bytes the sum of H W rounded up to 4 per view (view v
 * at byte views[v].first_byte); range_bytes 8 V: (min, max) per view.  Padding and gaps are written as zeros. */
typedef struct ScgMpLayout {
    uint64_t body_offset, body_bytes;
    uint64_t depth_offset, depth_bytes;
    uint64_t byte_offset, byte_bytes;
    uint64_t range_offset, range_bytes;
    uint64_t total;
    uint64_t pixels;
    uint64_t resolve_groups, quant_groups;      /* workgroups of the two pixel kernels */
} ScgMpLayout;

typedef struct ScgMpView {
    int32_t H, W;
    int32_t first_pixel;        /* of the view's depth plane in the pixel arena */
    int32_t first_byte;         /* of its byte plane, a multiple of 4 */
    int32_t resolve_group;      /* its first workgroup in the resolve kernel: a workgroup works inside one view */
    int32_t quant_group;        /* ... and in the quantise kernel */
} ScgMpView;

/* Host only.  hw: V pairs (H, W).  views_out: V records, or NULL. */
SCG_API int scg_mp_layout(int32_t N, int32_t V, const int32_t* hw, ScgMpLayout* out, ScgMpView* views_out);

/* Bytes of the workspace: the winner map (one int32 per pixel of all views) and a (min, max) pair per workgroup of the resolve
 * kernel.  0 when the sizes are out of range. */
SCG_API size_t scg_mp_workspace_bytes(int32_t V, const int32_t* hw);

typedef struct ScgMpPack {
    int32_t struct_bytes;                  /* sizeof(ScgMpPack) of the caller */
    int32_t N, V, nseg;                    /* N >= 1 matches, V >= 1 views, 1 .. SCG_MP_MAX_SEGMENTS segments */
    const ScgSeedSegment* segments;        /* HOST table, validated before anything is launched: sorted, tiling [0, N) exactly */
    const ScgSeedSegment* segments_dev;    /* the same records in device memory */
    const ScgMpView* views;                /* HOST table: must equal what scg_mp_layout gives for its H and W */
    const ScgMpView* views_dev;            /* the same records in device memory (the kernels check every record they read against
                                              the buffer sizes: a copy that differs writes other pixels, never outside) */
    const float* rays_o;                   /* (N,3)  all inputs on the device, in arena order, read only */
    const float* rays_d;                   /* (N,3) */
    const float* z;                        /* (N) */
    const float* color;                    /* (N,3) */
    const float* uv;                       /* (N,2) */
    const float* cam_z;                    /* (N) */
} ScgMpPack;

/* buffer[0, layout.total), 16-byte aligned; workspace[0, scg_mp_workspace_bytes), 4-byte aligned.  Four launches whatever N, V and
 * nseg are: clear (winner map, gaps), matches (records, winners), resolve (depth planes, min / max partials), quantise (ranges,
 * byte planes).  Deterministic; capturable in a graph. */
SCG_API int scg_mp_pack(const ScgMpPack* args, void* buffer, size_t buffer_bytes, void* workspace, size_t workspace_bytes,
                        void* stream);

#ifdef __cplusplus
}
#endif
#endif

/* scg_mono.h — C ABI of the scene setup (csrc/mono.hip): GaussianModel.create_from_mono in three launches.
 *
 * The reference's scene/gaussian_model.py:284-360 builds `view_gs`, the dictionary every later step reads, in a Python loop over the
 * ordered view pairs: per pair two grid_sample calls, batched 3x3 products, three inverse() calls and a handful of small uploads.
 * Its rule decides every match from that match and its view's constants alone, except for the pair's count of valid matches, so
 * here it is one flat arena in the order the reference's loop walks (scgaussian_amd/_arena.py), written by
 *
 *     scg_mono_images     every view's uint8 image as fp32 byte / 255                                          1 launch
 *     scg_mono_matches    every match: uv, colour and mask samples, the three rays, the initial depth          1 launch
 *     scg_mono_pairs      every ordered pair: the partner's uv, valid, the pair's count, the loss weights       1 launch
 *
 * and no host read.  Same conventions as scg_geocheck.h: plain pointers, caller-owned device buffers, stream-ordered, int status,
 * arguments validated before anything touches a device, every value a kernel needs either a by-value argument or read from DEVICE
 * memory: the three calls can be captured in a graph.  The tables (views, segments, groups) are written by the caller on the host
 * and uploaded with the inputs; a kernel checks every index and offset it takes from them against the sizes in ScgMono and skips a
 * record that points outside, so a wrong table gives missing output, never an access outside the caller's buffers.
 *
 * Arithmetic.  The source is compiled without contraction: every operation below is rounded on its own.
 *   uv          = (fl(mx * W), fl(my * H)), m the fp32 match pixel, W and H as fp32.
 *   sampling    torch's grid_sample(mode="bilinear", padding_mode="zeros", align_corners=False) in its device form
 *               (ATen/native/GridSampler.h grid_sampler_unnormalize, ATen/native/cuda/GridSampler.cu), fp32:
 *                   g = fl(fl(m * 2) - 1);  ix = ((gx + 1) * W - 1) / 2;  iy likewise with H
 *                   x0 = floor(ix), x1 = x0 + 1, y0 = floor(iy), y1 = y0 + 1
 *                   nw = (x1 - ix) * (y1 - iy), ne = (ix - x0) * (y1 - iy), sw = (x1 - ix) * (iy - y0), se = (ix - x0) * (iy - y0)
 *                   out = 0; out += v(y0,x0) * nw; out += v(y0,x1) * ne; out += v(y1,x0) * sw; out += v(y1,x1) * se
 *               a tap outside the image adds nothing.  A view without a mask samples a plane of ones: the sum of its in-bounds
 *               weights.  A NaN coordinate samples nothing (colour 0, mask 0); a coordinate whose floor does not fit an int32 is
 *               outside; a NaN tap or weight otherwise propagates.
 *   rays        fp64 on the fp32 uv, from the view's fp64 constants, sums left to right:
 *                   p = Kinv (u, v, 1);  d = p / (sqrt(px*px + py*py + pz*pz) + 1e-8);  rays_d = Rc2w d;  cam_rays_d = Rw2c rays_d
 *                   rays_o = origin;  each output rounded to fp32 once, on its store;  cam_z = cam_rays_d.z
 *   z           = fl(fl(u * fl(far - near)) + near), u the match's uniform number.
 *   pairs       segment s = (a -> b), its partner t = (b -> a), both of M matches, element k:
 *                   uv_t[off_s + k] = uv[off_t + k];  valid = fl(mask[off_s + k] * mask[off_t + k]) > 0  (1.f or 0.f)
 *                   counts[s] = the number of valid elements: an integer, reduced in a fixed order (csrc/reduce.h)
 *                   wgt = valid / (float)counts[s], all zeros when the count is 0
 * Nothing is accumulated with atomics: two runs give the same bits. */
#ifndef SCG_MONO_H
#define SCG_MONO_H

#include <stddef.h>
#include <stdint.h>

#ifndef SCG_API
#define SCG_API __attribute__((visibility("default")))
#endif

#ifdef __cplusplus
extern "C" {
#endif

#define SCG_MONO_MAX_VIEWS 1024
#define SCG_MONO_MAX_SEGMENTS 65536

/* One view.  image_off: its first pixel in the image arenas, in pixels (bytes and floats both hold 3 per pixel); mask_off: its first
 * float in `masks`, or -1 for a view without a mask.  Kinv, Rc2w, Rw2c: row-major 3x3; origin: c2w[:3, 3]. */
typedef struct ScgMonoView {
    int64_t image_off, mask_off;
    int32_t H, W;
    float near_z, far_z;
    double Kinv[9], Rc2w[9], Rw2c[9], origin[3];
} ScgMonoView;

/* One ordered pair (a -> b): the elements [offset, offset + count) of every flat array; view: a's index; partner: the index of the
 * segment (b -> a), which holds the same number of elements. */
typedef struct ScgMonoSegment {
    int32_t offset, count, view, partner;
} ScgMonoSegment;

/* One workgroup of scg_mono_matches: the scg_mono_block() elements of `segment` from its element `first` on. */
typedef struct ScgMonoGroup {
    int32_t segment, first;
} ScgMonoGroup;

/* Everything the three calls take.  struct_bytes = sizeof(ScgMono).  All pointers are device memory.
 *   inputs    views (V), segments (nseg), groups (ngroups); image_bytes (image_pixels, 3) uint8; masks (mask_pixels) fp32, may be
 *             NULL when mask_pixels = 0; match_pixel (N, 2) and u (N) fp32
 *   outputs   image_color (image_pixels, 3); uv (N, 2); color (N, 3); blender_mask (N); rays_o, rays_d, cam_rays_d (N, 3); cam_z, z
 *             (N); uv_t (N, 2); valid, wgt (N), all fp32; counts (nseg) int32
 * max_view_pixels: the largest H * W of a view (the image launch's grid). */
typedef struct ScgMono {
    int32_t struct_bytes, V, nseg, ngroups, N, reserved;
    int64_t image_pixels, mask_pixels, max_view_pixels;
    const ScgMonoView* views;
    const ScgMonoSegment* segments;
    const ScgMonoGroup* groups;
    const uint8_t* image_bytes;
    const float* masks;
    const float* match_pixel;
    const float* u;
    float* image_color;
    float *uv, *color, *blender_mask, *rays_o, *rays_d, *cam_rays_d, *cam_z, *z, *uv_t, *valid, *wgt;
    int32_t* counts;
} ScgMono;

/* sizeof of ScgMono (0), ScgMonoView (1), ScgMonoSegment (2), ScgMonoGroup (3); anything else: 0 */
SCG_API size_t scg_mono_struct_bytes(int32_t which);

/* Elements per workgroup of scg_mono_matches and per trip of scg_mono_pairs.  For the group table and for tests at its edges. */
SCG_API int32_t scg_mono_block(void);

/* Every call validates the whole struct first, in this order: NULL `a` (SCG_E_NULL); struct_bytes (SCG_E_RANGE); 1 <= V <=
 * SCG_MONO_MAX_VIEWS, 1 <= nseg <= SCG_MONO_MAX_SEGMENTS, 1 <= N, 1 <= ngroups < 2^24, 1 <= max_view_pixels <=
 * image_pixels, max_view_pixels < 2^31, mask_pixels >= 0 (SCG_E_RANGE); a NULL pointer other than `masks` at mask_pixels = 0
 * (SCG_E_NULL); views not 8-byte or another pointer not 4-byte aligned (SCG_E_ALIGN). */

/* image_color = fl((float)byte / 255.f), the division correctly rounded.  Grid (trips over the largest view, V). */
SCG_API int scg_mono_images(const ScgMono* a, void* stream);

/* One workgroup per group, one thread per match.  Reads image_color: stream-ordered behind scg_mono_images. */
SCG_API int scg_mono_matches(const ScgMono* a, void* stream);

/* One workgroup per segment.  Reads uv and blender_mask: stream-ordered behind scg_mono_matches. */
SCG_API int scg_mono_pairs(const ScgMono* a, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SCG_MONO_H */

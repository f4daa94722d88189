/* scg_geocheck.h — C ABI of the cross-view depth consistency check (csrc/geocheck.hip).
 *
 * The reference's utils/geo_check.py:25-128 (`get_pairs`, `reproject_with_depth`, `geocheck`) keeps a pixel of a depth map when
 * enough of the nearest other views agree with it: the pixel is projected into a source view with its depth, the source depth is
 * sampled there, the sample is lifted and projected back, and the round trip has to land within `dist_thresh` pixels and
 * `depth_thresh` relative depth of where it started.  Every pixel is decided from that pixel alone, so the whole rule is
 *
 *     scg_geocheck_setup    nearest source views and the composed matrices of every (view, source) pair   1 launch
 *     scg_geocheck          every pixel of every view: votes, mask, filtered depth                        1 launch
 *
 * and no host read.  Same conventions as scg_loss.h: plain pointers, caller-owned device buffers, stream-ordered, int status,
 * arguments validated before anything touches a device, every value a kernel needs either a by-value argument or read from DEVICE
 * memory: both calls can be captured in a graph.
 *
 * Arithmetic.  The reference is numpy float64 between its fp32 casts, and so is this: the matrices are composed in fp64, the walk
 * of a pixel is fp64, and a value is rounded to fp32 exactly where utils/geo_check.py:109-110, :122 and :125-126 round it.  The
 * source is compiled without contraction.  cv2.remap's 5-bit fixed-point weights are not reproduced: the sampler is the exact-weight
 * bilinear with a zero border of oracle/geo_check_oracle.py.
 *
 * Pair selection (:25-31).  The distance of two cameras is sqrt(dx*dx + dy*dy + dz*dz) of the translation columns of their 4x4
 * matrices, summed in that order; a view's distance to itself is replaced by 1e3; the J = min(num_src, N) smallest are its sources,
 * equal distances in the order of their index (a stable sort), NaN last.  Two quirks of the reference are kept: with num_src >= N a
 * view is one of its own sources, sorted where 1e3 falls, and a camera farther away than 1e3 sorts behind the view itself.
 *
 * Per (view i, slot s) with source j, the setup writes
 *     M1 = K_j R_ji K_i^-1     t1 = K_j t_ji        [R_ji | t_ji] = E_j E_i^-1        reference pixel and depth -> source image
 *     M2 = R_ij K_j^-1         t2 = t_ij            [R_ij | t_ij] = E_i E_j^-1        source pixel and sample   -> reference camera
 * and K_i once per view.  E are the 4x4 matrices the reference calls c2ws and uses as each camera's view transform.  Inverses are
 * the explicit adjugate over the determinant: a singular matrix gives non-finite entries and therefore no votes, not an error. */
#ifndef SCG_GEOCHECK_H
#define SCG_GEOCHECK_H

#include <stddef.h>
#include <stdint.h>

#ifndef SCG_API
#define SCG_API __attribute__((visibility("default")))
#endif

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of the workspace of N views with num_src sources each: the (N, J) int32 pair table at its start, then K_i, then the pair
 * records.  1 <= N <= 1024 and 1 <= num_src <= 64, anything else: 0. */
SCG_API size_t scg_geocheck_workspace_bytes(int32_t N, int32_t num_src);

/* Pixel tile of one workgroup of scg_geocheck: axis 0 its width, axis 1 its height (anything else: 0).  For tests at its edges. */
SCG_API int32_t scg_geocheck_tile(int32_t axis);

/* intrs (N,3,3) and exts (N,4,4), fp64, row-major, in device memory.  1 <= N <= 1024, 1 <= num_src <= 64: otherwise SCG_E_RANGE.
 * workspace: scg_geocheck_workspace_bytes(N, num_src) bytes, 8-byte aligned, caller-owned; it is written here and read by
 * scg_geocheck, and its first N * J int32 are the pair table, row i the sources of view i in slot order.  One thread per view. */
SCG_API int scg_geocheck_setup(const double* intrs, const double* exts, int32_t N, int32_t num_src, void* workspace,
                               size_t workspace_bytes, void* stream);

/* depths (N,H,W) fp32; workspace: what scg_geocheck_setup wrote for the same N and num_src.  H, W >= 1 and H * W < 2^31, N and
 * num_src as above: otherwise SCG_E_RANGE.  Views are indexed in 64 bits.  The grid is (pixel tiles, N); one thread per reference
 * pixel (u, v) walks the J slots of its view in slot order, with d its fp32 depth widened to fp64:
 *     k = M1 (u d, v d, d) + t1;  xs = k0 / k2, ys = k1 / k2                      IEEE divisions, no guard on k2
 *     s = the source depth at (fp32(xs), fp32(ys)): bilinear in fp64, x0 = floor, weights x - x0 and 1 - that, the four taps in
 *         the order (y0,x0) (y0,x0+1) (y0+1,x0) (y0+1,x0+1), each value * wx * wy, taps outside the image 0, rounded to fp32;
 *         a non-finite coordinate, or one whose floor does not fit an int32, samples 0
 *     X = M2 (xs s, ys s, s) + t2 with the unrounded xs, ys;  d_back = fp32(X.z);  (ub, vb) = fp32 of (K_i X).xy / (K_i X).z
 *     agree = hypot(ub - u, vb - v) < dist_thresh && |d_back - d| / d < depth_thresh          fp64; NaN compares false
 *     votes += agree;  sum += agree ? d_back : 0                                                fp64
 * Outputs, each (N,H,W):
 *     votes      uint8
 *     masks      fp32, 1 where votes > view_thresh, else 0
 *     filtered   fp32((sum + d) / (votes + 1)) * mask: a product, as in the reference, so a NaN depth stays NaN
 * The slot records are the same for a whole workgroup and are fetched with scalar loads; no LDS, no atomics, no workgroup waits
 * for another.  Nothing is accumulated across threads: two runs give the same bits. */
SCG_API int scg_geocheck(const float* depths, int32_t N, int32_t H, int32_t W, int32_t num_src, double dist_thresh,
                         double depth_thresh, int32_t view_thresh, const void* workspace, size_t workspace_bytes, uint8_t* votes,
                         float* masks, float* filtered, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SCG_GEOCHECK_H */

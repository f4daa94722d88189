/* scg_viz.h — C ABI of the depth colour maps and the video frames (csrc/depthviz.hip).
 *
 * The reference ends every view of render.py and render_video.py with `visualization(depth, path)` (render.py:97-110,
 * render_video.py:98-113): the normalised depth goes to the host, np.percentile(depth, 98) and depth.min() become matplotlib's
 * Normalize(vmin, vmax), a 256-entry turbo table is looked up through ScalarMappable.to_rgba and the float64 RGBA image is
 * truncated to bytes.  render_video.py:148 adds the colour frame (rendering * 255.).astype(uint8)[..., ::-1].  Every pixel is
 * decided from that pixel and two scalars of the image, so a frame is
 *
 *     scg_viz_select    the minimum and the two order statistics under the percentile, exactly     1 reset + 4 launches
 *     scg_viz_frame     every 8-bit image of the frame                                             1 launch
 *
 * and no host read.  Same conventions as scg_eval.h: plain pointers, caller-owned device buffers, stream-ordered, int status,
 * arguments validated before anything touches a device, every value a kernel needs read from DEVICE memory: every call can be
 * captured in a graph.
 *
 * x is the plane being coloured: with `range` (the two floats of scg_eval_depth_range) x = fl(fl(depth - min) / fl(max - min)),
 * the expression scg_eval_view uses for depth_u8; with range == NULL x = depth.  All arithmetic is fp32, every operation rounded on
 * its own.
 *
 * The rule (numpy >= 2's np.percentile on a float32 array, method 'linear'; matplotlib's Normalize and Colormap.__call__):
 *     q = fl(f32(p) / 100), pos = fl(f32(n - 1) * q), lo = floor(pos), hi = min(lo + 1, n - 1), g = fl(pos - f32(lo))
 *     a, b = the values of rank lo, hi of x in ascending order, d = fl(b - a)
 *     vmax = g < 0.5 ? fl(a + fl(d * g)) : fl(b - fl(d * fl(1 - g)));   vmin = the value of rank 0
 *     one NaN anywhere in x makes vmin and vmax NaN (ndarray.min, np.percentile)
 *     vmin == vmax: every pixel has index 0.  Otherwise t = fl32(fl32(x - vmin) / (f64(vmax) - f64(vmin))), the division in fp64
 *     (Normalize keeps vmin and vmax as Python floats; with vmin = 0, as for every normalised depth, it is the fp32 division
 *     fl(x / vmax)), s = fl(t * 256):
 *     t NaN -> the pixel is (0, 0, 0);  s < 0 -> index 0;  s >= 256 -> index 255;  otherwise trunc(s);  colour = lut[index]. */
#ifndef SCG_VIZ_H
#define SCG_VIZ_H

#include <stddef.h>
#include <stdint.h>

#ifndef SCG_API
#define SCG_API __attribute__((visibility("default")))
#endif

#ifdef __cplusplus
extern "C" {
#endif

/* Elements of x one workgroup of the select passes reads.  For tests at its edges. */
SCG_API int32_t scg_viz_select_block(void);

/* Bytes of scratch scg_viz_select needs for n values (the histograms of its passes; 0 when n is out of range). */
SCG_API size_t scg_viz_select_scratch_bytes(int64_t n);

/* Exact selection.  depth: n fp32, 1 <= n <= 2^24 (n - 1 must be exact in fp32), otherwise SCG_E_RANGE; percentile in [0, 100],
 * otherwise SCG_E_RANGE; lo, hi and g are formed on the host from n and percentile alone.  range: 2 device floats or NULL.
 * stats: 4 device floats (vmin, vmax, a, b).  nan_count: one device int32, the number of NaNs in x.  scratch: 4-byte aligned,
 * reset by this call.
 * A radix select on the order-preserving 32-bit key of x in three passes of 11, 11 and 10 bits; the prefixes of rank lo and rank
 * hi are both carried.  Each pass builds a workgroup's histogram in LDS and adds it to a global one with integer atomics (exact
 * in any order: the result is deterministic); the workgroups of the next pass each re-derive the chosen digits from the global
 * histograms themselves, and a last one-workgroup launch writes the outputs.  No workgroup waits for another.  The minimum and
 * the NaN count ride on the first pass.  NaNs sort behind +inf (np.sort); -0.0 sorts in front of +0.0. */
SCG_API int scg_viz_select(const float* depth, const float* range, int64_t n, double percentile, float* stats, int32_t* nan_count,
                           void* scratch, size_t scratch_bytes, void* stream);

/* One frame, one launch.  render (3,H,W) fp32 unclamped or NULL; depth (H,W) fp32; range as above; stats and nan_count as
 * scg_viz_select wrote them for the same depth and range; lut: 768 bytes in device memory, 256 x (R, G, B).  1 <= H * W < 2^31.
 * Outputs, (H,W,3) bytes written as whole pixels; every one but the first may be NULL:
 *   depth_color_u8       the colour map, R, G, B
 *   depth_color_bgr_u8   the same, B, G, R (what a video writer takes)
 *   depth_u8             (H,W): q(x), q the quantiser of scg_eval.h
 *   render_u8            q(clamp(render, 0, 1)); needs render
 *   frame_bgr_u8         render_video.py:132,148: trunc(fl(clamp(render, 0, 1) * 255)) per channel, NaN -> 0, stored B, G, R;
 *                        needs render */
SCG_API int scg_viz_frame(const float* render, const float* depth, const float* range, const float* stats, const int32_t* nan_count,
                          const uint8_t* lut, int32_t H, int32_t W, uint8_t* depth_color_u8, uint8_t* depth_color_bgr_u8,
                          uint8_t* depth_u8, uint8_t* render_u8, uint8_t* frame_bgr_u8, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SCG_VIZ_H */

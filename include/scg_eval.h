/* scg_eval.h — C ABI of the test-set evaluation (csrc/evalview.hip).
 *
 * The reference evaluates a trained model in two scripts.  render.py:119-162 (`render_set`) renders every test view, normalises the
 * depth by its own min / max, builds the error map utils/loss_utils.py:195-205 (`get_pixel_loss`: an L1 term plus a 5x5 box-window
 * SSIM behind a reflection pad) and writes render, ground truth, depth, error map and DTU mask as 8-bit PNGs.  metrics.py:26-118
 * reads the PNGs back, forms image * mask + (1 - mask) and computes the 11x11 SSIM and a PSNR under mask == 1.  PNG is lossless:
 * everything metrics.py computes is a function of the QUANTISED pixels, so both scripts are, per view,
 *
 *     scg_eval_depth_range      the two scalars of the depth map                                       2 launches
 *     scg_eval_view             quantised images, error map, masked images, the integers of the PSNR   1 reset + 1 launch
 *     scg_image_loss_forward    (scg_loss.h) the 11x11 SSIM of the two masked images                   2 launches
 *
 * and no host read.  Same conventions as scg_loss.h: plain pointers, caller-owned device buffers, stream-ordered, int status,
 * arguments validated before anything touches a device, every value a kernel needs read from DEVICE memory: every call can be
 * captured in a graph.
 *
 * The quantiser is what torchvision.utils.save_image applies (mul(255).add_(0.5).clamp_(0, 255).to(uint8)), each operation rounded
 * on its own in fp32:
 *     q(x) = uint8(trunc(clamp(fl(fl(x * 255) + 0.5), 0, 255)))
 * torch leaves the cast of NaN to uint8 undefined; here q(NaN) = 0.  +inf gives 255, -inf and -0.0 give 0. */
#ifndef SCG_EVAL_H
#define SCG_EVAL_H

#include <stddef.h>
#include <stdint.h>

#ifndef SCG_API
#define SCG_API __attribute__((visibility("default")))
#endif

#ifdef __cplusplus
extern "C" {
#endif

/* Depth range (render.py:143: depth.min(), depth.max()).  depth: n fp32, 1 <= n < 2^31.  range: 2 floats in device memory,
 * range[0] = min, range[1] = max; one NaN among the inputs makes both NaN, as torch.min / torch.max do.  Per-workgroup partial
 * results, then one workgroup combines them: min and max do not depend on the order. */
SCG_API size_t scg_eval_depth_range_scratch_bytes(int64_t n);
SCG_API int scg_eval_depth_range(const float* depth, int64_t n, float* range, void* scratch, size_t scratch_bytes, void* stream);

/* Pixel tile of one workgroup of scg_eval_view: axis 0 its width, axis 1 its height (anything else: 0).  For tests at its edges. */
SCG_API int32_t scg_eval_view_tile(int32_t axis);

/* One view.  render (3,H,W) fp32, unclamped; gt (3,H,W) fp32; depth (H,W) fp32; dtumask (H,W) fp32 or NULL; range: the two floats
 * scg_eval_depth_range wrote.  H >= 3 and W >= 3 (torch's ReflectionPad2d(2) refuses smaller inputs), H * W < 2^31: otherwise
 * SCG_E_RANGE.  One workgroup per pixel tile; the six image planes go through LDS with a halo of 2, reflected at the image
 * border; no workgroup waits for another.  Outputs:
 *   render_u8, gt_u8   (H,W,3) bytes, interleaved as an image file wants them: q(render), q(gt)
 *   depth_u8           (H,W): q((depth - min) / (max - min)), two subtractions and one correctly rounded division, as torch rounds
 *                      them; max == min gives NaN and therefore a zero image
 *   error_f32          (H,W) fp32 or NULL: get_pixel_loss(render, gt) =
 *                          0.5 * mean_c |r - g| + 0.5 * mean_c clamp((1 - n / d) / 2, 0, 1)
 *                      n = (2 mu_x mu_y + C1)(2 sigma_xy + C2), d = (mu_x^2 + mu_y^2 + C1)(sigma_x + sigma_y + C2), the means of
 *                      x, y, x^2, y^2, xy taken over the 5x5 window of the reflection-padded images, C1 = 1e-4, C2 = 9e-4
 *   error_u8           (H,W): q of the kernel's own fp32 error value
 *   mask_u8            (H,W): q(dtumask); required with dtumask, not written without
 *   render_masked, gt_masked   (3,H,W) fp32, metrics.py:43-44 on the quantised values: with a = fl(float(q) / 255) and
 *                      m = fl(float(q_mask) / 255), fl(fl(a * m) + fl(1 - m)); without a mask m = 1 and the images are a
 *   sk                 2 x uint64, 8-byte aligned, reset and written by this call:
 *                      sk[0] = S = sum of (q_render - q_gt)^2 over the three channels of the pixels with q_mask == 255 (metrics.py:42,
 *                      mask == 1.; without a mask every pixel), sk[1] = K = the number of such ELEMENTS (3 per pixel).
 *                      Integer atomics: exact in any order.  PSNR = 10 log10(255^2 K / S). */
SCG_API int scg_eval_view(const float* render, const float* gt, const float* depth, const float* dtumask, const float* range,
                          int32_t H, int32_t W, uint8_t* render_u8, uint8_t* gt_u8, uint8_t* depth_u8, uint8_t* error_u8,
                          uint8_t* mask_u8, float* error_f32, float* render_masked, float* gt_masked, uint64_t* sk, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SCG_EVAL_H */

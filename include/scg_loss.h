/* scg_loss.h — C ABI of the fused image loss.
 *
 * The reference's per-iteration image loss (train.py:160-161):
 *     Ll1  = l1_loss(image, gt_image)                                   utils/loss_utils.py:40
 *     loss = (1 - lambda_dssim) * Ll1 + lambda_dssim * (1 - ssim(image, gt_image))    utils/loss_utils.py:56-94
 * where ssim() is the 11x11 Gaussian-window (sigma 1.5) SSIM, computed by the reference with five zero-padded
 * grouped conv2d calls per iteration (plus their backward).  Here the whole loss and its gradient w.r.t. `image`
 * are two kernels: separable 11-tap convolutions staged through LDS, SSIM map and its three derivative maps in the
 * forward, three more separable convolutions in the backward.
 *
 * Same conventions as scg_raster.h (caller-owned device buffers, stream-ordered, int status). */
#ifndef SCG_LOSS_H
#define SCG_LOSS_H

#include <stddef.h>
#include <stdint.h>

/* The library is built with -fvisibility=hidden: exactly the entry points declared in the headers under include/ are exported. */
#ifndef SCG_API
#define SCG_API __attribute__((visibility("default")))
#endif

#ifdef __cplusplus
extern "C" {
#endif

/* bytes of the `dmaps` buffer: three (C,H,W) fp32 derivative maps saved by the forward for the backward */
SCG_API size_t scg_image_loss_dmaps_bytes(int32_t C, int32_t H, int32_t W);

/* bytes of the forward's scratch (per-workgroup partial sums, reduced in fixed order by a second tiny kernel:
 * no same-address atomics, bitwise reproducible) */
SCG_API size_t scg_image_loss_scratch_bytes(int32_t C, int32_t H, int32_t W);

/* Forward.  img, gt: (C,H,W) fp32.  sums: 2 floats written by this call:
 *   sums[0] = sum over all elements of |img - gt|,  sums[1] = sum over all elements of the SSIM map
 * (the caller divides by C*H*W: L1 = sums[0]/N, SSIM = sums[1]/N).  dmaps: see above (may be NULL when no
 * gradient is needed). */
SCG_API int scg_image_loss_forward(const float* img, const float* gt, int32_t C, int32_t H, int32_t W, float* sums,
                           float* dmaps, void* scratch, size_t scratch_bytes, void* stream);

/* Backward.  d_img (C,H,W) = w[0] * sign(img - gt) + w[1] * d(sum of SSIM map)/d(img), with the two weights read
 * from DEVICE memory (`weights`, 2 floats) so that the upstream gradients — device scalars under autograd — never
 * force a host read.  For loss = (1-l)*L1 + l*(1-SSIM) with upstream gradient g:  w[0] = g*(1-l)/N,  w[1] = -g*l/N. */
SCG_API int scg_image_loss_backward(const float* img, const float* gt, const float* dmaps, int32_t C, int32_t H, int32_t W,
                            const float* weights, float* d_img, void* stream);

/* The training loss in one piece (round 5): like scg_image_loss_forward, and sums3[2] = (1 - lambda_dssim) * sums3[0] / N +
 * lambda_dssim * (1 - sums3[1] / N) — train.py:160-161, the reference's expression in its order of operations — written by the
 * same reduction kernel; scg_image_loss_backward_combined takes the upstream gradient of THAT scalar (`upstream`: one float in
 * DEVICE memory) and forms the two weights itself: d_img = upstream * ((1-l)/N * sign(img - gt) - l/N * d(sum SSIM)/d(img)).
 * A training iteration's image loss is then two library calls and no tensor arithmetic around them (the separate form costs
 * the caller's framework about a dozen one-element kernels per iteration). */
SCG_API int scg_image_loss_forward_combined(const float* img, const float* gt, int32_t C, int32_t H, int32_t W,
                                            float lambda_dssim, float* sums3, float* dmaps, void* scratch,
                                            size_t scratch_bytes, void* stream);
SCG_API int scg_image_loss_backward_combined(const float* img, const float* gt, const float* dmaps, int32_t C, int32_t H,
                                             int32_t W, const float* upstream, float lambda_dssim, float* d_img,
                                             void* stream);

/* ---- DTU scenes (csrc/dtumask.hip): what train.py runs only when "dtu" is in the source path ------------------------------
 * Same conventions: caller-owned buffers, stream-ordered, int status, arguments validated before anything touches a device;
 * counts and upstream gradients are read from DEVICE memory, so nothing here forces a host read and every call can be captured
 * in a graph.
 *
 * Background mask (train.py:149-158).  gt: (3,H,W) fp32.  mask (H,W) uint8 = 1 where the pixel is dark (max over the channels
 * < thr) and the run of dark pixels ending at its row in its column is at least min(row + 1, run) long — the closed form of the
 * reference's 49 shifted products (run = 50).  gt_masked (3,H,W) = gt with the masked pixels zeroed; it MAY BE gt itself (the
 * reference's in-place form) when thr > 0, since a zeroed pixel stays dark; thr <= 0 with aliasing, a partial overlap and
 * run < 1 are refused with SCG_E_RANGE.  count: one uint32, the number of masked pixels (reset and written by this call).
 * Comparisons only: the result is exact. */
SCG_API int scg_dtu_bg_mask(const float* gt, int32_t H, int32_t W, float thr, int32_t run, uint8_t* mask, float* gt_masked,
                            uint32_t* count, void* stream);
/* rows of one row segment of the mask kernel (a segment re-reads up to run - 1 rows above itself): for tests at its edges */
SCG_API int32_t scg_dtu_bg_mask_segment_rows(void);

/* Alpha term (train.py:167-168: rendered_alpha[bg_mask].mean()).  x: n fp32, mask: n uint8, count: one uint32 in device memory
 * (what scg_dtu_bg_mask wrote).  Forward: out[0] = sum(x[mask]) / count, per-workgroup partial sums added in a fixed order
 * (bitwise reproducible); count == 0 gives NaN, as torch's mean of an empty selection.  Backward: d_x = mask ? upstream / count : 0
 * with `upstream` one float in device memory; count == 0 gives all zeros. */
SCG_API size_t scg_masked_mean_scratch_bytes(int64_t n);
SCG_API int scg_masked_mean_forward(const float* x, const uint8_t* mask, int64_t n, const uint32_t* count, float* out,
                                    void* scratch, size_t scratch_bytes, void* stream);
SCG_API int scg_masked_mean_backward(const uint8_t* mask, int64_t n, const uint32_t* count, const float* upstream, float* d_x,
                                     void* stream);

/* Evaluation metrics (train.py:252-265).  img, gt: (C,H,W) fp32, C <= 16, both clamped to [0, 1] inside the kernel; mask: (H,W)
 * fp32 or NULL, a pixel is selected when mask > 0 (NULL: all n = H*W pixels).  out: 2 + C floats,
 *   out[0] = l1 = mean of |a - b| over the selected C x n elements,
 *   out[1] = psnr = mean over c of 20 * log10(1 / sqrt(mse[c]))                                     utils/image_utils.py:17-19
 *   out[2 + c] = mse[c] = mean over the selected pixels of (a - b)^2 in channel c.
 * Reduced in a fixed order; an empty selection gives NaN everywhere. */
SCG_API size_t scg_eval_metrics_scratch_bytes(int32_t C, int32_t H, int32_t W);
SCG_API int scg_eval_metrics(const float* img, const float* gt, const float* mask, int32_t C, int32_t H, int32_t W, float* out,
                             void* scratch, size_t scratch_bytes, void* stream);

/* The evaluation (scg_eval.h), the cross-view depth check (scg_geocheck.h), the depth colour maps (scg_viz.h) and the scene setup
 * (scg_mono.h) each have their own header, and every entry point is declared in exactly one header under include/.  The 11x11
 * SSIM of the evaluation is scg_image_loss_forward above. */

#ifdef __cplusplus
}
#endif
#endif /* SCG_LOSS_H */

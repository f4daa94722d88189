/* scg_virtualwarp.h — C ABI of libscg_vw.so: the two sparse-view regularisers of utils/loss_utils.py, forward AND backward, on the
 * GPU (csrc/virtualwarp.hip, gfx950): get_virtual_warp_loss (:208-246, with the 5x5 box SSIM of :162-193) and get_smooth_loss
 * (:19-38).
 *
 * A fifth library next to libscg_raster.so, libscg_io.so, libscg_img.so and libscg_mp.so: its entry points are declared here and
 * in no other header.  Conventions as there: plain C, `void* stream` is a hipStream_t (NULL = the default stream), every launch is
 * asynchronous on it, return value 0 = ok, < 0 = invalid argument (the SCG_E_* codes of scg_raster.h), > 0 = a hipError_t; the
 * message of the last failure of the calling thread is scg_vw_last_error().  Every argument is validated before anything touches
 * a device.  The caller owns all buffers, scratch included; nothing is allocated, nothing is read back.  No float atomics: every
 * scalar is the sum of per-workgroup partial sums (csrc/reduce.h) folded by one workgroup in a fixed order, so two runs are bitwise
 * equal.  Precision: inputs and outputs are fp32; everything between them — the projection, the sampler, the 5x5 window sums, the
 * SSIM terms, the coefficients, every sum over pixels or windows — is formed in fp64, one rounding per operation (compiled with
 * -ffp-contract=off), and rounded to fp32 once, where an output or a coefficient map is stored.  (E[x x] - mx mx cancels: in
 * fp32 it alone costs the loss five digits, and a mean of per-pixel terms is held to one ulp only by a sum that carries more.)
 *
 * THE WARP LOSS.  Inputs: virtual_img (3,H,W), virtual_depth (H,W), vir_mask (H*W bytes, non-zero = true), img_colors (nv,3,H,W),
 * records (nv,12): per view M (3x3, row major) then t (3), where M_v = K_v R_v R_vir K_0^-1 and t_v = K_v (R_v t_vir + t_v) are
 * composed by the caller in fp64 and rounded once.  Per pixel q = (px, py) with depth d, and view v:
 *   a = M (px, py, 1);  (X, Y, Z) = d * a + t;  x = X / (Z + 1e-8), y = Y / (Z + 1e-8)
 *   nx = 2 x / (W - 1) - 1, ny = 2 y / (H - 1) - 1;  in bounds <=> |nx| <= 1 and |ny| <= 1 (a NaN is out of bounds; no test for a
 *   point behind the camera: it can land in bounds, as in the reference)
 *   y_v(q) = torch's grid_sample(bilinear, zeros, align_corners=False) of img_colors[v] at (nx, ny): the tap position is
 *   gx = ((nx + 1) W - 1) / 2, so normalised with W - 1 and sampled with W, as the reference does.  A NaN coordinate samples zero;
 *   a coordinate whose floor does not fit an int32 is outside (the rules of csrc/mono.hip).
 * Per pixel p, view v and channel c, with E[.] the mean over the 5x5 window behind ReflectionPad2d(2) (so H, W >= 3):
 *   mx = E[x], my = E[y], sx = E[x x] - mx mx, sy = E[y y] - my my, sxy = E[x y] - mx my     (x = virtual_img, y = y_v)
 *   n = (2 mx my + C1)(2 sxy + C2), dd = (mx mx + my my + C1)(sx + sy + C2), C1 = 0.01^2, C2 = 0.03^2
 *   term = clamp((1 - n / dd) / 2, 0, 1);  s_v(p) = mean over c of term; s_v(p) = 1000 where v is out of bounds at p itself
 *   winner w(p) = the lowest v attaining min_v s_v(p); -1 where that minimum is >= 1000 or vir_mask[p] is false
 *   loss_map(p) = s_w(p), or 0 where w(p) = -1;  loss = sum of loss_map / (H W).  The reference's dropped l1 is not computed.
 *
 * ITS BACKWARD, to virtual_img and virtual_depth (img_colors, records and mask are constants), gather form only.  For a window p
 * and channel c the derivative of `term` with respect to a window member j is (A + B y_j + C x_j) / 25 on the y side and
 * (A' + B' x_j + C y_j) / 25 on the x side, where with r = n / dd, n1, n2 the factors of n and d1, d2 those of dd:
 *   A = -[mx (n2 - n1) - r my (d2 - d1)] / dd, A' = -[my (n2 - n1) - r mx (d2 - d1)] / dd, B = B' = r d1 / dd, C = -n1 / dd
 * (B' equals B, so FOUR maps are kept), all zero where the clamp is active (term outside [0, 1], or a NaN) or w(p) = -1; only view
 * w(p) enters.  The gradient at q is the sum over the windows p that contain q, each counted as often as its padded 5x5 holds a
 * position that reflects onto q: per axis q itself, -q when 1 <= q <= 2, 2 (W - 1) - q when W - 3 <= q <= W - 2; every such
 * window's centre lies within 2 of q.  The sum is scaled by upstream / (25 * 3 * H W).  The depth gradient is the same sum with
 * each y-side term multiplied by d y_{w(p),c}(q) / d depth = dsample/dgx * dgx/dd + dsample/dgy * dgy/dd, with
 * dx/dd = (a_x (Z + 1e-8) - X a_z) / (Z + 1e-8)^2 and dgx/dx = W / (W - 1); taps outside the image contribute nothing.
 *
 * NON-FINITE VALUES of virtual_img or img_colors.  Everything above is formed as written, in IEEE arithmetic, except that a window
 * whose winner is not v (w(p) = -1 included) is SKIPPED in view v's sum, not multiplied by zero.  A tap inside the image enters the
 * sample whatever its weight (0 * NaN = NaN, as torch's sampler).  A window that holds a non-finite x or y_v has a NaN term, so
 * s_v(p) is a NaN; a NaN is the minimum and the FIRST view with one wins (torch.min); loss_map(p) and loss are NaN unless the mask
 * removes p.  Such a window's coefficients are zero, so it gives its finite members nothing: the gradients stay finite around the
 * value.  AT the element q that holds it the zero coefficients meet x_q or y_v(q) itself, and 0 * NaN = 0 * inf = NaN: d_img(c, q)
 * and d_depth(q) are NaN where any window within 2 of q has a winner, and d_img(c, q) is exactly 0 where none has.  d_depth(q) adds
 * (y-side sum) * dy_v,c(q)/ddepth over EVERY view and channel, a view that wins nothing near q with a sum of 0: where that
 * derivative is not finite (a non-finite texel under q's taps, a NaN depth) d_depth(q) is NaN, masked out or not.  (Autograd of the
 * reference's expression divides a zero upstream by the NaN denominator and marks the whole 9 x 9 block, masked out or not.)
 *
 * WHAT IS STORED, WHAT RECOMPUTED.  The forward WRITES to scratch the warped images y (nv,3,H,W) and the sampler's derivative
 * dy/ddepth (nv,3,H,W), both fp64, and the four coefficient maps (4,3,H,W) of the winning view, fp32; the backward reads them and
 * recomputes nothing.
 * Tiling: a workgroup is SCG_VW_TILE x SCG_VW_TILE pixels (one per thread) inside one view; windows are gathered through the cache.
 * Launches: forward 3 (warp, ssim, fold), backward 1, whatever nv is (1 .. SCG_VW_MAX_VIEWS).
 *
 * THE SMOOTHNESS LOSS.  depth (H,W); guide NULL (C = 0: weights 1), (H,W) (C = 1) or (C,H,W):
 *   loss = mean over H x (W-1) of |d[i,j] - d[i,j+1]| * exp(-gx) + mean over (H-1) x W of |d[i,j] - d[i+1,j]| * exp(-gy)
 * gx, gy the mean over C of the guide's absolute differences (the sum over C in channel order, then one division by C); exp is the
 * accurate expf.  An empty mean (W == 1 or H == 1) is NaN, as in torch.  Forward 2 launches (partials, fold); backward 1 gather
 * launch to depth with sign(0) = 0; the guide gets no gradient.
 */
#ifndef SCG_VIRTUALWARP_H
#define SCG_VIRTUALWARP_H

#include "../scg_raster.h"

#define SCG_VW_ABI_VERSION 1
#define SCG_VW_MAX_VIEWS 16           /* nv of one call */
#define SCG_VW_TILE 16                /* side of a workgroup's pixel tile in the warp kernels */
#define SCG_VW_SMOOTH_PIXELS 256      /* pixels per workgroup of the smoothness kernels */
#define SCG_VW_RECORD_FLOATS 12       /* M (9, row major) and t (3) per view */
#define SCG_VW_MIN_DIM 3              /* ReflectionPad2d(2) needs H, W >= 3 */
#define SCG_VW_MAX_DIM 16384          /* H and W */
#define SCG_VW_MAX_GUIDE_CHANNELS 64

#ifdef __cplusplus
extern "C" {
#endif

SCG_API const char* scg_vw_last_error(void);
SCG_API int32_t scg_vw_abi_version(void);

/* Bytes of the warp loss's scratch, in this order from its first byte: y and dy/ddepth ((nv,3,H,W) fp64 each), one fp64 partial sum
 * per workgroup, the coefficient maps ((4,3,H,W) fp32).  0 when a size is out of range. */
SCG_API size_t scg_vw_warp_scratch_bytes(int32_t nv, int32_t H, int32_t W);

/* loss: 1 float.  loss_map (H,W) float, winner (H,W) int8, in_bounds (nv,H,W) bytes.  scratch 16-byte aligned. */
SCG_API int scg_vw_warp_forward(int32_t nv, int32_t H, int32_t W, const float* virtual_img, const float* virtual_depth,
                                const uint8_t* vir_mask, const float* img_colors, const float* records, float* loss,
                                float* loss_map, int8_t* winner, uint8_t* in_bounds, void* scratch, size_t scratch_bytes,
                                void* stream);

/* scratch and winner as the forward of the same inputs left them.  upstream: 1 float in device memory.  d_img (3,H,W),
 * d_depth (H,W): every element is written. */
SCG_API int scg_vw_warp_backward(int32_t nv, int32_t H, int32_t W, const float* virtual_img, const float* upstream,
                                 const int8_t* winner, const void* scratch, size_t scratch_bytes, float* d_img, float* d_depth,
                                 void* stream);

/* Bytes of the smoothness loss's scratch (two fp64 partial sums per workgroup; 8-byte aligned).  0 when a size is out of range. */
SCG_API size_t scg_vw_smooth_scratch_bytes(int32_t H, int32_t W);

/* C = 0: guide must be NULL.  C >= 1: guide is (C,H,W).  loss: 1 float. */
SCG_API int scg_vw_smooth_forward(int32_t H, int32_t W, int32_t C, const float* depth, const float* guide, float* loss,
                                  void* scratch, size_t scratch_bytes, void* stream);
SCG_API int scg_vw_smooth_backward(int32_t H, int32_t W, int32_t C, const float* depth, const float* guide, const float* upstream,
                                   float* d_depth, void* stream);

#ifdef __cplusplus
}
#endif
#endif

/* scg_lpips.h — C ABI of libscg_lp.so: the LPIPS metric of metrics.py:90, `lpips(render, gt, net_type='vgg')`, on the GPU
 * (csrc/lpips.hip, gfx950): the thirteen 3x3 convolutions of VGG16 on the fp32 matrix pipe and the LPIPS head, forward only, with
 * the caller's weights.
 *
 * A sixth library next to libscg_raster.so, libscg_io.so, libscg_img.so, libscg_mp.so and libscg_vw.so: its entry points are
 * declared here and in no other header.  Conventions as there: plain C, `void* stream` is a hipStream_t (NULL = the default
 * stream), every launch is asynchronous on it, return value 0 = ok, < 0 = invalid argument (the SCG_E_* codes of scg_raster.h),
 * > 0 = a hipError_t; the message of the last failure of the calling thread is scg_lp_last_error().  Every argument is validated
 * before anything touches a device.  The caller owns all buffers, scratch included; nothing is allocated, nothing is read back, so
 * a call can be captured in a graph.  No atomics anywhere: two runs are bitwise equal.
 *
 * THE RULE (lpipsPyTorch/modules/{lpips,networks,utils}.py, VGG16, version 0.1, quirks kept).  Two fp32 images x, y (3,H,W), taken
 * as they come (metrics.py feeds [0,1]; nothing is rescaled), H, W >= 16.
 *   z = (p - mean[c]) / std[c], mean = (-.030, -.088, -.188), std = (.458, .448, .450) as fp32, the division correctly rounded
 *   the first convolution pads with zeros IN THE z DOMAIN: the z-score is therefore not folded into its weights
 *   thirteen 3x3 / pad 1 / stride 1 convolutions with bias, each followed by a ReLU, channels
 *       64, 64 | 128, 128 | 256, 256, 256 | 512, 512, 512 | 512, 512, 512
 *   with a 2x2 / stride 2 max pool at each `|` in floor mode (an odd last row or column is dropped); no pool after the last
 *   taps l = 0..4 after relu1_2, relu2_2, relu3_3, relu4_3, relu5_3:  n = f / (sqrt(sum_c f^2) + 1e-10)   (all zero -> zeros)
 *   term_l = mean over the tap's pixels of sum_c lin_l[c] (n_x[c] - n_y[c])^2;  value = term_0 + ... + term_4
 * ReLU and the pool pass a NaN on (torch's do), so a NaN or infinite pixel gives a NaN value.
 *
 * PRECISION.  fp32 in and out.  A convolution sum is formed in fp32 in a FIXED order: k = (ky * 3 + kx) * cin + ci runs in chunks
 * of 32; a chunk's sum is ONE fma chain from +0 in the order 8q + j, 8q + 4 + j for q = 0..3, j = 0..3 (the two k of one
 * v_mfma_f32_32x32x2_f32, whose result is the k-ordered fmaf chain); the chunks' sums are added one after the other in chunk order
 * from +0; the bias is added last, then the ReLU.  The first layer (K = 27) runs on the vector pipe as one fmaf chain in k order.
 * No split-K, no reduced-precision operand, no Winograd, no algorithm choice.
 * The head is fp64 from the fp32 features on: the channel sums, the square root, the quotients, the weighted squared difference,
 * a wave's tree (csrc/reduce.h), the workgroups' partial sums and their fold by one workgroup in a fixed order; a term is that
 * fp64 mean rounded once, the value the fp64 sum of the five means rounded once.  (n_x - n_y)^2 is symmetric and a pixel's chain
 * does not depend on which image of the pair it belongs to: swapping x and y gives the same bits, and x == y gives exactly 0.
 *
 * LAYOUTS (the library's business, stated here).  Activations are channels-last: (n, h, w, C) fp32.  A layer's weights are
 * [cout][9 cin] with k = (ky * 3 + kx) * cin + ci contiguous, i.e. torch's (cout, cin, 3, 3) permuted to (cout, 3, 3, cin).
 * `params` of scg_lp_forward is ONE array of SCG_LP_PARAM_FLOATS floats: the thirteen weight blocks in network order, then the
 * thirteen biases, then the five linear weights (64, 128, 256, 512, 512).
 *
 * KERNELS AND LAUNCHES.  An implicit GEMM per layer, M = the pixels of both images, N = cout, K = 9 cin: a workgroup of four
 * waves owns SCG_LP_TILE_M = 128 pixels x 128 channels (x 64 where cout = 64), stages 32 k of both operands through LDS and
 * accumulates 32x32 tiles on the fp32 MFMA; bias and ReLU in the epilogue.  A layer that would have at most SCG_LP_SMALL_GRID such
 * workgroups (half the compute units of an MI355X) runs with 128 x 64 ones instead: the same sums, the same bits.  The pool is fused into the CONSUMING layer's loader
 * (the maximum of four loads), so the unpooled tap survives for the head.  One call is 13 convolution launches, one head launch
 * for all five taps (SCG_LP_HEAD_PIXELS pixels per workgroup) and one fold: 15 at any size, no reset.
 *
 * SCRATCH of scg_lp_forward, with h_0 = H, w_0 = W and h_{l+1} = h_l / 2 (floor), P_l = h_l w_l, in this order from its first byte:
 *   tap_0 (2 P_0 64), A (2 P_0 64), tap_1 (2 P_1 128), tap_2 (2 P_2 256), B (2 P_2 256), tap_3 (2 P_3 512), tap_4 (2 P_4 512)
 *   floats, then 5 ceil(P_0 / SCG_LP_HEAD_PIXELS) doubles of partial sums.  A and B hold the layers between the taps.
 * At 504 x 378 that is 0.31 GB, at 1600 x 1200 3.1 GB (one 64-channel activation of the pair alone is 983 MB).
 */
#ifndef SCG_LPIPS_H
#define SCG_LPIPS_H

#include "../scg_raster.h"

#define SCG_LP_ABI_VERSION 1
#define SCG_LP_LAYERS 13
#define SCG_LP_TAPS 5
#define SCG_LP_TILE_M 128             /* pixels of one workgroup of the convolution */
#define SCG_LP_HEAD_PIXELS 32         /* pixels of one workgroup of the head */
#define SCG_LP_SMALL_GRID 128          /* a layer with at most this many 128 x 128 workgroups runs with 128 x 64 ones */
#define SCG_LP_MIN_DIM 16             /* H and W of scg_lp_forward: below it a pool has nothing to pool */
#define SCG_LP_MAX_DIM 16384          /* h and w */
#define SCG_LP_MAX_PIXELS 16777216    /* h * w of one image */
#define SCG_LP_MAX_BATCH 2            /* n of scg_lp_conv3x3 */
#define SCG_LP_PARAM_FLOATS 14716160  /* 9 * 1634496 weights + 4224 biases + 1472 linear weights */
#define SCG_LP_RELU 1                 /* flags of scg_lp_conv3x3 */
#define SCG_LP_POOL 2                 /* the input is max-pooled 2x2 (floor) first: out is (n, h / 2, w / 2, cout); cin >= 64 */
#define SCG_LP_ZSCORE 4               /* the input is z-scored first, padding zero in the z domain; cin = 3 */

#ifdef __cplusplus
extern "C" {
#endif

SCG_API const char* scg_lp_last_error(void);
SCG_API int32_t scg_lp_abi_version(void);

/* Bytes of scg_lp_forward's scratch (the arithmetic above); 0 when a size is out of range. */
SCG_API size_t scg_lp_scratch_bytes(int32_t H, int32_t W);

/* Floats of the optional feature output: sum over the taps of 2 P_l C_l; 0 when a size is out of range. */
SCG_API size_t scg_lp_feature_floats(int32_t H, int32_t W);

/* One layer on its own: in (n, h, w, cin), weights [cout][9 cin], bias [cout], out (n, h', w', cout) with h' = h, w' = w, or
 * h / 2, w / 2 under SCG_LP_POOL.  (cin, cout) is one of the network's eight pairs: (3,64) (64,64) (64,128) (128,128) (128,256)
 * (256,256) (256,512) (512,512).  1 <= n <= SCG_LP_MAX_BATCH; h, w >= 1 (>= 2 under SCG_LP_POOL).  All pointers 16-byte aligned. */
SCG_API int scg_lp_conv3x3(int32_t n, int32_t cin, int32_t cout, int32_t h, int32_t w, const float* in, const float* weights,
                           const float* bias, float* out, int32_t flags, void* stream);

/* x, y: (3,H,W) planar.  value: 1 float, terms: 5 floats.  features: NULL, or scg_lp_feature_floats(H, W) floats that receive the
 * normalised maps, tap by tap, each (2, h_l, w_l, C_l) with x's first.  params, features and scratch 16-byte aligned. */
SCG_API int scg_lp_forward(int32_t H, int32_t W, const float* x, const float* y, const float* params, float* value, float* terms,
                           float* features, void* scratch, size_t scratch_bytes, void* stream);

/* The head and the fold alone (2 launches), on the taps that a scg_lp_forward of the same H, W left in `scratch`: the same value,
 * terms and features, bit for bit.  For timing and for reading the features after a call. */
SCG_API int scg_lp_head(int32_t H, int32_t W, const float* params, float* value, float* terms, float* features, void* scratch,
                        size_t scratch_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif

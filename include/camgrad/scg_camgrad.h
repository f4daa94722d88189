/* scg_camgrad.h — C ABI of libscg_camgrad.so: the rasterizer's gradient with respect to the CAMERA (camgrad.hip in csrc/, gfx950):
 * dL/dviewmatrix, dL/dprojmatrix and dL/dcampos of one view from the per-Gaussian gradient records its blend backward left.
 *
 * A side library (build.SIDE_LIBRARIES "camgrad").  Conventions as in
 * the other libraries: plain C, pointers and scalars only, `void* stream` is a hipStream_t (NULL = the default stream), every launch
 * is asynchronous on it, return value 0 = ok, < 0 = invalid argument (the SCG_E_* codes of scg_raster.h), > 0 = a hipError_t; the
 * message of the last failure of the calling thread is scg_camgrad_last_error().  Every argument is validated before anything touches
 * a device.  The caller owns all buffers: nothing is allocated, nothing is read back, nothing is synchronised (the call can be
 * captured in a graph), no atomics of any kind; two runs on the same inputs give the same bits.
 *
 * THE RULE (tests/camgrad_refs.py restates it in fp64 numpy), in the notation of geometry_backward_one (csrc/geometry.hip).
 *
 * The matrices are flat and transposed as everywhere here: t = [x y z 1] . V means t_i = sum_j V[4j+i] pos[j], pos = (x, y, z, 1);
 * h = [x y z 1] . PM likewise.  Only a Gaussian with radii[i] > 0 contributes.  Its record (SCG_DSPLAT_FLOATS floats, raw sums of
 * the blend backward) is turned into dL/dxy, dL/dconic and dL/ddepth, and the forward chain (project, cov3D, cov2D) is recomputed
 * from its inputs exactly as the geometry kernels recompute it (csrc/geometry_math.h), which gives dtx, dty, dtz (dtz includes
 * dL/ddepth), dT0[3], dT1[3] (the gradient of Tm = J . Wm) and dndc_x, dndc_y.  Then
 *   dV[4j+0] += dtx pos[j]      dV[4j+1] += dty pos[j]      dV[4j+2] += dtz pos[j]                                 j = 0..3
 *   dV[4k+0] += dT0[k] J00      dV[4k+1] += dT1[k] J11      dV[4k+2] += dT0[k] J02 + dT1[k] J12                    k = 0..2
 *   dPM[4j+0] += dndc_x m_w pos[j]      dPM[4j+1] += dndc_y m_w pos[j]
 *   dPM[4j+3] += -(hx dndc_x + hy dndc_y) m_w^2 pos[j]                                                             j = 0..3
 *   dcampos  -= (g - dir (dir . g)) / |mean - campos|,   g = sum_k (sh_k . dRGB) dbasis_k/ddir,   dir = (mean - campos) / |.|
 * with the oracle's decisions: a view-space component under an active 1.3 tanfov clamp is a constant (D2: dtx / dty are zero
 * there, J02 / J12 keep the clamped value), the cull is view z <= 0.2 only (D3: it is in radii already).  dRGB is the record's
 * dL/drgb with the channels zeroed whose forward colour was clamped at 0; the clamp is RECOMPUTED (eval_sh of csrc/sh_eval.h at the
 * forward's direction, + 0.5, < 0): no workspace of the forward is read.  dcampos is zero with colors_precomp and at degree 0.
 * The fourth column of V (V[4j+3]) and the third of PM (PM[4j+2]) are never read by the rasterizer: their gradients are exact
 * zeros.  That leaves SCG_CAMGRAD_SUMS = 12 + 12 + 3 live sums over the Gaussians.
 * The host scalars are formed as the rasterizer forms them: focal = (float)size / (2.0f * tanfov), lim = 1.3f * tanfov.
 *
 * THE CALL: two launches.
 *   1  one thread per Gaussian, workgroups of SCG_CAMGRAD_BLOCK threads.  A thread loads its inputs, its record and its radius
 *      up front, forms its 27 contributions (zeros when it has no visible Gaussian), and the workgroup reduces each in the fixed
 *      order of csrc/reduce.h (a shuffle tree over the offsets 32 .. 1 inside a wave, then the waves folded left to right) into
 *      partials[block][SCG_CAMGRAD_SUMS].  A wave without a visible Gaussian skips the arithmetic, not the barriers.
 *   2  ONE workgroup folds the partials in fp64: the blocks are cut into 32 consecutive runs, each summed in block order, the
 *      32 sums folded in run order; one rounding to fp32; all SCG_CAMGRAD_OUT_FLOATS outputs are written (the dead ones as 0).
 * out: dV as (4,4) flat [0, 16), dPM [16, 32), dcampos [32, 35).
 */
#ifndef SCG_CAMGRAD_H
#define SCG_CAMGRAD_H

#include "../scg_raster.h"

#define SCG_CAMGRAD_ABI_VERSION 2
#define SCG_CAMGRAD_BLOCK 256             /* Gaussians (threads) of a workgroup of the first launch */
#define SCG_CAMGRAD_SUMS 27               /* live sums: floats of one workgroup's partial record */
#define SCG_CAMGRAD_OUT_FLOATS 35         /* dV (16) | dPM (16) | dcampos (3) */
#define SCG_CAMGRAD_MAX_DIM 1048560       /* H and W: 65535 tiles, as the rasterizer */
#define SCG_CAMGRAD_NO_CAMPOS 1           /* flags: dL/dcampos is not wanted: the SH records are not read, out[32..35) = 0 */

#ifdef __cplusplus
extern "C" {
#endif

SCG_API const char* scg_camgrad_last_error(void);
SCG_API int32_t scg_camgrad_abi_version(void);

/* Host only.  The workgroups of the first launch for P >= 0 Gaussians and the bytes of `partials` (0 for P = 0). */
SCG_API int scg_camgrad_sizes(int32_t P, int32_t* n_blocks, uint64_t* partial_bytes);

/* The operator's inputs as scg_geometry_backward takes them (activated values; exactly one of shs | colors_precomp and of
 * scales + rotations | cov3D_precomp; rotations 16-byte aligned; M = SH coefficients per Gaussian, at least (sh_degree + 1)^2
 * with shs), radii (P) as the forward wrote them, dsplats (P, SCG_DSPLAT_FLOATS) as the blend backward left them (16-byte aligned),
 * view / proj (16 floats) and campos (3) in device memory, partials of scg_camgrad_sizes' bytes (4-byte aligned; every word the
 * second launch reads is written by the first: fresh or reused, never cleared), out35 (SCG_CAMGRAD_OUT_FLOATS floats).  With P = 0
 * the per-Gaussian pointers and partials are ignored and out35 receives zeros. */
SCG_API int scg_camgrad_backward(int32_t H, int32_t W, float tanfovx, float tanfovy, float scale_modifier, int32_t sh_degree,
                                 int32_t M, int32_t P, const float* view, const float* proj, const float* campos,
                                 const float* means3D, const float* opacities, const float* shs, const float* colors_precomp,
                                 const float* scales, const float* rotations, const float* cov3D_precomp, const int32_t* radii,
                                 const float* dsplats, float* partials, float* out35, int32_t flags, void* stream);

/* The same with the reference model's raw parameter tensors (ScgModel of scg_raster.h: SH colours, scale + rotation covariance,
 * M = 16; P must equal model->ray.count + model->bg.count; the activations are the geometry kernels' own device functions). */
SCG_API int scg_camgrad_backward_model(int32_t H, int32_t W, float tanfovx, float tanfovy, float scale_modifier, int32_t sh_degree,
                                       int32_t P, const float* view, const float* proj, const float* campos, const ScgModel* model,
                                       const int32_t* radii, const float* dsplats, float* partials, float* out35, int32_t flags,
                                       void* stream);

#ifdef __cplusplus
}
#endif
#endif

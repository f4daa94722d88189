/* scg_matchloss.h — C ABI of the fused depth-consumer step.
 *
 * The reference's GaussianModel.get_matchloss_from_renderdepth (scene/gaussian_model.py:241-282), called every
 * training iteration on the rasterizer's depth output (train.py:164): for each matched view pair, bilinear-sample
 * the rendered depth at the <= 2000 match pixels of view 0, lift them along their rays, project into view 1 and
 * take the normalised L1 distance to the matched pixels, averaged over the matches that project inside the image
 * and are valid in both masks.  In the reference this is ~30 small torch kernels per pair and as many again in
 * backward; here it is ONE kernel per pair that also produces the gradient w.r.t. the depth image (the only
 * differentiable input), scattered to the four bilinear taps of every match.
 *
 * Same conventions as scg_raster.h (caller-owned device buffers, stream-ordered, int status). */
#ifndef SCG_MATCHLOSS_H
#define SCG_MATCHLOSS_H

#include <stdint.h>

/* The library is built with -fvisibility=hidden: exactly the entry points declared in the headers under include/ are exported. */
#ifndef SCG_API
#define SCG_API __attribute__((visibility("default")))
#endif

#ifdef __cplusplus
extern "C" {
#endif

/* One view pair.
 *   depth (H,W) fp32                      rendered depth of view 0 (rasterizer output, squeezed)
 *   uv0 (M,2)                             match pixels in view 0            (:253 match_data["uv"])
 *   rays_o (M,3), rays_d (M,3)            world-space rays of those pixels  (:261)
 *   cam_rays_d (M,3)                      camera-space ray directions; only .z is used (:262)
 *   mask0, mask1 (M) or NULL              blender masks of both views; valid = mask0*mask1 > 0 (:249-251)
 *   intr1 (3,3), w2c1 (4,4) row-major     intrinsics / world-to-camera of view 1 (:265)
 *   uv1 (M,2)                             matched pixels in view 1          (:273)
 *   width, height                         normalisation and in-image test   (:244,:271,:277)
 * Outputs (both ACCUMULATED, the caller zeroes them once per view):
 *   loss (1)            += sum_i(l_i m_i) / (sum_i m_i + 1e-8)
 *   grad_depth (H,W)    += d(that term)/d(depth), or NULL when no gradient is needed */
SCG_API int scg_match_loss_pair(const float* depth, int32_t H, int32_t W, const float* uv0, const float* rays_o,
                        const float* rays_d, const float* cam_rays_d, const float* mask0, const float* mask1,
                        const float* intr1, const float* w2c1, const float* uv1, int32_t M, float width, float height,
                        float* loss, float* grad_depth, void* stream);

/* ---- The ray-depth init stage (train.py:49-95 of the reference) ------------------------------------------------------------
 *
 * 2 000 Adam iterations on the per-match ray depths z_val against GaussianModel.get_matchloss_from_base
 * (scene/gaussian_model.py:175-239), keeping for every match the depth at which its own loss term was smallest.  Once the
 * number of valid matches of a view pair is known every match is independent of every other, so one thread carries one match
 * through n_steps consecutive iterations in registers: loss term, gradient, best-state rule, one Adam step.
 *
 * One flat arena over all ORDERED view pairs (a -> b), N = sum of their match counts.  Per element:
 *   rays_o (N,3), rays_d (N,3)   the ray of the match in view a
 *   uv_t (N,2)                   the matched pixel in the target view b (8-byte aligned)
 *   wgt (N)                      1 / (valid matches of the pair) where mask_a * mask_b > 0, else 0 (all 0 for a pair without
 *                                a valid match: its elements get no gradient and never move)
 * State, fp32 (N) each: z, exp_avg, exp_avg_sq, best_z, min_loss.
 * Per ordered pair one ScgInitSegment of a DEVICE table (any number of them; every element lies in exactly one). */
typedef struct ScgInitSegment {
    int32_t offset;              /* first element */
    int32_t count;               /* matches of this ordered pair */
    float width, height;         /* the normalisation (the reference takes them from the earlier view of the pair) */
    float intr[9];               /* intrinsics of the target view b, row-major */
    float w2c[12];               /* first three rows of its world-to-camera matrix, row-major */
} ScgInitSegment;

#define SCG_INIT_STAGE_MAX_STEPS 4096

/* Per element and iteration (global index it = first_iter + k, k < n_steps):
 *   (X,Y,Z) = K_b (R_b (o + d z) + t_b);  px = X / (Z + 1e-8);  py = Y / (Z + 1e-8)
 *   ml = 0.5 (|px - u| / width + |py - v| / height)           the unmasked loss_state entry
 *   g  = loss_scale * wgt * d ml / d z                         (sign(0) = 0)
 *   it == 0: min_loss = ml, and best_z = z AFTER this iteration's step (the reference's best state aliases the parameter
 *            through the first step); it == 1: min_loss = min_loss < ml ? min_loss : ml, best_z untouched;
 *   it >= 2: best_z = min_loss < ml ? best_z : z (before the step), then min_loss as for it == 1.  A NaN on either side takes
 *            the current value, as torch.where does.
 *   one Adam step (torch's single-tensor order, betas (beta1, beta2), eps, learning rate lr, step count it + 1).
 * n_steps >= 1 (run): inputs are read once, the five state arrays are written once.  partials, when not NULL, receives for every
 *   iteration k and workgroup w the sum of wgt * ml over the workgroup's elements, at partials[k * W + w], in a fixed order (no
 *   atomics: bitwise reproducible); the sum of row k is the reference's match loss of that iteration (without the NaN of a
 *   pair that has no valid match: the caller knows its counts).  loss_state and grad are not used.
 * n_steps == 0 (evaluate): writes loss_state (N) = ml and grad (N) = g where not NULL, and one row of partials; changes no state
 *   (exp_avg, exp_avg_sq, best_z and min_loss may be NULL).
 * partials_bytes must be at least scg_init_stage_partials_bytes(N, n_steps) = max(n_steps, 1) * W * 4. */
SCG_API size_t scg_init_stage_partials_bytes(int32_t N, int32_t n_steps);   /* 0 for arguments out of range */
SCG_API int scg_init_stage_run(const ScgInitSegment* segments, int32_t nseg, int32_t N, const float* rays_o,
                       const float* rays_d, const float* uv_t, const float* wgt, float* z, float* exp_avg,
                       float* exp_avg_sq, float* best_z, float* min_loss, int32_t first_iter, int32_t n_steps, double lr,
                       double beta1, double beta2, double eps, float loss_scale, float* loss_state, float* grad,
                       float* partials, size_t partials_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SCG_MATCHLOSS_H */

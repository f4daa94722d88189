// sh_eval.h — the SH colour polynomial, once: the rasterizer's geometry kernels (geometry.hip) and the colour cloud of the scene
// files (plypack.hip) evaluate the same text, so a viewer's colours are the renderer's.  Include it inside a translation unit
// that is compiled with contraction off (both are: -ffp-contract=off and `#pragma clang fp contract(off)`).
#pragma once

#include <hip/hip_runtime.h>

namespace scg {

__constant__ const float kC0 = 0.28209479177387814f;
__constant__ const float kC1 = 0.4886025119029199f;
__constant__ const float kC2[5] = {1.0925484305920792f, -1.0925484305920792f, 0.31539156525252005f,
                                   -1.0925484305920792f, 0.5462742152960396f};
__constant__ const float kC3[7] = {-0.5900435899266435f, 2.890611442640554f, -0.4570457994644658f,
                                   0.3731763325901154f, -0.4570457994644658f, 1.445305721320277f,
                                   -0.5900435899266435f};

// rgb = eval_sh(deg, sh, dir) in the operation order of oracle eval_sh_rgb (== utils/sh_utils.py:57-103).
template <int DEG>
__device__ __forceinline__ void eval_sh(const float* sh, float x, float y, float z, float* rgb) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float res = kC0 * sh[c];
        if (DEG > 0) {
            res = res - (kC1 * y) * sh[3 + c] + (kC1 * z) * sh[6 + c] - (kC1 * x) * sh[9 + c];
            if (DEG > 1) {
                const float xx = x * x, yy = y * y, zz = z * z;
                const float xy = x * y, yz = y * z, xz = x * z;
                res = res + (kC2[0] * xy) * sh[12 + c] + (kC2[1] * yz) * sh[15 + c] +
                      (kC2[2] * (2.0f * zz - xx - yy)) * sh[18 + c] + (kC2[3] * xz) * sh[21 + c] +
                      (kC2[4] * (xx - yy)) * sh[24 + c];
                if (DEG > 2) {
                    res = res + ((kC3[0] * y) * (3.0f * xx - yy)) * sh[27 + c] +
                          ((kC3[1] * xy) * z) * sh[30 + c] +
                          ((kC3[2] * y) * (4.0f * zz - xx - yy)) * sh[33 + c] +
                          ((kC3[3] * z) * (2.0f * zz - 3.0f * xx - 3.0f * yy)) * sh[36 + c] +
                          ((kC3[4] * x) * (4.0f * zz - xx - yy)) * sh[39 + c] +
                          ((kC3[5] * z) * (xx - yy)) * sh[42 + c] +
                          ((kC3[6] * x) * (xx - 3.0f * yy)) * sh[45 + c];
                }
            }
        }
        rgb[c] = res;
    }
}

}  // namespace scg

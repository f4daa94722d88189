// adam_math.h — one element of torch's single-tensor Adam (weight_decay 0, no amsgrad, no maximize), shared by optim.hip and
// initstage.hip.  Both are compiled with -ffp-contract=off: fp32 throughout, torch's order of operations, one rounding per
// operation.  That is the contract (tests/optim_refs.py restates it bit for bit); torch's own bits may differ in the last place
// where torch fuses, as its lerp does.
#pragma once

#include <hip/hip_runtime.h>

namespace scg {

struct AdamCoef {
    float w1, b2f, w2, eps, bc2s, nss;    // nss = -(lr / bc1) as fp32
};

// The two step-dependent coefficients of step t (counted from 1), as torch forms them: Python floats (double), then fp32
__device__ __forceinline__ void adam_bias_coefs(double b1, double b2, double lr, double t, float& bc2s, float& nss) {
    const double bc1 = 1.0 - pow(b1, t);
    const double bc2 = 1.0 - pow(b2, t);
    bc2s = (float)sqrt(bc2);
    nss = (float)(-(lr / bc1));
}

// torch's order: exp_avg.lerp_(g, 1-b1); exp_avg_sq.mul_(b2).addcmul_(g, g, 1-b2);
// denom = exp_avg_sq.sqrt() / sqrt(bc2) + eps; param.addcdiv_(exp_avg, denom, -lr/bc1)
__device__ __forceinline__ void adam_update(float& p, float& m, float& v, float g, const AdamCoef& c) {
    m = m + c.w1 * (g - m);                       // lerp with a weight < 0.5
    v = v * c.b2f + c.w2 * g * g;
    const float denom = sqrtf(v) / c.bc2s + c.eps;
    p = p + c.nss * (m / denom);
}

}  // namespace scg

// pixel_rules.h — how a float becomes a byte of an image (evalview.hip, depthviz.hip; the clamp also in dtumask.hip).  The PNGs of
// render_set and the frames of render_video are compared byte for byte across those files: the rules exist once, here.
// include/scg_eval.h states the quantiser, include/scg_viz.h the video byte.
#pragma once

#include "scg_common.h"

namespace scg {

// torch.clamp(v, 0, 1) (render_video.py:132, train.py:253-254): a NaN stays a NaN
__device__ __forceinline__ float unit_clamp(float v) { return v < 0.f ? 0.f : (v > 1.f ? 1.f : v); }

// torchvision.utils.save_image's quantiser (the calls of render.py:150-156 and render_video.py:139-140; metrics.py:26-47 reads the
// PNGs back): mul(255).add_(0.5).clamp_(0, 255).to(uint8), every operator rounded on its own, so
// q(x) = trunc(clamp(fl(fl(x * 255) + 0.5), 0, 255)); q(NaN) = 0 (torch leaves that cast undefined)
__device__ __forceinline__ uint32_t quantise(float x) {
#pragma clang fp contract(off)                         // two roundings, whatever the including file is compiled with
    const float v = x * 255.f + 0.5f;
    if (!(v >= 0.f)) return 0u;                        // below the clamp, and NaN
    return v >= 255.f ? 255u : (uint32_t)v;            // the cast truncates
}

// render_video.py:148: the truncating cast of clamp(r) * 255.; NaN -> 0
__device__ __forceinline__ uint32_t video_byte(float r) {
    const float v = unit_clamp(r) * 255.f;
    return v != v ? 0u : (uint32_t)v;
}

}  // namespace scg

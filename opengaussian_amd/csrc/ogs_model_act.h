// Activations of the reference model's raw parameters (scene/gaussian_model.py:122-169: get_scaling = exp, get_rotation =
// F.normalize, get_opacity = sigmoid, get_features = cat(dc, rest)) and their chain rules, as device functions.  ONE place:
// the raw forms of the per-Gaussian kernels (preprocess_fwd.hip, preprocess_bwd.hip) and the stand-alone ogs_model_activate
// kernel all go through these, so a raw pass and the existing pass fed by ogs_model_activate see the same bits.
//
// Plain IEEE fp32: expf / sqrtf / division as the library gives them (no __expf, no rcp), and no contraction into FMAs
// whatever the including file is compiled with -- the sum of squares of the norm must come out the same in every kernel.
#pragma once

#include <hip/hip_runtime.h>

#include "../../include/ogs_model.h"

namespace ogs {

constexpr float kNormalizeEps = 1e-12f;         // F.normalize's eps: q / max(|q|, eps)

// A value the optimiser cannot see through.  The raw form of preprocess_backward_kernel puts its activated inputs and the
// gradients it hands to the chain rule through this, so that the arithmetic in between is compiled on its own, not fused or
// re-associated with the activation code around it: dL/dscale of a large Gaussian is a difference of terms 1e3 times its size,
// and two differently contracted fp32 evaluations of it were measured 2.5e-4 of the family maximum apart.
__device__ __forceinline__ float opaque(float v) {
    asm volatile("" : "+v"(v));
    return v;
}

__device__ __forceinline__ float act_scale(float s) { return expf(s); }

__device__ __forceinline__ float act_opacity(float o) {
#pragma clang fp contract(off)
    return 1.0f / (1.0f + expf(-o));
}

__device__ __forceinline__ float quat_norm(float4 q) {
#pragma clang fp contract(off)
    return sqrtf(q.x * q.x + q.y * q.y + q.z * q.z + q.w * q.w);
}

// q / max(|q|, eps); `norm` = quat_norm(q)
__device__ __forceinline__ float4 act_rotation(float4 q, float norm) {
    const float d = fmaxf(norm, kNormalizeEps);
    return make_float4(q.x / d, q.y / d, q.z / d, q.w / d);
}

// SH coefficient k, channel c of one Gaussian as flat index i = 3 k + c: row 0 lives in features_dc [P,1,3], rows 1..M-1 in
// features_rest [P,M-1,3].  `i` is a compile-time constant wherever the callers unroll, so the select folds away.
struct RawShRow {
    const float* dc;        // this Gaussian's 3 floats
    const float* rest;      // this Gaussian's 3 (M - 1) floats (never dereferenced when M == 1)
    __device__ __forceinline__ float operator[](int i) const { return i < 3 ? dc[i] : rest[i - 3]; }
};
__device__ __forceinline__ RawShRow raw_sh_row(const float* features_dc, const float* features_rest, int idx, int M) {
    return RawShRow{features_dc + (size_t)idx * 3, features_rest + (size_t)idx * (size_t)(M - 1) * 3};
}

// ---- chain rules: gradient w.r.t. the activated value -> gradient w.r.t. the raw parameter -------------------------------
__device__ __forceinline__ float act_scale_bwd(float g, float scale) { return g * scale; }

__device__ __forceinline__ float act_opacity_bwd(float g, float sigma) {
#pragma clang fp contract(off)
    return g * (sigma * (1.0f - sigma));
}

// qhat = act_rotation(q, norm).  |q| >= eps: (g - qhat (qhat . g)) / |q|; below: g / eps (the denominator is the constant
// clamp_min chose, which is what autograd differentiates)
__device__ __forceinline__ float4 act_rotation_bwd(float4 g, float4 qhat, float norm) {
#pragma clang fp contract(off)
    if (norm >= kNormalizeEps) {
        const float d = qhat.x * g.x + qhat.y * g.y + qhat.z * g.z + qhat.w * g.w;
        return make_float4((g.x - qhat.x * d) / norm, (g.y - qhat.y * d) / norm, (g.z - qhat.z * d) / norm,
                           (g.w - qhat.w * d) / norm);
    }
    return make_float4(g.x / kNormalizeEps, g.y / kNormalizeEps, g.z / kNormalizeEps, g.w / kNormalizeEps);
}

}  // namespace ogs

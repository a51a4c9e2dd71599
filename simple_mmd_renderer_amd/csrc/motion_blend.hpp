// motion_blend.hpp -- the cross-fade between two clips of a motion set (mmdx_motion_set_blend_*_time,
// mmdx_skeleton_solve_motion_set_blend_time): the device operands of a call and the blend itself, shared by the bone kernels
// (rig_kernels.hip) and the morph kernel (kernels.hip).  Both translation units are built with -ffp-contract=off, so every
// product below stays a separate rounding.  The two rows that are blended come from eval_bone_pose / eval_morph_rate unchanged;
// the only arithmetic of the feature is in blend_pose / blend_rate.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace mmdx {

// every array [ni], device memory
struct BlendOperands {
    const uint32_t *clips_a, *clips_b;          // ids >= n_clips (MMDX_CLIP_NONE included) play nothing
    const double *times_a, *times_b;            // seconds
    const float *weights;                       // 0 = a, 1 = b
    uint32_t n_clips;
};

// NLerpProxy::operator[]'s short circuits (L/util/math_impl.inl:1265-1269), applied to the whole row and closed over NaN:
// anything that is not >= eps is A.  Only a kBlendMix row evaluates both clips.
enum : uint32_t { kBlendA = 0, kBlendB = 1, kBlendMix = 2 };
__device__ __forceinline__ uint32_t blend_side(float w) {
    if (!(w >= 1e-7f)) return kBlendA;
    if (w > 1.0f - 1e-7f) return kBlendB;
    return kBlendMix;
}

// (t, q) = A on entry, the blended pose on return; w is a kBlendMix weight.
//   translation: l*(1-lambda) + r*lambda per channel, L/motion/motion_impl.inl:364-372
//   rotation:    the middle branch of NLerp(l, r)[lambda], L/util/math_impl.inl:1271-1275, with Vector4D::Normalize's
//                1 / float(sqrt(double(sum))) (math_impl.inl:717-728) -- as between two keys in eval_bone_pose
__device__ __forceinline__ void blend_pose(float4 &t, float4 &q, const float4 tb, const float4 qb, const float w) {
    t.x = t.x * (1.0f - w) + tb.x * w;
    t.y = t.y * (1.0f - w) + tb.y * w;
    t.z = t.z * (1.0f - w) + tb.z * w;
    t.w = 0.f;
    const float dot = q.x * qb.x + q.y * qb.y + q.z * qb.z + q.w * qb.w;
    const float a = 1.0f - w;
    float4 v;
    if (dot < 0.0f) {
        v = make_float4(a * q.x - w * qb.x, a * q.y - w * qb.y, a * q.z - w * qb.z, a * q.w - w * qb.w);
    } else {
        v = make_float4(a * q.x + w * qb.x, a * q.y + w * qb.y, a * q.z + w * qb.z, a * q.w + w * qb.w);
    }
    const float s = v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w;
    const float n = 1.0f / float(sqrt(double(s)));
    q = make_float4(v.x * n, v.y * n, v.z * n, v.w * n);
}

// morph rate: l*(1-lambda) + r*lambda, L/motion/motion_impl.inl:462
__device__ __forceinline__ float blend_rate(const float a, const float b, const float w) { return a * (1.0f - w) + b * w; }

}  // namespace mmdx

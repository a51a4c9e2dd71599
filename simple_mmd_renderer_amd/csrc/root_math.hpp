// root_math.hpp -- the arithmetic of mmdx_animator_root_motion (include/mmdx.h states it), once: the gfx950 kernel
// (animator_root_motion_kernel in rig_kernels.hip) and a CPU driver (tests/root_math_driver.cpp) compile these same lines, and
// tests/root_motion_ref.py restates them in numpy.  IEEE operations only, binary32 in the order written (the clocks are
// anim_math.hpp's, in double); both builds pass -ffp-contract=off, so nothing is fused.
// What is NOT here is called, not restated: the clock of a side is anim_wrap (anim_math.hpp), the heading's matrix is
// place_matrix_from_pose (place_math.hpp), the blend of the two sides is motion_blend.hpp's blend_side / blend_rate -- device-only
// functions, so root_blend takes the side and the rate function from its caller -- and R(c, t), the root bone's translation, is
// eval_bone_pose in the kernel and Motion::GetBonePose in the golden rows.
#pragma once

#include <cstdint>

#include "anim_math.hpp"
#include "place_math.hpp"

#if defined(__HIPCC__)
#define MMDX_ROOT_FN __host__ __device__ __forceinline__
#else
#define MMDX_ROOT_FN inline
#endif

namespace mmdx {

// the values of MMDX_ROOT_X / _Y / _Z of include/mmdx.h (anim_api.cpp asserts they agree)
enum : uint32_t { kRootX = 1u, kRootY = 2u, kRootZ = 4u };
// the four instants of one side, in the order of the kernel's lanes
enum : uint32_t { kRootT0 = 0, kRootT1 = 1, kRootNear = 2, kRootFar = 3 };
// the values of motion_blend.hpp's kBlendA / kBlendB / kBlendMix (rig_kernels.hip asserts they agree)
enum : uint32_t { kRootSideA = 0, kRootSideB = 1, kRootSideMix = 2 };

struct RootVec {
    float x, y, z;
};

// libmmd's Vector3D operator- and operator+: per component
MMDX_ROOT_FN RootVec root_sub(const RootVec a, const RootVec b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
MMDX_ROOT_FN RootVec root_add(const RootVec a, const RootVec b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }

// Step 2, the clocks: where a side (clip c at t0) is sampled for a step of s seconds.  near / far are the two ends of the loop seam
// the step crossed and mean something only when `folded`; a fold implies c < n_clips (anim_wrap folds only a looping clip).
struct RootTimes {
    double t0, t1, near, far;
    uint32_t folded;
};
MMDX_ROOT_FN RootTimes root_times(const AnimClips &k, uint32_t c, double t0, double s) {
    RootTimes r;
    const double raw = t0 + s;
    r.t0 = t0;
    r.t1 = anim_wrap(k, c, raw, &r.folded);
    r.near = 0.0;
    r.far = 0.0;
    if (r.folded) {
        const double L = k.length[c];
        if (raw >= L) r.near = L;               // forwards: up to the end, then on from the start
        else r.far = L;                         // a negative step: down to the start, then on from the end
    }
    return r;
}
// the instant `which` (kRootT0 ...) of a side; selects, so a lane's own `which` costs no indexed array
MMDX_ROOT_FN double root_time_of(const RootTimes &r, uint32_t which) {
    return which == kRootT0 ? r.t0 : which == kRootT1 ? r.t1 : which == kRootNear ? r.near : r.far;
}

// Step 2, the displacement of a side from R at its four instants (r_near / r_far are not looked at without a fold)
MMDX_ROOT_FN RootVec root_displacement(const RootVec r_t0, const RootVec r_t1, const RootVec r_near, const RootVec r_far, uint32_t folded) {
    if (!folded) return root_sub(r_t1, r_t0);
    return root_add(root_sub(r_near, r_t0), root_sub(r_t1, r_far));
}

// Step 4: `side` is blend_side(w), `rate` is blend_rate (motion_blend.hpp); an end-point row is that side's displacement unchanged
template <class Rate>
MMDX_ROOT_FN RootVec root_blend(const RootVec da, const RootVec db, uint32_t side, float w, Rate rate) {
    if (side == kRootSideA) return da;
    if (side == kRootSideB) return db;
    return {rate(da.x, db.x, w), rate(da.y, db.y, w), rate(da.z, db.z, w)};
}

// Step 5: a component whose bit is absent becomes +0.0f (a select: -0, NaN and infinity do not leak through a multiply)
MMDX_ROOT_FN RootVec root_mask(const RootVec d, uint32_t axes) {
    return {(axes & kRootX) ? d.x : 0.0f, (axes & kRootY) ? d.y : 0.0f, (axes & kRootZ) ? d.z : 0.0f};
}

// Step 6: pose = one placement {tx, ty, tz, (untouched), qx, qy, qz, qw}; d rotated by the heading -- libmmd's
// rotate(Vector3D, Matrix4x4), L/util/math_impl.inl:1032-1038, three-term sums left to right -- is added to pose[0..2].
// pose[3] is neither read nor written.
MMDX_ROOT_FN void root_accumulate(const RootVec d, float *pose) {
    float m[16];
    place_matrix_from_pose(pose, m);
    const float rx = d.x * m[0] + d.y * m[4] + d.z * m[8];
    const float ry = d.x * m[1] + d.y * m[5] + d.z * m[9];
    const float rz = d.x * m[2] + d.y * m[6] + d.z * m[10];
    pose[0] = pose[0] + rx;
    pose[1] = pose[1] + ry;
    pose[2] = pose[2] + rz;
}

}  // namespace mmdx

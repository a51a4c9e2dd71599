// root_math.hpp -- the arithmetic of mmdx_animator_root_motion and, in the second half, of mmdx_animator_root_motion_turn
// (include/mmdx.h states both), once: the gfx950 kernel
// (animator_root_motion_kernel in rig_kernels.hip) and a CPU driver (tests/root_math_driver.cpp) compile these same lines, and
// tests/root_motion_ref.py restates them in numpy.  IEEE operations only, binary32 in the order written (the clocks are
// anim_math.hpp's, in double); both builds pass -ffp-contract=off, so nothing is fused.
// What is NOT here is called, not restated: the clock of a side is anim_wrap (anim_math.hpp), the heading's matrix is
// place_matrix_from_pose (place_math.hpp), the blend of the two sides is motion_blend.hpp's blend_side / blend_rate -- device-only
// functions, so root_blend takes the side and the rate function from its caller -- and R(c, t), the root bone's translation, is
// eval_bone_pose in the kernel and Motion::GetBonePose in the golden rows.
#pragma once

#include <cmath>
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

// ---- root motion that turns (mmdx_animator_root_motion_turn; include/mmdx.h states it) -------------------------------------------
// The same clocks, sides, blend rows and axes select as above; a side is now a pair (D, dq) -- the root's displacement in its own
// frame at t0 and its rotation delta -- and the placement's heading is multiplied by the blended delta.  The kernel
// (animator_root_turn_kernel in rig_kernels.hip) and tests/root_turn_math_driver.cpp compile these lines, tests/root_turn_ref.py
// restates them.  rig_kernels.hip's q_mul / q_inverse are device-only and local to that translation unit, so the three quaternion
// operations are restated here as root_sub is; the blend of two pairs is motion_blend.hpp's blend_pose, passed in by the caller.
struct RootQuat {
    float x, y, z, w;                            // libmmd's i, j, k, e
};
struct RootDelta {
    RootVec d;
    RootQuat q;
};

// Quaternion::operator*(const Quaternion &), L/util/math_impl.inl:510-517.  M(a * b) = M(b) * M(a) in the row-vector convention.
MMDX_ROOT_FN RootQuat root_q_mul(const RootQuat a, const RootQuat q) {
    RootQuat r;
    r.x = (a.w * q.x + a.x * q.w + a.y * q.z) - a.z * q.y;
    r.y = (a.w * q.y + a.y * q.w + a.z * q.x) - a.x * q.z;
    r.z = (a.w * q.z + a.x * q.y + a.z * q.w) - a.y * q.x;
    r.w = a.w * q.w - (a.x * q.x + a.y * q.y + a.z * q.z);
    return r;
}
// Quaternion::Inverse, :474-477: Conjugate() (:466-473) * (1 / the squared norm, summed left to right) (operator*(elem_type), :486-493)
MMDX_ROOT_FN RootQuat root_q_inverse(const RootQuat a) {
    const float n = 1.0f / (a.x * a.x + a.y * a.y + a.z * a.z + a.w * a.w);
    return {-a.x * n, -a.y * n, -a.z * n, a.w * n};
}
// Quaternion::Normalize, :457-465, with Norm (:454-456) and math::sqrt (L/util/math.inl:28-30): float(sqrt(double(sum)))
MMDX_ROOT_FN RootQuat root_q_normalize(const RootQuat a) {
    const float s = a.x * a.x + a.y * a.y + a.z * a.z + a.w * a.w;
    const float n = 1.0f / float(sqrt(double(s)));
    return {a.x * n, a.y * n, a.z * n, a.w * n};
}
// rotate(v, q.ToRotateMatrix()): L/util/math_impl.inl:1032-1038 over :540-563 (place_matrix_from_pose; q is not normalised)
MMDX_ROOT_FN RootVec root_rotate(const RootVec v, const RootQuat q) {
    const float pose[8] = {0.0f, 0.0f, 0.0f, 0.0f, q.x, q.y, q.z, q.w};
    float m[16];
    place_matrix_from_pose(pose, m);
    return {v.x * m[0] + v.y * m[4] + v.z * m[8], v.x * m[1] + v.y * m[5] + v.z * m[9], v.x * m[2] + v.y * m[6] + v.z * m[10]};
}

// One leg from (t0, q0) to (t1, q1): qi = q0.Inverse(); dq = qi * q1; D = rotate(t1 - t0, M(qi))
MMDX_ROOT_FN RootDelta root_turn_leg(const RootVec t0, const RootQuat q0, const RootVec t1, const RootQuat q1) {
    const RootQuat qi = root_q_inverse(q0);
    return {root_rotate(root_sub(t1, t0), qi), root_q_mul(qi, q1)};
}
// A side from (T, Q) at its four instants (near / far are not looked at without a fold).  Folded: the leg t0 -> near, then the leg
// far -> t1 carried into the first one's frame: D = d1 + rotate(d2, M(dq1)), dq = dq1 * dq2.
MMDX_ROOT_FN RootDelta root_turn_side(const RootVec *t, const RootQuat *q, uint32_t folded) {
    if (!folded) return root_turn_leg(t[kRootT0], q[kRootT0], t[kRootT1], q[kRootT1]);
    const RootDelta one = root_turn_leg(t[kRootT0], q[kRootT0], t[kRootNear], q[kRootNear]);
    const RootDelta two = root_turn_leg(t[kRootFar], q[kRootFar], t[kRootT1], q[kRootT1]);
    return {root_add(one.d, root_rotate(two.d, one.q)), root_q_mul(one.q, two.q)};
}

// `side` is blend_side(w); `pose` is blend_pose (motion_blend.hpp) over two pairs: the lerp per channel and NLerp's middle branch
// with its normalisation.  An end-point row is that side's pair unchanged.
template <class Pose>
MMDX_ROOT_FN RootDelta root_turn_blend(const RootDelta a, const RootDelta b, uint32_t side, float w, Pose pose) {
    if (side == kRootSideA) return a;
    if (side == kRootSideB) return b;
    return pose(a, b, w);
}

// pose = one placement {p, (untouched), h}: p.c = p.c + rotate(D, M(h)).c with the heading BEFORE the step, then h = h * dq and,
// with `normalize`, its Normalize().  No short circuit for an identity dq.  pose[3] is neither read nor written.
MMDX_ROOT_FN void root_turn_accumulate(const RootDelta s, bool normalize, float *pose) {
    const RootQuat h = {pose[4], pose[5], pose[6], pose[7]};
    const RootVec r = root_rotate(s.d, h);
    pose[0] = pose[0] + r.x;
    pose[1] = pose[1] + r.y;
    pose[2] = pose[2] + r.z;
    RootQuat n = root_q_mul(h, s.q);
    if (normalize) n = root_q_normalize(n);
    pose[4] = n.x; pose[5] = n.y; pose[6] = n.z; pose[7] = n.w;
}

}  // namespace mmdx

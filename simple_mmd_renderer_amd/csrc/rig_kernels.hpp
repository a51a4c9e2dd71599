// rig_kernels.hpp -- launchers of rig_kernels.hip.
#pragma once

#include <hip/hip_runtime.h>

#include "anim_math.hpp"
#include "instance_list.hpp"
#include "rig.hpp"
#include "row_blend_kernels.hpp"

namespace mmdx {
int env_int(const char *name, int dflt);   // api.cpp

hipError_t launch_bone_track_eval(const BoneTrackParams &p, hipStream_t stream);
hipError_t launch_skeleton_fk(const SkeletonParams &p, hipStream_t stream);
// bone tracks -> palette in one launch (parallel-FK skeletons): poses of an instance live in LDS (nb * 32 bytes <= kMotionFkMaxLds)
constexpr size_t kMotionFkMaxLds = 64 * 1024;
hipError_t launch_motion_fk(const BoneTrackParams &t, const SkeletonParams &p, hipStream_t stream);
// the same two for a motion set (rig.hpp MotionSetHost): p / t hold the set's concatenated tables, clips[ni] the clip of every
// instance (device memory); ids >= n_clips play nothing (rest pose)
hipError_t launch_bone_track_eval_set(const BoneTrackParams &p, const uint32_t *clips, uint32_t n_clips, hipStream_t stream);
hipError_t launch_motion_fk_set(const BoneTrackParams &t, const SkeletonParams &p, const uint32_t *clips, uint32_t n_clips,
                                hipStream_t stream);
struct BlendOperands;
// the cross-fade between two clips of a set (motion_blend.hpp): the same two with the five per-instance operand arrays of
// mmdx_motion_blend_args in device memory; time clock only
hipError_t launch_bone_track_blend_set(const BoneTrackParams &p, const BlendOperands &o, hipStream_t stream);
hipError_t launch_motion_fk_blend_set(const BoneTrackParams &t, const SkeletonParams &p, const BlendOperands &o, hipStream_t stream);
// `shape` (solve_shape.hpp; may be nullptr) receives what the call launched, and only when every launch succeeded
struct SolveShape;
hipError_t launch_skeleton_ordered(const SerialParams &p, const uint8_t *round_coop /* host, [n_rounds] or nullptr */, hipStream_t stream,
                                   SolveShape *shape);
hipError_t launch_bone_morph(const BoneMorphParams &p, hipStream_t stream);
hipError_t launch_physics_override(const PhysicsParams &p, hipStream_t stream);
// mmdx_skeleton_solve_select: the select forms of the one-step solve's kernels.  Their parameter blocks are the plain ones with
// ni = the list's CAPACITY (state and bone-morph cells are per list position); the list travels as a kernel argument of its own.
// (InstanceList: instance_list.hpp)
hipError_t launch_skeleton_fk_select(const SkeletonParams &p, const InstanceList &list, hipStream_t stream);
hipError_t launch_bone_morph_select(const BoneMorphParams &p, const InstanceList &list, hipStream_t stream);
hipError_t launch_skeleton_ordered_select(const SerialParams &p, const uint8_t *round_coop, const InstanceList &list, hipStream_t stream,
                                          SolveShape *shape);
// mmdx_motion_set_blend_bones_time_select / mmdx_skeleton_solve_motion_set_blend_time_select: the select forms of the two blend
// kernels.  p.ni / t.ni = the list's capacity; operand rows, pose rows and palette rows are addressed by id (list.n_rows of them).
hipError_t launch_bone_track_blend_set_select(const BoneTrackParams &p, const BlendOperands &o, const InstanceList &list, hipStream_t stream);
hipError_t launch_motion_fk_blend_set_select(const BoneTrackParams &t, const SkeletonParams &p, const BlendOperands &o,
                                             const InstanceList &list, hipStream_t stream);
// mmdx_animator_root_motion.  It lives here, not in anim_kernels.hip, next to the other kernels that call eval_bone_pose.
// p: the concatenated bone tables of a set with k.n_clips clips (clock and output fields unused); the seven arrays are the
// animator's, [ni] each, only read; placements [ni][8], of which [0..2] are updated.  dt / dt_dev as launch_animator_advance.
struct RootMotionParams {
    const uint32_t *clips_a, *clips_b;
    const double *times_a, *times_b;
    const float *weights, *speed, *fade_rate;
    uint32_t ni;
    AnimClips k;
    uint32_t root_bone, axes;                   // root_bone < p.nb; MMDX_ROOT_X | _Y | _Z
    float *placements;
};
hipError_t launch_animator_root_motion(const BoneTrackParams &p, const RootMotionParams &r, double dt, const double *dt_dev,
                                       hipStream_t stream);
// mmdx_animator_root_motion_turn: the same operands; placements[i][0..2] and [4..7] are updated.  normalize: MMDX_ROOT_NORMALIZE.
hipError_t launch_animator_root_turn(const BoneTrackParams &p, const RootMotionParams &r, bool normalize, double dt, const double *dt_dev,
                                     hipStream_t stream);
// mmdx_pose_add.  It lives here, not in row_blend_kernels.hip, because q_mul, q_inverse and q_slerp_from_identity are local to
// rig_kernels.hip.  Operands and conditions as launch_pose_blend (row_blend_kernels.hpp); refs is not read when n_refs == 0.
hipError_t launch_pose_add(const RowAddLaunch &p, const InstanceList *list, uint32_t cells, hipStream_t stream);

}  // namespace mmdx

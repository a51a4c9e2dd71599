// anim_kernels.hpp -- launchers of anim_kernels.hip (mmdx_animator_advance, mmdx_animator_request) and what anim_api.cpp shares
// with rig_api.cpp, the owner of the motion-set handle.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "anim_math.hpp"
#include "rig.hpp"

namespace mmdx {

constexpr uint32_t kAnimThreads = 256;          // one lane per instance

// the eleven state arrays, [ni] each, device memory
struct AnimArrays {
    uint32_t *clips_a, *clips_b;
    double *times_a, *times_b;
    float *weights, *speed, *fade_rate;
    uint32_t *req_clip;
    float *req_fade;
    double *req_time;
    uint32_t *loops;
    uint32_t ni;
};

// dt_dev != nullptr: the step is read from device memory when the kernel runs, `dt` is ignored
hipError_t launch_animator_advance(const AnimArrays &a, const AnimClips &k, double dt, const double *dt_dev, hipStream_t stream);

// n requests, device memory: ids[n], clips[n], fades[n] or nullptr (0), times[n] or nullptr (0); an id >= ni is skipped
struct AnimRequests {
    const uint32_t *ids, *clips;
    const float *fades;
    const double *times;
    uint32_t n;
};
hipError_t launch_animator_request(const AnimArrays &a, const AnimRequests &r, hipStream_t stream);

// anim_api.cpp: the largest key frame of every clip of a set, over the sides the set has (Motion::GetLength of those tracks)
std::vector<uint32_t> motion_set_last_frames(const MotionSetHost &h);
// rig_api.cpp: that table of a set handle, computed at mmdx_motion_set_create
const std::vector<uint32_t> &motion_set_clip_frames(const mmdx_motion_set_s *set);

}  // namespace mmdx

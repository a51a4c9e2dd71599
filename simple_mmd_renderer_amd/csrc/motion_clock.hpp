// motion_clock.hpp -- the instant a VMD track is sampled at, for the track-evaluation kernels (bone tracks in rig_kernels.hip,
// morph tracks in kernels.hip).  The kernels are templated on the clock; the key search, the curve lookup and the blends are
// shared.  Both translation units are built with -ffp-contract=off and without fast-math, so `time * 30.0` stays a separate
// rounding and the double division below is correctly rounded.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace mmdx {

// Motion::GetBonePose / GetMorphPose(name, size_t frame), L/motion/motion_impl.inl:255-319, :382-424 (MotionPlayer::SeekFrame):
// a whole frame number; an exact key hit returns the key unchanged; bary = float(frame-lf) / float(rf-lf) in f32.
struct FrameClock {
    uint32_t frame;
    __device__ __forceinline__ bool at_or_before_first(uint32_t kf) const { return kf >= frame; }
    __device__ __forceinline__ bool at_or_after_last(uint32_t kf) const { return kf <= frame; }
    __device__ __forceinline__ uint32_t search() const { return frame; }
    __device__ __forceinline__ bool exact(uint32_t lf) const { return lf == frame; }
    __device__ __forceinline__ float bary(uint32_t lf, uint32_t rf) const { return float(frame - lf) / float(rf - lf); }
};

// GetBonePose / GetMorphPose(name, double time), :321-380, :426-465 (MotionPlayer::SeekTime, poser_impl.inl:548-555): seconds.
// dframe = time * 30.0 in double; the clamps compare the key frames as doubles (NaN, undefined in the reference, takes the
// first key); the bracket is upper_bound(size_t(dframe)) -- in range, the clamps have left dframe inside [first, last);
// bary = float((dframe - lf) / (rf - lf)) in double, rounded once; no exact-hit shortcut (dframe == lf interpolates at 0).
struct TimeClock {
    double dframe;
    __device__ __forceinline__ bool at_or_before_first(uint32_t kf) const { return !(double(kf) < dframe); }
    __device__ __forceinline__ bool at_or_after_last(uint32_t kf) const { return double(kf) <= dframe; }
    __device__ __forceinline__ uint32_t search() const { return uint32_t(dframe); }
    __device__ __forceinline__ bool exact(uint32_t) const { return false; }
    __device__ __forceinline__ float bary(uint32_t lf, uint32_t rf) const {
        return float((dframe - double(lf)) / double(rf - lf));
    }
};

// the clock of instance i: frames[i] (FrameClock) or times[i] seconds (TimeClock)
template <class Clock>
__device__ __forceinline__ Clock clock_of(const uint32_t *frames, const double *times, uint32_t i);
template <>
__device__ __forceinline__ FrameClock clock_of<FrameClock>(const uint32_t *frames, const double *, uint32_t i) {
    return {frames[i]};
}
template <>
__device__ __forceinline__ TimeClock clock_of<TimeClock>(const uint32_t *, const double *times, uint32_t i) {
    return {times[i] * 30.0};
}

// the instantiation of a clock-templated kernel that a call launches: seconds when it carries times, else frames
#define MMDX_BY_CLOCK(kernel, times) ((times) ? kernel<TimeClock> : kernel<FrameClock>)

}  // namespace mmdx

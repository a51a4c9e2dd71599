// anim_kernels.hip -- mmdx_animator_advance and mmdx_animator_request on gfx950 (include/mmdx.h states the arithmetic;
// anim_math.hpp holds it, shared with the CPU driver of the tests; this file is built with -ffp-contract=off like the rest).
//
// one lane per instance     the state is eleven arrays [ni]: a wave loads and stores 256 or 512 contiguous bytes of each, 56 bytes per
//                           instance in all.  A lane touches no row but its own, so the arrays are updated in place.  The eight
//                           arrays a step can change are stored back whether it changed them or not: no branch decides a store
//                           (speed, req_fade and req_time are only read).
// the clip table            [n_clips] x 24 bytes, read through the lane's clip ids (a gather, but a crowd plays a handful of clips: the
//                           table stays in the scalar / vector caches).
// dt                        a kernel argument, or -- dt_dev != nullptr -- one double in device memory that every lane reads when the
//                           kernel runs (wave-uniform address: a scalar load).  A NaN step returns before any store.
#include <hip/hip_runtime.h>

#include "anim_kernels.hpp"

namespace mmdx {

namespace {

__global__ __launch_bounds__(kAnimThreads) void animator_advance_kernel(AnimArrays a, AnimClips k, double dt, const double *dt_dev) {
    if (dt_dev) dt = *dt_dev;
    if (dt != dt) return;
    const uint32_t i = blockIdx.x * kAnimThreads + threadIdx.x;
    if (i >= a.ni) return;
    AnimLane s;
    s.clip_a = a.clips_a[i];    s.clip_b = a.clips_b[i];
    s.time_a = a.times_a[i];    s.time_b = a.times_b[i];
    s.weight = a.weights[i];    s.speed = a.speed[i];      s.fade_rate = a.fade_rate[i];
    s.req_clip = a.req_clip[i]; s.req_fade = a.req_fade[i]; s.req_time = a.req_time[i];
    s.loops = a.loops[i];
    anim_advance(k, s, dt);
    a.clips_a[i] = s.clip_a;    a.clips_b[i] = s.clip_b;
    a.times_a[i] = s.time_a;    a.times_b[i] = s.time_b;
    a.weights[i] = s.weight;    a.fade_rate[i] = s.fade_rate;
    a.req_clip[i] = s.req_clip;
    a.loops[i] = s.loops;
}

// request j -> row ids[j] of the three request arrays; the ids of one call are distinct, so no two lanes write one row
__global__ __launch_bounds__(kAnimThreads) void animator_request_kernel(AnimArrays a, AnimRequests r) {
    const uint32_t j = blockIdx.x * kAnimThreads + threadIdx.x;
    if (j >= r.n) return;
    const uint32_t i = r.ids[j];
    if (i >= a.ni) return;
    a.req_clip[i] = r.clips[j];
    a.req_fade[i] = r.fades ? r.fades[j] : 0.0f;
    a.req_time[i] = r.times ? r.times[j] : 0.0;
}

}  // namespace

hipError_t launch_animator_advance(const AnimArrays &a, const AnimClips &k, double dt, const double *dt_dev, hipStream_t stream) {
    if (!a.ni) return hipSuccess;
    const dim3 grid((a.ni + kAnimThreads - 1) / kAnimThreads), block(kAnimThreads);
    hipLaunchKernelGGL(animator_advance_kernel, grid, block, 0, stream, a, k, dt, dt_dev);
    return hipGetLastError();
}

hipError_t launch_animator_request(const AnimArrays &a, const AnimRequests &r, hipStream_t stream) {
    if (!r.n) return hipSuccess;
    const dim3 grid((r.n + kAnimThreads - 1) / kAnimThreads), block(kAnimThreads);
    hipLaunchKernelGGL(animator_request_kernel, grid, block, 0, stream, a, r);
    return hipGetLastError();
}

}  // namespace mmdx

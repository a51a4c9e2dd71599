// events_kernels.hpp -- the launcher of events_kernels.hip (mmdx_animator_events) and what events_api.cpp takes from anim_api.cpp,
// the owner of the animator handle.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "../../include/mmdx.h"
#include "anim_kernels.hpp"
#include "events_math.hpp"
#include "graph_pin.hpp"

struct mmdx_animator_s;

namespace mmdx {

constexpr uint32_t kEventsChunk = 256;          // instances per chunk = lanes per workgroup, by default
constexpr uint32_t kEventsMaxChunk = 1024;

// MMDX_EVENTS_CHUNK as read for this call (0 = not set) -> the chunk: a multiple of 64 from 64 to 1 024, rounded down and clamped
inline uint32_t events_chunk(int env) {
    if (env <= 0) return kEventsChunk;
    const uint32_t c = uint32_t(env) / 64u * 64u;
    return c < 64u ? 64u : (c > kEventsMaxChunk ? kEventsMaxChunk : c);
}

// one call: the seven state arrays it reads (device memory, [ni]), both tables, and where the results go
struct EventsLaunch {
    const uint32_t *clips_a, *clips_b;
    const double *times_a, *times_b;
    const float *weights, *speed, *fade_rate;
    uint32_t ni;
    AnimClips clips;
    EventTable markers;
    bool dominant;                              // MMDX_EVENTS_DOMINANT_SIDE
    uint32_t *out_fired;                        // [ni]
    uint32_t n_lists, list_stride;              // n_lists == 0: one launch, nothing below is looked at
    uint32_t list_mask[kEventsMaxLists];        // entries >= n_lists: 0 (no instance is in such a list)
    const uint32_t *levels;                     // [ni] or nullptr
    uint32_t *out_ids, *out_counts;
    uint32_t *chunk_counts;                     // [ceil(ni / chunk)][kEventsMaxLists], the set's scratch
};
// dt_dev != nullptr: the step is read from device memory when the kernels run, `dt` is ignored
hipError_t launch_animator_events(const EventsLaunch &e, uint32_t chunk, double dt, const double *dt_dev, hipStream_t stream);

// anim_api.cpp, for events_api.cpp: what an event set copies of an animator at creation (no device) ...
struct AnimatorHostTable {
    uint32_t ni, n_clips;
    const mmdx_animator_clip *clips;            // [n_clips] as resolved: what mmdx_animator_get_info reports; the animator's own
};
AnimatorHostTable animator_host_table(const mmdx_animator_s *a);
// ... and, for a call, its state on `device` (allocated there by the first call that needs it), its table and its pin
mmdx_status animator_on_device(mmdx_animator_s *a, int device, AnimArrays *arrays, AnimClips *table, GraphPin **pin);

}  // namespace mmdx

// events_math.hpp -- the arithmetic of mmdx_animator_events (include/mmdx.h states it), once: the gfx950 kernels
// (events_kernels.hip) and a CPU driver (tests/events_math_driver.cpp) compile these same lines, and tests/animator_events_ref.py
// restates them in numpy.  Comparisons of doubles only; the clocks are called, not restated: the instants of a side are root_times
// (root_math.hpp) over anim_wrap (anim_math.hpp).  Both builds pass -ffp-contract=off like the rest.
#pragma once

#include <cstdint>

#include "anim_math.hpp"
#include "root_math.hpp"

#if defined(__HIPCC__)
#define MMDX_EVENTS_FN __host__ __device__ __forceinline__
#else
#define MMDX_EVENTS_FN inline
#endif

namespace mmdx {

// the values of MMDX_CULLED and MMDX_EVENTS_MAX_LISTS of include/mmdx.h (events_api.cpp asserts they agree)
constexpr uint32_t kEventsCulled = 0xFFFFFFFFu, kEventsMaxLists = 4;

// mmdx_event_marker's layout (events_api.cpp asserts it)
struct EventMarker {
    double time;
    uint32_t clip, channel;
};

// the marker table: markers sorted by (clip, time), those of clip c at [first[c], first[c + 1])
struct EventTable {
    const EventMarker *markers;
    const uint32_t *first;                      // [n_clips + 1]
    uint32_t n_clips;
};

// Step 3: does the leg u -> v pass m?  The direction is the leg's own; `closed` says whether u itself counts (v always does).
MMDX_EVENTS_FN bool events_leg(double u, double v, bool closed, double m) {
    if (u <= v) return (closed ? u <= m : u < m) && m <= v;
    return v <= m && (closed ? m <= u : m < u);
}

// Step 4: does the side whose instants are r pass m?
MMDX_EVENTS_FN bool events_passes(const RootTimes &r, double m) {
    if (!r.folded) return events_leg(r.t0, r.t1, false, m);
    return events_leg(r.t0, r.near, false, m) || events_leg(r.far, r.t1, true, m);
}

// Steps 2, 4 and 5: what the side (c, t0) fires during a step of s seconds.  A scan of the clip's markers, not a search: a clip has
// a handful, a folded side would need four bounds instead of one pass, and neighbouring lanes on one clip read the same entries.
// (Measured: the scan is what the call costs beyond a launch, 0.3 us per marker of the clip, and it is the comparisons a lone wave
// issues, not the loads: four markers loaded per pass ahead of their comparisons changed nothing and was not kept.)
MMDX_EVENTS_FN uint32_t events_side(const AnimClips &k, const EventTable &e, uint32_t c, double t0, double s) {
    if (c >= e.n_clips || c >= k.n_clips) return 0u;
    if (s != s) return 0u;                      // a NaN step: wrap would clamp the NaN clock of a HOLD clip to 0
    const RootTimes r = root_times(k, c, t0, s);
    uint32_t fired = 0u;
    for (uint32_t j = e.first[c]; j < e.first[c + 1]; ++j)
        if (events_passes(r, e.markers[j].time)) fired |= 1u << (e.markers[j].channel & 31u);
    return fired;
}

// Step 6: one instance's mask from its row of the seven arrays the call reads
MMDX_EVENTS_FN uint32_t events_fired(const AnimClips &k, const EventTable &e, uint32_t clip_a, uint32_t clip_b, double time_a, double time_b,
                                     float weight, float speed, float fade_rate, double dt, bool dominant) {
    const double s = double(speed) * dt;
    const bool fading = fade_rate > 0.0f;
    if (dominant) {
        if (fading && weight > 0.5f) return events_side(k, e, clip_b, time_b, s);
        return events_side(k, e, clip_a, time_a, s);
    }
    uint32_t fired = events_side(k, e, clip_a, time_a, s);
    if (fading) fired |= events_side(k, e, clip_b, time_b, s);
    return fired;
}

// Step 7: is an instance with this mask (and this level, when levels are given) in the list of `list_mask`?
MMDX_EVENTS_FN bool events_in_list(uint32_t fired, uint32_t list_mask, bool has_levels, uint32_t level) {
    return (fired & list_mask) != 0u && !(has_levels && level == kEventsCulled);
}

}  // namespace mmdx

// events_table.hpp -- the marker table of an event set as mmdx_event_set_create stores it: host code, compiled by events_api.cpp
// and by the CPU driver of the tests (tests/events_math_driver.cpp), which prints what it made.
#pragma once

#include <algorithm>
#include <cstdint>
#include <vector>

#include "events_math.hpp"

namespace mmdx {

// markers (every clip < n_clips, checked by the caller) -> sorted by (clip, time), markers of equal clip and time in the order
// given; first[c] .. first[c + 1] are those of clip c.
inline void events_table_build(const EventMarker *markers, uint32_t n, uint32_t n_clips, std::vector<EventMarker> *sorted,
                               std::vector<uint32_t> *first) {
    sorted->assign(markers, markers + n);
    std::stable_sort(sorted->begin(), sorted->end(), [](const EventMarker &a, const EventMarker &b) {
        return a.clip != b.clip ? a.clip < b.clip : a.time < b.time;
    });
    first->assign(size_t(n_clips) + 1, 0);
    for (const EventMarker &m : *sorted) ++(*first)[size_t(m.clip) + 1];
    for (uint32_t c = 0; c < n_clips; ++c) (*first)[c + 1] += (*first)[c];
}

}  // namespace mmdx

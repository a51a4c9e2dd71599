// events_api.cpp -- the event set handle (a marker table) and mmdx_animator_events (include/mmdx.h): validation on the host before
// the first HIP call, the table's device copy on the first call that needs it, and the launches (events_kernels.hip) on the model's
// stream.  The animator is reached through animator_host_table / animator_on_device (anim_api.cpp) only.
#include <cstddef>
#include <cstring>
#include <memory>
#include <new>
#include <string>
#include <vector>

#include "api_internal.hpp"
#include "events_kernels.hpp"
#include "events_table.hpp"

using namespace mmdx;

static_assert(sizeof(mmdx_event_marker) == 16 && sizeof(EventMarker) == 16 && offsetof(mmdx_event_marker, clip) == offsetof(EventMarker, clip) &&
                  offsetof(mmdx_event_marker, channel) == offsetof(EventMarker, channel),
              "events_math.hpp restates mmdx_event_marker");
static_assert(kEventsCulled == MMDX_CULLED && kEventsMaxLists == MMDX_EVENTS_MAX_LISTS, "events_math.hpp restates mmdx.h");
static_assert((MMDX_EVENTS_DOMINANT_SIDE & (MMDX_ANIM_DT_ON_DEVICE | MMDX_ROOT_NORMALIZE | MMDX_BLEND_PARAMS_ON_DEVICE)) == 0,
              "MMDX_EVENTS_DOMINANT_SIDE shares a bit");

struct mmdx_event_set_s {
    uint32_t n_markers = 0, n_clips = 0;
    std::vector<EventMarker> sorted;              // by (clip, time)
    std::vector<uint32_t> first;                  // [n_clips + 1]
    int device = -1;                              // where the copy lives, -1 = not made yet
    DevBuf table;                                 // static: sorted[n_markers], then first[n_clips + 1]
    DevBuf counts;                                // per-chunk, per-list counts of a call with lists
    GraphPin pin;                                 // recorded graphs that hold these addresses
    mmdx_event_set_s() { table.pin = counts.pin = &pin; }
};

namespace {

// The table goes to the device of the first call that needs it and stays there.
mmdx_status table_to_device(mmdx_event_set_t s, int device) {
    if (s->device == device) return MMDX_OK;
    if (s->device >= 0)
        return fail(MMDX_ERR_INVALID_ARGUMENT, "this event set's table lives on device " + std::to_string(s->device) + ", the call runs on device " +
                                               std::to_string(device));
    if (graph_recording())
        return fail(MMDX_ERR_INVALID_ARGUMENT, "while a graph is being recorded the event set must have run on this device before");
    const size_t marker_bytes = s->sorted.size() * sizeof(EventMarker);
    std::vector<char> image(marker_bytes + s->first.size() * 4);
    if (marker_bytes) std::memcpy(image.data(), s->sorted.data(), marker_bytes);
    std::memcpy(image.data() + marker_bytes, s->first.data(), s->first.size() * 4);
    if (hipError_t e = s->table.upload(image)) {
        s->table.release();
        return hip_fail(e, "event table upload");
    }
    s->device = device;
    return MMDX_OK;
}

}  // namespace

extern "C" {

mmdx_status mmdx_event_set_create(mmdx_animator_t animator, const mmdx_event_set_desc *desc, mmdx_event_set_t *out_set) {
    if (!out_set) return fail(MMDX_ERR_INVALID_ARGUMENT, "out_set is NULL");
    *out_set = nullptr;
    if (!animator || !desc) return fail(MMDX_ERR_INVALID_ARGUMENT, "animator / desc is NULL");
    if (desc->struct_size != sizeof(mmdx_event_set_desc)) return fail(MMDX_ERR_INVALID_ARGUMENT, "mmdx_event_set_desc.struct_size mismatch");
    if (desc->n_markers && !desc->markers) return fail(MMDX_ERR_INVALID_ARGUMENT, "mmdx_event_set_desc.markers is NULL");
    try {
        const AnimatorHostTable t = animator_host_table(animator);
        for (uint32_t j = 0; j < desc->n_markers; ++j) {
            const mmdx_event_marker &m = desc->markers[j];
            const std::string at = "mmdx_event_set_desc.markers[" + std::to_string(j) + "]";
            if (m.clip >= t.n_clips)
                return fail(MMDX_ERR_BAD_INDEX, at + ".clip = " + std::to_string(m.clip) + ": the animator has " + std::to_string(t.n_clips) + " clips");
            if (m.channel >= 32) return fail(MMDX_ERR_INVALID_ARGUMENT, at + ".channel = " + std::to_string(m.channel) + " is not below 32");
            if (!(m.time >= 0.0 && m.time <= t.clips[m.clip].length))
                return fail(MMDX_ERR_INVALID_ARGUMENT, at + ".time = " + std::to_string(m.time) + " is NaN or outside [0, " +
                                                       std::to_string(t.clips[m.clip].length) + "], the length of clip " + std::to_string(m.clip));
        }
        std::unique_ptr<mmdx_event_set_s> s(new mmdx_event_set_s);
        s->n_markers = desc->n_markers;
        s->n_clips = t.n_clips;
        events_table_build(reinterpret_cast<const EventMarker *>(desc->markers), desc->n_markers, t.n_clips, &s->sorted, &s->first);
        *out_set = s.release();
    } catch (const std::bad_alloc &) {
        return fail(MMDX_ERR_OUT_OF_MEMORY, "host allocation failed");
    }
    return MMDX_OK;
}

void mmdx_event_set_destroy(mmdx_event_set_t set) {
    if (!set) return;
    graph_drop_handle(&set->pin);
    if (set->device >= 0) (void)hipSetDevice(set->device);
    set->table.release();
    set->counts.release();
    delete set;
}

mmdx_status mmdx_event_set_get_info(mmdx_event_set_t set, mmdx_event_set_info *info) {
    if (!set || !info || info->struct_size != sizeof(mmdx_event_set_info))
        return fail(MMDX_ERR_INVALID_ARGUMENT, "NULL argument or mmdx_event_set_info.struct_size mismatch");
    info->n_markers = set->n_markers;
    info->n_clips = set->n_clips;
    info->device_ordinal = set->device;
    return MMDX_OK;
}

mmdx_status mmdx_animator_events(mmdx_animator_t a, mmdx_event_set_t set, mmdx_model_t model, const mmdx_events_args *args) {
    if (!a || !set || !args) return fail(MMDX_ERR_INVALID_ARGUMENT, "animator / set / args is NULL");
    if (args->struct_size != sizeof(mmdx_events_args)) return fail(MMDX_ERR_INVALID_ARGUMENT, "mmdx_events_args.struct_size mismatch");
    if (!args->dt || !args->out_fired) return fail(MMDX_ERR_INVALID_ARGUMENT, "dt / out_fired is NULL");
    if (args->flags & ~uint32_t(MMDX_ANIM_DT_ON_DEVICE | MMDX_EVENTS_DOMINANT_SIDE)) return fail(MMDX_ERR_INVALID_ARGUMENT, "unknown flag bits");
    const AnimatorHostTable t = animator_host_table(a);
    if (args->n_lists > MMDX_EVENTS_MAX_LISTS)
        return fail(MMDX_ERR_INVALID_ARGUMENT, "n_lists = " + std::to_string(args->n_lists) + ": at most MMDX_EVENTS_MAX_LISTS (4)");
    if (args->n_lists) {
        if (!args->out_ids || !args->out_counts) return fail(MMDX_ERR_INVALID_ARGUMENT, "out_ids / out_counts is NULL with n_lists > 0");
        if (args->list_stride < t.ni)
            return fail(MMDX_ERR_INVALID_ARGUMENT, "list_stride = " + std::to_string(args->list_stride) + " is below the animator's " +
                                                   std::to_string(t.ni) + " instances");
    }
    uintptr_t four = reinterpret_cast<uintptr_t>(args->out_fired) | reinterpret_cast<uintptr_t>(args->levels);
    if (args->n_lists) four |= reinterpret_cast<uintptr_t>(args->out_ids) | reinterpret_cast<uintptr_t>(args->out_counts);
    if (four & 3) return fail(MMDX_ERR_INVALID_ARGUMENT, "out_fired / levels / out_ids / out_counts must be 4-byte aligned");
    if (set->n_clips != t.n_clips)
        return fail(MMDX_ERR_INVALID_ARGUMENT, "the event set has " + std::to_string(set->n_clips) + " clips, the animator's table " +
                                               std::to_string(t.n_clips));
    const bool on_device = (args->flags & MMDX_ANIM_DT_ON_DEVICE) != 0;
    if (on_device) {
        if (reinterpret_cast<uintptr_t>(args->dt) & 7) return fail(MMDX_ERR_INVALID_ARGUMENT, "a device dt must be 8-byte aligned");
    } else if (*args->dt != *args->dt) {
        return fail(MMDX_ERR_INVALID_ARGUMENT, "dt is NaN");
    }
    int device;
    hipStream_t st;
    if (mmdx_status r = resolve_stream(model, &device, &st)) return r;
    AnimArrays s;
    AnimClips table;
    GraphPin *animator_pin;
    if (mmdx_status r = animator_on_device(a, device, &s, &table, &animator_pin)) return r;
    if (mmdx_status r = table_to_device(set, device)) return r;
    const uint32_t chunk = events_chunk(env_int("MMDX_EVENTS_CHUNK", 0));
    if (args->n_lists) {
        const size_t nchunks = (size_t(t.ni) + chunk - 1) / chunk;
        if (hipError_t e = set->counts.ensure(nchunks * kEventsMaxLists * sizeof(uint32_t))) return hip_fail(e, "the event set's count scratch");
    }
    graph_note_handle(model, animator_pin);
    graph_note_handle(model, &set->pin);
    EventsLaunch e{};
    e.clips_a = s.clips_a; e.clips_b = s.clips_b;
    e.times_a = s.times_a; e.times_b = s.times_b;
    e.weights = s.weights; e.speed = s.speed; e.fade_rate = s.fade_rate;
    e.ni = s.ni;
    e.clips = table;
    const char *tb = static_cast<const char *>(set->table.ptr);
    e.markers = EventTable{reinterpret_cast<const EventMarker *>(tb),
                           reinterpret_cast<const uint32_t *>(tb + size_t(set->n_markers) * sizeof(EventMarker)), set->n_clips};
    e.dominant = (args->flags & MMDX_EVENTS_DOMINANT_SIDE) != 0;
    e.out_fired = args->out_fired;
    e.n_lists = args->n_lists;
    e.list_stride = args->list_stride;
    for (uint32_t l = 0; l < args->n_lists; ++l) e.list_mask[l] = args->list_mask[l];
    e.levels = args->n_lists ? args->levels : nullptr;
    e.out_ids = args->out_ids;
    e.out_counts = args->out_counts;
    e.chunk_counts = static_cast<uint32_t *>(set->counts.ptr);
    HIP_TRY(launch_animator_events(e, chunk, on_device ? 0.0 : *args->dt, on_device ? args->dt : nullptr, st));
    return MMDX_OK;
}

}  // extern "C"

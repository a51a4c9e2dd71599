// anim_api.cpp -- the crowd animator (include/mmdx.h, mmdx_animator_*): the per-instance playback state in device memory, argument
// validation on the host before the first HIP call, and the launches (anim_kernels.hip) on the model's stream.  Also the clip
// lengths of a motion set (mmdx_motion_set_clip_frames reads what motion_set_last_frames computed at mmdx_motion_set_create).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <memory>
#include <new>
#include <string>
#include <vector>

#include "../../include/mmdx.h"
#include "anim_kernels.hpp"
#include "api_internal.hpp"
#include "error.hpp"
#include "events_kernels.hpp"
#include "graph_pin.hpp"
#include "host_runtime.hpp"
#include "rig_kernels.hpp"
#include "root_math.hpp"

using namespace mmdx;

static_assert(kRootX == MMDX_ROOT_X && kRootY == MMDX_ROOT_Y && kRootZ == MMDX_ROOT_Z, "root_math.hpp restates mmdx.h");
static_assert(kAnimClipNone == MMDX_CLIP_NONE && kAnimNoRequest == MMDX_ANIM_NO_REQUEST, "anim_math.hpp restates mmdx.h");
static_assert(kAnimLoop == MMDX_ANIM_LOOP && kAnimHold == MMDX_ANIM_HOLD && kAnimThen == MMDX_ANIM_THEN, "anim_math.hpp restates mmdx.h");

namespace {

constexpr size_t kStateBytes = 3 * 8 + 8 * 4;     // per instance: three f64 arrays, eight 4-byte arrays
constexpr size_t kTableBytes = 8 + 3 * 4;         // per clip: length, mode, next, fade
constexpr size_t kRequestBytes = 8 + 3 * 4;       // per request of a host list: start time, id, clip, fade

bool is_nan(double x) { return x != x; }

}  // namespace

struct mmdx_animator_s {
    uint32_t ni = 0, n_clips = 0;
    std::vector<mmdx_animator_clip> clips;        // the table as resolved (lengths in seconds)
    int device = -1;                              // where the state lives, -1 = not allocated yet
    void *block = nullptr;                        // the eleven arrays, the table and the request staging, one allocation
    AnimArrays arrays{};
    AnimClips table{};
    void *req = nullptr;                          // mmdx_animator_request with host lists: times[n], ids[n], clips[n], fades[n]; room
                                                  // for n = ni (the ids of a call are distinct), so it never has to grow
    std::vector<char> req_host;                   // ... its source, alive until the copy has left it
    GraphPin pin;                                 // recorded graphs that hold these addresses
};

namespace {

bool valid_clip(const mmdx_animator_s *a, uint32_t c) { return c < a->n_clips || c == MMDX_CLIP_NONE; }

// The state goes to the device of the first call that needs it, initialised, and stays there.
mmdx_status state_to_device(mmdx_animator_t a, int device) {
    if (a->device == device) return MMDX_OK;
    if (a->device >= 0)
        return fail(MMDX_ERR_INVALID_ARGUMENT, "this animator's state lives on device " + std::to_string(a->device) + ", the call runs on device " +
                                               std::to_string(device));
    if (graph_recording())
        return fail(MMDX_ERR_INVALID_ARGUMENT, "while a graph is being recorded the animator must have run on this device before");
    const size_t ni = a->ni, nc = a->n_clips, bytes = ni * kStateBytes + nc * kTableBytes;
    const size_t req_at = (bytes + 7) & ~size_t(7);
    std::vector<char> image(bytes, 0);
    char *h = image.data();
    // layout: times_a, times_b, req_time | clips_a, clips_b, weights, speed, fade_rate, req_clip, req_fade, loops | the table
    uint32_t *clips_a = reinterpret_cast<uint32_t *>(h + ni * 24), *clips_b = clips_a + ni;
    float *speed = reinterpret_cast<float *>(clips_a + ni * 3);
    uint32_t *req_clip = clips_a + ni * 5;
    for (size_t i = 0; i < ni; ++i) {
        clips_a[i] = clips_b[i] = MMDX_CLIP_NONE;
        speed[i] = 1.0f;
        req_clip[i] = MMDX_ANIM_NO_REQUEST;
    }
    char *t = h + ni * kStateBytes;
    double *length = reinterpret_cast<double *>(t);
    uint32_t *mode = reinterpret_cast<uint32_t *>(t + nc * 8), *next = mode + nc;
    float *fade = reinterpret_cast<float *>(next + nc);
    for (size_t c = 0; c < nc; ++c) {
        length[c] = a->clips[c].length;
        mode[c] = a->clips[c].mode;
        next[c] = a->clips[c].next;
        fade[c] = a->clips[c].fade;
    }
    void *d = nullptr;
    HIP_TRY(hipMalloc(&d, req_at + ni * kRequestBytes));
    if (hipError_t e = hipMemcpy(d, h, bytes, hipMemcpyHostToDevice)) {
        (void)hipFree(d);
        return hip_fail(e, "hipMemcpy of the animator's initial state");
    }
    char *b = static_cast<char *>(d);
    AnimArrays &s = a->arrays;
    s.times_a = reinterpret_cast<double *>(b);
    s.times_b = s.times_a + ni;
    s.req_time = s.times_b + ni;
    s.clips_a = reinterpret_cast<uint32_t *>(b + ni * 24);
    s.clips_b = s.clips_a + ni;
    s.weights = reinterpret_cast<float *>(s.clips_a + ni * 2);
    s.speed = s.weights + ni;
    s.fade_rate = s.weights + ni * 2;
    s.req_clip = s.clips_a + ni * 5;
    s.req_fade = s.weights + ni * 4;
    s.loops = s.clips_a + ni * 7;
    s.ni = a->ni;
    char *bt = b + ni * kStateBytes;
    a->table.length = reinterpret_cast<const double *>(bt);
    a->table.mode = reinterpret_cast<const uint32_t *>(bt + nc * 8);
    a->table.next = a->table.mode + nc;
    a->table.fade = reinterpret_cast<const float *>(a->table.next + nc);
    a->table.n_clips = a->n_clips;
    a->req = b + req_at;
    a->block = d;
    a->device = device;
    return MMDX_OK;
}

struct Member {
    void *host;
    void *dev;
    size_t elem;
};
// the members of a host mmdx_animator_arrays next to the device arrays they copy from / to
std::vector<Member> members(const mmdx_animator_arrays &h, const AnimArrays &d) {
    return {{h.clips_a, d.clips_a, 4},     {h.clips_b, d.clips_b, 4},   {h.times_a, d.times_a, 8},   {h.times_b, d.times_b, 8},
            {h.weights, d.weights, 4},     {h.speed, d.speed, 4},       {h.fade_rate, d.fade_rate, 4}, {h.req_clip, d.req_clip, 4},
            {h.req_fade, d.req_fade, 4},   {h.req_time, d.req_time, 8}, {h.loops, d.loops, 4}};
}

mmdx_status check_state_call(mmdx_animator_t a, const mmdx_animator_arrays *s) {
    if (!a || !s) return fail(MMDX_ERR_INVALID_ARGUMENT, "animator / state is NULL");
    if (s->struct_size != sizeof(mmdx_animator_arrays)) return fail(MMDX_ERR_INVALID_ARGUMENT, "mmdx_animator_arrays.struct_size mismatch");
    if (s->n_instances != a->ni)
        return fail(MMDX_ERR_INVALID_ARGUMENT, "mmdx_animator_arrays.n_instances is " + std::to_string(s->n_instances) + ", the animator has " +
                                               std::to_string(a->ni) + " instances");
    return MMDX_OK;
}

mmdx_status copy_state(mmdx_animator_t a, mmdx_model_t model, const mmdx_animator_arrays *s, bool to_device) {
    int device;
    hipStream_t st;
    if (mmdx_status r = resolve_stream(model, &device, &st)) return r;
    if (graph_recording())
        return fail(MMDX_ERR_INVALID_ARGUMENT, "mmdx_animator_set_state / _get_state copy host memory: not while a graph is being recorded");
    if (mmdx_status r = state_to_device(a, device)) return r;
    for (const Member &m : members(*s, a->arrays)) {
        if (!m.host) continue;
        const size_t bytes = size_t(a->ni) * m.elem;
        if (to_device) HIP_TRY(hipMemcpyAsync(m.dev, m.host, bytes, hipMemcpyHostToDevice, st));
        else HIP_TRY(hipMemcpyAsync(m.host, m.dev, bytes, hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(wait_stream(st));                     // the host arrays are borrowed for the call only
    return MMDX_OK;
}

}  // namespace

// events_api.cpp reaches an animator through these two and nothing else
AnimatorHostTable mmdx::animator_host_table(const mmdx_animator_s *a) {
    return AnimatorHostTable{a->ni, a->n_clips, a->clips.data()};
}

mmdx_status mmdx::animator_on_device(mmdx_animator_s *a, int device, AnimArrays *arrays, AnimClips *table, GraphPin **pin) {
    if (mmdx_status r = state_to_device(a, device)) return r;
    *arrays = a->arrays;
    *table = a->table;
    *pin = &a->pin;
    return MMDX_OK;
}

std::vector<uint32_t> mmdx::motion_set_last_frames(const MotionSetHost &h) {
    std::vector<uint32_t> last(h.n_clips, 0);
    for (uint32_t c = 0; c < h.n_clips; ++c) {
        if (h.has_bones) {
            const uint32_t *off = h.bones.key_off.data() + size_t(c) * (h.bones.nb + 1);
            for (uint32_t k = off[0]; k < off[h.bones.nb]; ++k) last[c] = std::max(last[c], h.bones.key_frame[k]);
        }
        if (h.has_morphs) {
            const uint32_t *off = h.morph_key_off.data() + size_t(c) * (h.nm + 1);
            for (uint32_t k = off[0]; k < off[h.nm]; ++k) last[c] = std::max(last[c], h.morph_frames[k]);
        }
    }
    return last;
}

extern "C" {

mmdx_status mmdx_motion_set_clip_frames(mmdx_motion_set_t set, uint32_t *last_frames) {
    if (!set || !last_frames) return fail(MMDX_ERR_INVALID_ARGUMENT, "set / last_frames is NULL");
    const std::vector<uint32_t> &f = motion_set_clip_frames(set);
    std::copy(f.begin(), f.end(), last_frames);
    return MMDX_OK;
}

mmdx_status mmdx_animator_create(mmdx_motion_set_t set, const mmdx_animator_desc *desc, mmdx_animator_t *out) {
    if (!out) return fail(MMDX_ERR_INVALID_ARGUMENT, "out_animator is NULL");
    *out = nullptr;
    if (!set || !desc) return fail(MMDX_ERR_INVALID_ARGUMENT, "set / desc is NULL");
    if (desc->struct_size != sizeof(mmdx_animator_desc)) return fail(MMDX_ERR_INVALID_ARGUMENT, "mmdx_animator_desc.struct_size mismatch");
    if (desc->reserved0 != 0) return fail(MMDX_ERR_INVALID_ARGUMENT, "mmdx_animator_desc.reserved0 must be 0");
    if (!desc->n_instances) return fail(MMDX_ERR_INVALID_ARGUMENT, "mmdx_animator_desc.n_instances == 0");
    const std::vector<uint32_t> &frames = motion_set_clip_frames(set);
    const uint32_t nc = uint32_t(frames.size());
    if (desc->clips && desc->n_clips != nc)
        return fail(MMDX_ERR_INVALID_ARGUMENT, "mmdx_animator_desc.n_clips is " + std::to_string(desc->n_clips) + ", the set has " +
                                               std::to_string(nc) + " clips");
    try {
        std::unique_ptr<mmdx_animator_s> a(new mmdx_animator_s);
        a->ni = desc->n_instances;
        a->n_clips = nc;
        a->clips.resize(nc);
        for (uint32_t c = 0; c < nc; ++c) {
            mmdx_animator_clip k{0.0, MMDX_ANIM_LOOP, MMDX_CLIP_NONE, 0.0f, 0};
            if (desc->clips) k = desc->clips[c];
            const std::string at = "mmdx_animator_desc.clips[" + std::to_string(c) + "]";
            if (k.mode > MMDX_ANIM_THEN) return fail(MMDX_ERR_INVALID_ARGUMENT, at + ".mode is not MMDX_ANIM_LOOP / _HOLD / _THEN");
            if (k.reserved0 != 0) return fail(MMDX_ERR_INVALID_ARGUMENT, at + ".reserved0 must be 0");
            if (k.mode == MMDX_ANIM_THEN) {
                if (!valid_clip(a.get(), k.next))
                    return fail(MMDX_ERR_BAD_INDEX, at + ".next = " + std::to_string(k.next) + ": the set has " + std::to_string(nc) + " clips");
                if (k.fade != k.fade) return fail(MMDX_ERR_INVALID_ARGUMENT, at + ".fade is NaN");
            } else {
                k.next = MMDX_CLIP_NONE;
                k.fade = 0.0f;
            }
            if (!(k.length > 0.0)) k.length = double(frames[c]) / 30.0;     // <= 0 or NaN: the clip's own length
            a->clips[c] = k;
        }
        *out = a.release();
    } catch (const std::bad_alloc &) {
        return fail(MMDX_ERR_OUT_OF_MEMORY, "host allocation failed");
    }
    return MMDX_OK;
}

void mmdx_animator_destroy(mmdx_animator_t a) {
    if (!a) return;
    graph_drop_handle(&a->pin);
    if (a->device >= 0) (void)hipSetDevice(a->device);
    device_free_or_defer(a->block);
    delete a;
}

mmdx_status mmdx_animator_get_info(mmdx_animator_t a, mmdx_animator_info *info, mmdx_animator_clip *clips) {
    if (!a || !info || info->struct_size != sizeof(mmdx_animator_info))
        return fail(MMDX_ERR_INVALID_ARGUMENT, "NULL argument or mmdx_animator_info.struct_size mismatch");
    info->n_instances = a->ni;
    info->n_clips = a->n_clips;
    info->device_ordinal = a->device;
    if (clips) std::copy(a->clips.begin(), a->clips.end(), clips);
    return MMDX_OK;
}

mmdx_status mmdx_animator_operands(mmdx_animator_t a, mmdx_motion_blend_args *out) {
    if (!a || !out) return fail(MMDX_ERR_INVALID_ARGUMENT, "animator / out is NULL");
    if (a->device < 0) {
        int device;
        hipStream_t st;
        if (mmdx_status r = resolve_stream(nullptr, &device, &st)) return r;
        if (mmdx_status r = state_to_device(a, device)) return r;
    }
    std::memset(out, 0, sizeof(*out));
    out->struct_size = sizeof(mmdx_motion_blend_args);
    out->n_instances = a->ni;
    out->clips_a = a->arrays.clips_a; out->clips_b = a->arrays.clips_b;
    out->times_a = a->arrays.times_a; out->times_b = a->arrays.times_b;
    out->weights = a->arrays.weights;
    out->flags = MMDX_TIMES_ON_DEVICE | MMDX_OUT_ON_DEVICE;
    return MMDX_OK;
}

mmdx_status mmdx_animator_device_arrays(mmdx_animator_t a, mmdx_animator_arrays *out) {
    if (!a || !out) return fail(MMDX_ERR_INVALID_ARGUMENT, "animator / out is NULL");
    if (out->struct_size != sizeof(mmdx_animator_arrays)) return fail(MMDX_ERR_INVALID_ARGUMENT, "mmdx_animator_arrays.struct_size mismatch");
    if (a->device < 0) {
        int device;
        hipStream_t st;
        if (mmdx_status r = resolve_stream(nullptr, &device, &st)) return r;
        if (mmdx_status r = state_to_device(a, device)) return r;
    }
    const AnimArrays &s = a->arrays;
    out->n_instances = a->ni;
    out->clips_a = s.clips_a; out->clips_b = s.clips_b;
    out->times_a = s.times_a; out->times_b = s.times_b;
    out->weights = s.weights; out->speed = s.speed; out->fade_rate = s.fade_rate;
    out->req_clip = s.req_clip; out->req_fade = s.req_fade; out->req_time = s.req_time;
    out->loops = s.loops;
    return MMDX_OK;
}

mmdx_status mmdx_animator_set_state(mmdx_animator_t a, mmdx_model_t model, const mmdx_animator_arrays *s) {
    if (mmdx_status r = check_state_call(a, s)) return r;
    const struct { const char *name; const uint32_t *ids; bool request; } id_arrays[3] = {
        {"clips_a", s->clips_a, false}, {"clips_b", s->clips_b, false}, {"req_clip", s->req_clip, true}};
    for (const auto &m : id_arrays)
        for (uint32_t i = 0; m.ids && i < a->ni; ++i)
            if (!valid_clip(a, m.ids[i]) && !(m.request && m.ids[i] == MMDX_ANIM_NO_REQUEST))
                return fail(MMDX_ERR_BAD_INDEX, std::string(m.name) + "[" + std::to_string(i) + "] = " + std::to_string(m.ids[i]) +
                                                ": the set has " + std::to_string(a->n_clips) + " clips");
    const struct { const char *name; const double *v; } f64_arrays[3] = {{"times_a", s->times_a}, {"times_b", s->times_b}, {"req_time", s->req_time}};
    for (const auto &m : f64_arrays)
        for (uint32_t i = 0; m.v && i < a->ni; ++i)
            if (is_nan(m.v[i])) return fail(MMDX_ERR_INVALID_ARGUMENT, std::string(m.name) + "[" + std::to_string(i) + "] is NaN");
    const struct { const char *name; const float *v; } f32_arrays[4] = {{"weights", s->weights}, {"speed", s->speed}, {"fade_rate", s->fade_rate},
                                                                        {"req_fade", s->req_fade}};
    for (const auto &m : f32_arrays)
        for (uint32_t i = 0; m.v && i < a->ni; ++i)
            if (is_nan(m.v[i])) return fail(MMDX_ERR_INVALID_ARGUMENT, std::string(m.name) + "[" + std::to_string(i) + "] is NaN");
    return copy_state(a, model, s, true);
}

mmdx_status mmdx_animator_get_state(mmdx_animator_t a, mmdx_model_t model, const mmdx_animator_arrays *s) {
    if (mmdx_status r = check_state_call(a, s)) return r;
    return copy_state(a, model, s, false);
}

mmdx_status mmdx_animator_request(mmdx_animator_t a, mmdx_model_t model, uint32_t n, const uint32_t *ids, const uint32_t *clips,
                                  const float *fades, const double *start_times, uint32_t flags) {
    if (!a) return fail(MMDX_ERR_INVALID_ARGUMENT, "animator is NULL");
    if (flags & ~uint32_t(MMDX_TIMES_ON_DEVICE)) return fail(MMDX_ERR_INVALID_ARGUMENT, "unknown flag bits");
    if (!n) return MMDX_OK;
    if (!ids || !clips) return fail(MMDX_ERR_INVALID_ARGUMENT, "ids / clips is NULL");
    const bool on_device = (flags & MMDX_TIMES_ON_DEVICE) != 0;
    if (on_device) {
        const uintptr_t four = reinterpret_cast<uintptr_t>(ids) | reinterpret_cast<uintptr_t>(clips) | reinterpret_cast<uintptr_t>(fades);
        if ((four & 3) || (reinterpret_cast<uintptr_t>(start_times) & 7))
            return fail(MMDX_ERR_INVALID_ARGUMENT, "device ids / clips / fades must be 4-byte aligned, start_times 8-byte aligned");
    } else {
        if (n > a->ni) return fail(MMDX_ERR_INVALID_ARGUMENT, "more requests than instances: the ids of one call must be distinct");
        for (uint32_t j = 0; j < n; ++j)
            if (ids[j] >= a->ni)
                return fail(MMDX_ERR_BAD_INDEX, "ids[" + std::to_string(j) + "] = " + std::to_string(ids[j]) + ": the animator has " +
                                                std::to_string(a->ni) + " instances");
        for (uint32_t j = 0; j < n; ++j)
            if (!valid_clip(a, clips[j]))
                return fail(MMDX_ERR_BAD_INDEX, "clips[" + std::to_string(j) + "] = " + std::to_string(clips[j]) + ": the set has " +
                                                std::to_string(a->n_clips) + " clips");
        for (uint32_t j = 0; j < n; ++j) {
            if (fades && fades[j] != fades[j]) return fail(MMDX_ERR_INVALID_ARGUMENT, "fades[" + std::to_string(j) + "] is NaN");
            if (start_times && is_nan(start_times[j])) return fail(MMDX_ERR_INVALID_ARGUMENT, "start_times[" + std::to_string(j) + "] is NaN");
        }
    }
    int device;
    hipStream_t st;
    if (mmdx_status r = resolve_stream(model, &device, &st)) return r;
    if (graph_recording() && !on_device)
        return fail(MMDX_ERR_INVALID_ARGUMENT, "while a graph is being recorded the request lists must be in device memory");
    if (mmdx_status r = state_to_device(a, device)) return r;
    graph_note_handle(model, &a->pin);
    AnimRequests r{ids, clips, fades, start_times, n};
    if (!on_device) {
        const size_t bytes = size_t(n) * kRequestBytes;
        a->req_host.assign(bytes, 0);
        char *h = a->req_host.data();
        std::memcpy(h + size_t(n) * 8, ids, size_t(n) * 4);
        std::memcpy(h + size_t(n) * 12, clips, size_t(n) * 4);
        if (start_times) std::memcpy(h, start_times, size_t(n) * 8);
        if (fades) std::memcpy(h + size_t(n) * 16, fades, size_t(n) * 4);
        HIP_TRY(hipMemcpyAsync(a->req, h, bytes, hipMemcpyHostToDevice, st));
        const char *d = static_cast<const char *>(a->req);
        r.times = reinterpret_cast<const double *>(d);
        r.ids = reinterpret_cast<const uint32_t *>(d + size_t(n) * 8);
        r.clips = r.ids + n;
        r.fades = reinterpret_cast<const float *>(r.ids + size_t(n) * 2);
    }
    HIP_TRY(launch_animator_request(a->arrays, r, st));
    if (!on_device) HIP_TRY(wait_stream(st));     // the staging image must be consumed before the next call rewrites it
    return MMDX_OK;
}

mmdx_status mmdx_animator_advance(mmdx_animator_t a, mmdx_model_t model, const double *dt, uint32_t flags) {
    if (!a || !dt) return fail(MMDX_ERR_INVALID_ARGUMENT, "animator / dt is NULL");
    if (flags & ~uint32_t(MMDX_ANIM_DT_ON_DEVICE)) return fail(MMDX_ERR_INVALID_ARGUMENT, "unknown flag bits");
    const bool on_device = (flags & MMDX_ANIM_DT_ON_DEVICE) != 0;
    if (on_device) {
        if (reinterpret_cast<uintptr_t>(dt) & 7) return fail(MMDX_ERR_INVALID_ARGUMENT, "a device dt must be 8-byte aligned");
    } else if (is_nan(*dt)) {
        return fail(MMDX_ERR_INVALID_ARGUMENT, "dt is NaN");
    }
    int device;
    hipStream_t st;
    if (mmdx_status r = resolve_stream(model, &device, &st)) return r;
    if (mmdx_status r = state_to_device(a, device)) return r;
    graph_note_handle(model, &a->pin);
    HIP_TRY(launch_animator_advance(a->arrays, a->table, on_device ? 0.0 : *dt, on_device ? dt : nullptr, st));
    return MMDX_OK;
}

}  // extern "C"

// mmdx_animator_root_motion and mmdx_animator_root_motion_turn: two structs with the same fields, one set of rules.  `turn` picks
// the kernel that also moves the heading; `allowed` is what the call accepts in flags.
template <class Args>
static mmdx_status root_motion_call(mmdx_animator_t a, mmdx_motion_set_t set, mmdx_model_t model, const Args *args, const char *size_error,
                                    uint32_t allowed, bool turn) {
    if (!a || !set || !args) return fail(MMDX_ERR_INVALID_ARGUMENT, "animator / set / args is NULL");
    if (args->struct_size != sizeof(Args)) return fail(MMDX_ERR_INVALID_ARGUMENT, size_error);
    if (!args->dt || !args->placements) return fail(MMDX_ERR_INVALID_ARGUMENT, "dt / placements is NULL");
    if (args->flags & ~allowed) return fail(MMDX_ERR_INVALID_ARGUMENT, "unknown flag bits");
    if (args->axes & ~uint32_t(MMDX_ROOT_X | MMDX_ROOT_Y | MMDX_ROOT_Z)) return fail(MMDX_ERR_INVALID_ARGUMENT, "unknown axes bits");
    const SetBoneSide side = motion_set_bone_side(set);
    if (!side.has_bones) return fail(MMDX_ERR_INVALID_ARGUMENT, "this motion set was created without bone motions");
    if (side.n_clips != a->n_clips)
        return fail(MMDX_ERR_INVALID_ARGUMENT, "the set has " + std::to_string(side.n_clips) + " clips, the animator's table " +
                                               std::to_string(a->n_clips));
    if (args->root_bone >= side.nb)
        return fail(MMDX_ERR_BAD_INDEX, "root_bone = " + std::to_string(args->root_bone) + ": the set has " + std::to_string(side.nb) + " bones");
    if (reinterpret_cast<uintptr_t>(args->placements) & 3) return fail(MMDX_ERR_INVALID_ARGUMENT, "placements must be 4-byte aligned");
    const bool on_device = (args->flags & MMDX_ANIM_DT_ON_DEVICE) != 0;
    if (on_device) {
        if (reinterpret_cast<uintptr_t>(args->dt) & 7) return fail(MMDX_ERR_INVALID_ARGUMENT, "a device dt must be 8-byte aligned");
    } else if (is_nan(*args->dt)) {
        return fail(MMDX_ERR_INVALID_ARGUMENT, "dt is NaN");
    }
    int device;
    hipStream_t st;
    if (mmdx_status r = resolve_stream(model, &device, &st)) return r;
    if (mmdx_status r = refuse_recording(0, 0, device, {side.device},
                                         "while a graph is being recorded the motion set must have run on this device before"))
        return r;
    if (mmdx_status r = state_to_device(a, device)) return r;
    BoneTrackParams p;
    if (mmdx_status r = motion_set_bone_tables(set, model, device, &p)) return r;
    graph_note_handle(model, &a->pin);
    const AnimArrays &s = a->arrays;
    const RootMotionParams rp{s.clips_a, s.clips_b, s.times_a, s.times_b, s.weights, s.speed, s.fade_rate, s.ni, a->table,
                              args->root_bone, args->axes, args->placements};
    const double dt = on_device ? 0.0 : *args->dt;
    const double *dt_dev = on_device ? args->dt : nullptr;
    if (turn) HIP_TRY(launch_animator_root_turn(p, rp, (args->flags & MMDX_ROOT_NORMALIZE) != 0, dt, dt_dev, st));
    else HIP_TRY(launch_animator_root_motion(p, rp, dt, dt_dev, st));
    return MMDX_OK;
}

extern "C" {

mmdx_status mmdx_animator_root_motion(mmdx_animator_t a, mmdx_motion_set_t set, mmdx_model_t model, const mmdx_root_motion_args *args) {
    return root_motion_call(a, set, model, args, "mmdx_root_motion_args.struct_size mismatch", uint32_t(MMDX_ANIM_DT_ON_DEVICE), false);
}

mmdx_status mmdx_animator_root_motion_turn(mmdx_animator_t a, mmdx_motion_set_t set, mmdx_model_t model, const mmdx_root_turn_args *args) {
    return root_motion_call(a, set, model, args, "mmdx_root_turn_args.struct_size mismatch",
                            uint32_t(MMDX_ANIM_DT_ON_DEVICE | MMDX_ROOT_NORMALIZE), true);
}

}  // extern "C"

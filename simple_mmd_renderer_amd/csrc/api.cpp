// api.cpp -- the C ABI of include/mmdx.h over the HIP runtime.  Host side of the drop-in boundary:
// validates and compiles the model once (plan.cpp), keeps the static streams resident in HBM, and
// turns one mmdx_deform*() call into at most three launches on the handle's stream:
//     [flatten group morphs -> slot weights] -> [shared morph pass] -> deform (skin + write-out).
// There is NO CPU fallback: without a usable HIP device every compute entry point fails loudly.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <chrono>
#include <cstring>
#include <mutex>
#include <new>
#include <string>
#include <thread>
#include <vector>

#include "api_internal.hpp"

using namespace mmdx;

namespace {

// Device selection follows hipSetDevice's model: mmdx_device_select() binds the CALLING THREAD (one host thread per
// device may each select its own and create / run its models concurrently) and also becomes the default of
// threads that never selected one (a process that selects once in its main thread and works from a pool).
std::atomic<int> g_default_device{0};
thread_local int tl_device = -1;
int current_device() { return tl_device >= 0 ? tl_device : g_default_device.load(std::memory_order_relaxed); }
std::once_flag g_prepare_once[16];
hipError_t g_prepare_status[16];



// Streams of this thread that are recording a graph (hipStreamCaptureModeThreadLocal: begin and end happen on one thread,
// mmdx_graph_end enforces it): while > 0 nothing on this thread may allocate, copy from the host or wait.
thread_local int tl_recording_depth = 0;

}  // namespace


struct mmdx_graph_s {
    void *exec = nullptr;      // hipGraphExec_t
    void *stream = nullptr;    // the model's stream at recording time
    int device = 0;
    std::atomic<bool> valid{true};        // false once a handle it was recorded from has been destroyed
    std::vector<GraphPin *> pins;         // those handles (guarded by g_graph_mu)
};

namespace {
std::mutex g_graph_mu;          // graph <-> handle links (rare operations: record, destroy)
}
void mmdx::graph_note_handle(mmdx_model_s *model, GraphPin *pin) {
    if (!model || !model->capturing || !pin) return;
    std::lock_guard<std::mutex> lk(g_graph_mu);
    if (std::find(model->rec_pins.begin(), model->rec_pins.end(), pin) == model->rec_pins.end()) {
        model->rec_pins.push_back(pin);
        pin->recorders.push_back(model);
    }
}
void mmdx::graph_drop_handle(GraphPin *pin) {
    std::lock_guard<std::mutex> lk(g_graph_mu);
    for (mmdx_model_s *rec : pin->recorders) {        // a recording in progress used this handle: it can no longer become a graph
        rec->rec_pins.erase(std::remove(rec->rec_pins.begin(), rec->rec_pins.end(), pin), rec->rec_pins.end());
        rec->rec_poisoned = true;
    }
    pin->recorders.clear();
    for (mmdx_graph_s *g : pin->graphs) {
        g->valid.store(false, std::memory_order_release);
        g->pins.erase(std::remove(g->pins.begin(), g->pins.end(), pin), g->pins.end());
    }
    pin->graphs.clear();
    pin->pins.store(0, std::memory_order_release);
}

namespace {

constexpr size_t kMaxProfiledCalls = 1 << 16;

// The device-side address of a host pointer that lies in page-locked, device-mapped memory; nullptr for
// pageable memory (and for device memory: callers pass that with the *_ON_DEVICE flags).  MMDX_HOST_DIRECT=0
// turns the direct path off (A/B against the staging copy).
bool host_direct_enabled() {
    static const bool enabled = [] { const char *e = std::getenv("MMDX_HOST_DIRECT"); return !(e && e[0] == '0'); }();
    return enabled;
}
// What a pointer handed over WITHOUT an *_ON_DEVICE flag is: pageable host memory (unknown to the runtime),
// page-locked host memory (`*mapped` = its device-side address; interior pointers are fine, the offset carries
// over), or device memory -- a caller's mistake that must not reach a CPU memcpy.
enum class PtrKind { Pageable, Mapped, Device };
PtrKind classify_pointer(const void *p, void **mapped) {
    *mapped = nullptr;
    hipPointerAttribute_t attr;
    if (!p || hipPointerGetAttributes(&attr, p) != hipSuccess) {
        (void)hipGetLastError();                    // pageable memory: "invalid value", not an error of ours
        return PtrKind::Pageable;
    }
    if (attr.type == hipMemoryTypeDevice) return PtrKind::Device;
    if (attr.type != hipMemoryTypeHost) return PtrKind::Pageable;
    if (hipHostGetDevicePointer(mapped, const_cast<void *>(p), 0) != hipSuccess) {
        (void)hipGetLastError();
        *mapped = nullptr;
        return PtrKind::Pageable;
    }
    return PtrKind::Mapped;
}
void *mapped_host_pointer(const void *host) {
    void *dev = nullptr;
    if (!host_direct_enabled()) return nullptr;
    (void)classify_pointer(host, &dev);
    return dev;
}

// Host-to-device copy of a per-call input.  Small pageable inputs (one frame's palette, its rates) are first
// copied by the CPU into the model's page-locked bounce buffer -- slot `slot_off` of it, the palette and the rates
// use different halves -- so the copy command is a plain DMA instead of the runtime's pageable path.  The previous
// call's copy out of the same slot has completed: every call with host inputs waits on the stream before it returns.
constexpr size_t kBounceInBytes = size_t(256) << 10;
hipError_t copy_in(mmdx_model_s *m, void *dst, const void *src, PtrKind kind, size_t bytes, size_t slot_off,
                   hipStream_t st) {
    if (!bytes) return hipSuccess;
    if (bytes <= kBounceInBytes / 2 && host_direct_enabled() && kind == PtrKind::Pageable) {
        if (!m->bounce_in && hipHostMalloc(&m->bounce_in, kBounceInBytes, hipHostMallocDefault) != hipSuccess) {
            (void)hipGetLastError();
            m->bounce_in = nullptr;
        }
        if (m->bounce_in) {
            void *slot = static_cast<unsigned char *>(m->bounce_in) + slot_off;
            std::memcpy(slot, src, bytes);
            return hipMemcpyAsync(dst, slot, bytes, hipMemcpyHostToDevice, st);
        }
    }
    return hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, st);
}



// every static stream and the two buffers of the shared morph pass; their sizes are mmdx_model_info.device_bytes
mmdx_status upload_model(mmdx_model_s *m) {
    Plan &p = m->plan;
    HIP_TRY(m->tiles.upload(p.tiles));
    if (p.f16) HIP_TRY(m->spos.upload(p.spos16)); else HIP_TRY(m->spos.upload(p.spos));
    HIP_TRY(m->snrm.upload(p.snrm));
    HIP_TRY(m->suv.upload(p.suv));
    HIP_TRY(m->perm.upload(p.perm));
    HIP_TRY(m->skin1.upload(p.skin1));
    HIP_TRY(m->skin2_ids.upload(p.skin2_ids));
    HIP_TRY(m->skin2_w.upload(p.skin2_w));
    HIP_TRY(m->skin4_ids.upload(p.skin4_ids));
    HIP_TRY(m->skin4_w.upload(p.skin4_w));
    HIP_TRY(m->bone_list.upload(p.bone_list));
    HIP_TRY(m->ell.upload(p.ell));
    if (p.f16) HIP_TRY(m->entries.upload(p.entries16)); else HIP_TRY(m->entries.upload(p.entries));
    HIP_TRY(m->slot_top.upload(p.slot_top));
    HIP_TRY(m->chain_off.upload(p.chain_off));
    HIP_TRY(m->chain_rate.upload(p.chain_rate));
    HIP_TRY(m->bone_boxes.upload(bone_box_device_table(p)));
    if (p.ns) {
        HIP_TRY(m->morphed.ensure(size_t(p.nv) * 12));
        // which rates `morphed` was last computed from (kernels.hpp, RatesSeen): nothing yet
        const size_t seen_bytes = (size_t(kSeenRates) + p.nm) * 4;
        HIP_TRY(m->seen.ensure(seen_bytes));
        HIP_TRY(hipMemset(m->seen.ptr, 0, seen_bytes));
        HIP_TRY(hipStreamSynchronize(nullptr));
    }
    for (const DevBuf *b : {&m->tiles, &m->spos, &m->snrm, &m->suv, &m->perm, &m->skin1, &m->skin2_ids, &m->skin2_w, &m->skin4_ids,
                            &m->skin4_w, &m->bone_list, &m->ell, &m->entries, &m->slot_top, &m->chain_off, &m->chain_rate,
                            &m->bone_boxes, &m->morphed, &m->seen})
        m->device_bytes += b->bytes;
    return MMDX_OK;
}

void free_model(mmdx_model_s *m) {
    graph_drop_handle(&m->pin);              // graphs recorded from this model hold addresses that are about to be freed
    socket_sets_forget_model(m);             // ... and its socket sets hold the handle itself
    if (m->device >= 0) {
        (void)hipSetDevice(m->device);
        for (DevBuf *b : {&m->tiles, &m->spos, &m->snrm, &m->suv, &m->perm, &m->skin1, &m->skin2_ids,
                          &m->skin2_w, &m->skin4_ids, &m->skin4_w, &m->bone_list, &m->ell,
                          &m->entries, &m->slot_top, &m->chain_off, &m->chain_rate, &m->pal, &m->rates,
                          &m->wslot, &m->morphed, &m->seen, &m->out_a, &m->out_b, &m->bnd, &m->sel, &m->cull,
                          &m->place_in, &m->place_w, &m->place_out, &m->bone_boxes, &m->pbounds_in, &m->pbounds_out,
                          &m->blend_a, &m->blend_b, &m->blend_p, &m->blend_out, &m->blend_sel})
            b->release();
        if (m->bounce) (void)hipHostFree(m->bounce);
        if (m->bounce_in) (void)hipHostFree(m->bounce_in);
        for (hipEvent_t ev : {m->ev_t0, m->ev_t1, m->ev_switch})
            if (ev) (void)hipEventDestroy(ev);
        for (hipEvent_t ev : m->prof_events) (void)hipEventDestroy(ev);
        if (m->own_stream) (void)hipStreamDestroy(m->own_stream);
    }
    delete m;
}

size_t out_bytes_a(uint32_t layout, uint64_t nvi) {
    return size_t(layout == MMDX_OUT_SOA ? nvi * 12 : (layout == MMDX_OUT_VERTEX32 ? nvi * 32 : nvi * 6));
}
size_t out_bytes_b(uint32_t layout, uint64_t nvi) {
    return size_t(layout == MMDX_OUT_VERTEX32 ? 0 : nvi * 12);
}

}  // namespace


// ---- shared with bench_api.cpp (api_internal.hpp) -----------------------------------------------------------------------
mmdx_status mmdx::hip_fail(hipError_t e, const char *what) {
    // leave no sticky error behind for the next call
    (void)hipGetLastError();
    // the two refusals of DevBuf::ensure (no HIP call failed)
    if (e == hipErrorIllegalState)
        return fail(MMDX_ERR_INVALID_ARGUMENT, std::string(what) + ": a scratch buffer of this handle would have to grow, but a recorded "
                    "graph (mmdx_graph_*) holds its address -- destroy the graph first, or size the buffers with an un-recorded call of "
                    "the largest shape before recording");
    if (e == hipErrorStreamCaptureUnsupported)
        return fail(MMDX_ERR_INVALID_ARGUMENT, std::string(what) + ": this call would have to allocate device memory while a graph is "
                    "being recorded -- run the same sequence once un-recorded first");
    return fail(e == hipErrorOutOfMemory ? MMDX_ERR_OUT_OF_MEMORY
                                         : (e == hipErrorNoDevice ? MMDX_ERR_NO_DEVICE : MMDX_ERR_HIP),
                std::string(what) + ": " + hipGetErrorName(e) + " (" + hipGetErrorString(e) + ")");
}

int mmdx::env_int(const char *name, int dflt) {
    const char *s = std::getenv(name);
    return s && *s ? std::atoi(s) : dflt;
}

LaunchOverrides mmdx::read_launch_overrides() {
    return {env_int("MMDX_INTERLEAVE", 1), env_int("MMDX_THREADS", 0), env_int("MMDX_LDS_TARGET", 0),
            env_int("MMDX_GROUP", 0), env_int("MMDX_PLACEMENT_LOG", 0), env_int("MMDX_PLACEMENT_PARK", 0),
            env_int("MMDX_FRAME_KERNEL", 1), env_int("MMDX_FRAME_THREADS", 256), env_int("MMDX_SHARED_FUSED", 1),
            env_int("MMDX_STORE_WT", -1), env_int("MMDX_MORPH_AUTOSKIP", 1), env_int("MMDX_FUSED_PACK", 0), env_int("MMDX_STAGGER", 0),
            env_int("MMDX_SELECT_INTERLEAVE", 1)};
}
LaunchOverrides &mmdx::launch_overrides() {
    static LaunchOverrides o = read_launch_overrides();
    return o;
}

// The device side of a morph motion (vmd.cpp keeps the pointer and knows nothing of HIP): its tables, and the scratch of callers
// with host operands -- `frames_in` grows to 8 bytes per instance, room for the double times of mmdx_morph_motion_eval_time.
struct mmdx::MorphMotionDevice {
    DevBuf key_off, frames, weights, frames_in, out;
    int device = -1;
    GraphPin pin;                 // recorded graphs that hold these addresses
    std::array<DevBuf *, 5> all() { return {&key_off, &frames, &weights, &frames_in, &out}; }
    MorphMotionDevice() {
        for (DevBuf *b : all()) b->pin = &pin;
        out.floor = 16;
    }
};

void mmdx::morph_motion_release_device(MorphMotionDevice &d) {
    graph_drop_handle(&d.pin);               // graphs that hold these addresses can no longer be replayed
    if (d.device >= 0) (void)hipSetDevice(d.device);
    for (DevBuf *b : d.all()) b->release();
    delete &d;
}

// A stream that is recording takes calls from the recording thread only: the "nothing may allocate / copy from the host / wait"
// guards are per thread (thread-local capture mode), a call from another thread would slip past them.
static mmdx_status recording_thread_check(mmdx_model_t model) {
    if (model && model->capturing && model->capture_thread != std::this_thread::get_id())
        return fail(MMDX_ERR_INVALID_ARGUMENT, "this model's stream is recording a graph on another thread: recorded calls must come "
                                               "from the thread that called mmdx_graph_begin");
    return MMDX_OK;
}

static mmdx_status refuse_host_only(mmdx_model_t m) {
    if (m->device < 0)
        return fail(MMDX_ERR_NO_DEVICE, "model was created with MMDX_CREATE_HOST_ONLY: nothing to run on "
                                        "(this engine has no CPU fallback)");
    return MMDX_OK;
}

mmdx_status mmdx::model_call_begin(mmdx_model_t m, uint32_t flags, uint32_t need, const char *text) {
    if (mmdx_status st = refuse_host_only(m)) return st;
    if (mmdx_status st = recording_thread_check(m)) return st;
    if (mmdx_status st = refuse_recording(flags, need, m->device, {}, text)) return st;
    HIP_TRY(hipSetDevice(m->device));
    return MMDX_OK;
}

mmdx_status mmdx::resolve_stream(mmdx_model_t model, int *device, hipStream_t *stream) {
    if (mmdx_status st = recording_thread_check(model)) return st;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0)
        return fail(MMDX_ERR_NO_DEVICE, "no HIP device available (motion and rig evaluation run on the GPU)");
    const bool on_model = model && model->device >= 0;
    *device = on_model ? model->device : current_device();
    *stream = on_model ? model->stream : nullptr;
    HIP_TRY(hipSetDevice(*device));
    return MMDX_OK;
}
bool mmdx::graph_recording() { return tl_recording_depth > 0; }
// hipFree is one of the calls the runtime refuses on a thread whose stream is recording (it would also invalidate the recording):
// a handle destroyed in that window parks its blocks here, mmdx_graph_end frees them.
static thread_local std::vector<void *> tl_deferred_free;
// ... and so are the stream / event / page-locked-memory calls of a whole handle's teardown: a model destroyed on a thread that is
// recording (another model's graph) is only cut off from its graphs here; its resources go at mmdx_graph_end.
static thread_local std::vector<mmdx_model_s *> tl_deferred_models;
void mmdx::device_free_or_defer(void *ptr) {
    if (!ptr) return;
    if (tl_recording_depth > 0) tl_deferred_free.push_back(ptr);
    else (void)hipFree(ptr);
}

// The wait at the end of a call that hands results back to the host.  A per-frame call is tens of
// microseconds of device work; hipStreamSynchronize may put the thread to sleep and then pays a wake-up that is
// several times that on some hosts (tools/archive/probes/host_io_probe.py), so poll the stream first and only fall back to the
// blocking wait when the work is long.  MMDX_SPIN_WAIT_US: polling budget in microseconds (default 2000, 0 = off).
hipError_t mmdx::wait_stream(hipStream_t stream) {
    static const int spin_us = env_int("MMDX_SPIN_WAIT_US", 2000);
    if (spin_us > 0) {
        const auto t0 = std::chrono::steady_clock::now();
        for (;;) {
            const hipError_t e = hipStreamQuery(stream);
            if (e != hipErrorNotReady) return e;
            if (std::chrono::steady_clock::now() - t0 > std::chrono::microseconds(spin_us)) break;
        }
    }
    return hipStreamSynchronize(stream);
}

extern "C" {

uint32_t mmdx_abi_version(void) { return MMDX_ABI_VERSION; }

mmdx_status mmdx_device_count(int32_t *count) {
    if (!count) return fail(MMDX_ERR_INVALID_ARGUMENT, "count is NULL");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) {
        *count = 0;
        return hip_fail(e, "hipGetDeviceCount");
    }
    *count = n;
    return MMDX_OK;
}

mmdx_status mmdx_device_select(int32_t ordinal) {
    int n = 0;
    HIP_TRY(hipGetDeviceCount(&n));
    if (ordinal < 0 || ordinal >= n || ordinal >= 16)
        return fail(MMDX_ERR_INVALID_ARGUMENT, "device ordinal out of range");
    HIP_TRY(hipSetDevice(ordinal));
    tl_device = ordinal;
    g_default_device.store(ordinal, std::memory_order_relaxed);
    return MMDX_OK;
}

mmdx_status mmdx_device_name(int32_t ordinal, char *buf, size_t buf_size) {
    if (!buf || !buf_size) return fail(MMDX_ERR_INVALID_ARGUMENT, "buf is NULL");
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, ordinal));
    std::snprintf(buf, buf_size, "%s %s cus=%d lds=%zu l2=%d memclk=%d buswidth=%d", prop.name,
                  prop.gcnArchName, prop.multiProcessorCount, prop.sharedMemPerBlock,
                  prop.l2CacheSize, prop.memoryClockRate, prop.memoryBusWidth);
    return MMDX_OK;
}

mmdx_status mmdx_model_create(const mmdx_model_desc *desc, mmdx_model_t *out_model) {
    if (!desc || !out_model) return fail(MMDX_ERR_INVALID_ARGUMENT, "desc / out_model is NULL");
    *out_model = nullptr;
    if (desc->struct_size == sizeof(mmdx_model_desc) &&
        (desc->flags & ~uint32_t(MMDX_CREATE_NORMALIZE | MMDX_CREATE_HOST_ONLY | MMDX_CREATE_F16_POSITIONS | MMDX_CREATE_FAST_MATH |
                                 MMDX_CREATE_TILE_ORDER)))
        return fail(MMDX_ERR_INVALID_ARGUMENT, "unknown bits in mmdx_model_desc.flags");
    mmdx_model_s *m = new (std::nothrow) mmdx_model_s;
    if (!m) return fail(MMDX_ERR_OUT_OF_MEMORY, "host allocation failed");
    std::string err;
    mmdx_status st;
    try {
        st = build_plan(*desc, m->plan, err);
    } catch (const std::bad_alloc &) {
        delete m;
        return fail(MMDX_ERR_OUT_OF_MEMORY, "host allocation failed while compiling the model");
    }
    if (st != MMDX_OK) {
        delete m;
        return fail(st, err);
    }
    if (desc->flags & MMDX_CREATE_HOST_ONLY) {
        *out_model = m;
        return MMDX_OK;
    }
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) {
        delete m;
        return fail(MMDX_ERR_NO_DEVICE,
                    "no HIP device available (this engine has no CPU fallback; use "
                    "MMDX_CREATE_HOST_ONLY to validate a model without a GPU)");
    }
    m->device = current_device();
    auto bail = [&](mmdx_status s) { free_model(m); return s; };
    if ((e = hipSetDevice(m->device)) != hipSuccess) return bail(hip_fail(e, "hipSetDevice"));
    std::call_once(g_prepare_once[m->device], [&] {
        hipError_t pe = kernel_set(false).prepare();
        g_prepare_status[m->device] = pe != hipSuccess ? pe : kernel_set(true).prepare();
    });
    if (g_prepare_status[m->device] != hipSuccess)
        return bail(hip_fail(g_prepare_status[m->device], "hipFuncSetAttribute(dynamic LDS)"));
    if ((e = hipStreamCreateWithFlags(&m->own_stream, hipStreamNonBlocking)) != hipSuccess)
        return bail(hip_fail(e, "hipStreamCreate"));
    m->stream = m->own_stream;
    for (hipEvent_t *ev : {&m->ev_t0, &m->ev_t1})
        if ((e = hipEventCreate(ev)) != hipSuccess) return bail(hip_fail(e, "hipEventCreate"));
    if ((e = hipEventCreateWithFlags(&m->ev_switch, hipEventDisableTiming)) != hipSuccess) return bail(hip_fail(e, "hipEventCreate"));
    st = upload_model(m);
    if (st != MMDX_OK) return bail(st);
    *out_model = m;
    return MMDX_OK;
}

mmdx_status mmdx_model_destroy(mmdx_model_t model) {
    if (!model) return MMDX_OK;
    if (model->capturing) {              // destroyed in the middle of a recording: end it here so that no state is left behind
        if (model->capture_thread != std::this_thread::get_id())
            return fail(MMDX_ERR_INVALID_ARGUMENT, "this model is recording a graph on another thread: end the recording there first");
        mmdx_graph_t dropped = nullptr;
        (void)mmdx_graph_end(model, &dropped);
        mmdx_graph_destroy(dropped);
    }
    if (tl_recording_depth > 0 && model->device >= 0) {
        // this thread is (still) recording another model's graph: no wait, no stream / event / host-memory call now
        graph_drop_handle(&model->pin);
        tl_deferred_models.push_back(model);
        return MMDX_OK;
    }
    if (model->device >= 0) {
        (void)hipSetDevice(model->device);
        (void)hipStreamSynchronize(model->stream);
    }
    free_model(model);
    return MMDX_OK;
}

mmdx_status mmdx_model_get_vertex_order(mmdx_model_t m, uint32_t *engine_to_original, uint32_t *original_to_engine) {
    if (!m) return fail(MMDX_ERR_INVALID_ARGUMENT, "model is NULL");
    const Plan &p = m->plan;
    for (const TileHdr &t : p.tiles)
        for (uint32_t s = 0; s < t.nv; ++s) {
            const uint32_t e = t.v0 + s, o = t.v0 + p.perm[e];
            if (engine_to_original) engine_to_original[e] = o;
            if (original_to_engine) original_to_engine[o] = e;
        }
    return MMDX_OK;
}

mmdx_status mmdx_model_get_info(mmdx_model_t m, mmdx_model_info *info) {
    if (!m || !info) return fail(MMDX_ERR_INVALID_ARGUMENT, "model / info is NULL");
    if (info->struct_size != sizeof(mmdx_model_info))
        return fail(MMDX_ERR_INVALID_ARGUMENT, "mmdx_model_info.struct_size mismatch");
    const Plan &p = m->plan;
    info->n_vertices = p.nv; info->n_bones = p.nb; info->n_morphs = p.nm;
    info->n_slots = p.ns; info->n_entries = p.ne_real; info->n_entries_padded = p.ne;
    info->n_tiles = p.ntiles; info->tile_vertices = kTileVerts;
    info->n_bdef1 = p.n1; info->n_bdef2 = p.n2; info->n_bdef4 = p.n4;
    info->max_tile_bones = p.max_tile_bones;
    info->device_bytes = m->device_bytes;
    info->device_ordinal = m->device < 0 ? 0xffffffffu : uint32_t(m->device);
    info->flags = p.flags;
    return MMDX_OK;
}

mmdx_status mmdx_model_get_skin(mmdx_model_t m, int32_t *type, int32_t *ids, float *weights) {
    if (!m || !type || !ids || !weights) return fail(MMDX_ERR_INVALID_ARGUMENT, "NULL argument");
    const Plan &p = m->plan;
    for (uint32_t i = 0; i < p.nv; ++i)
        type[i] = p.cls[i] == 0 ? MMDX_SKIN_BDEF1 : (p.cls[i] == 1 ? MMDX_SKIN_BDEF2 : MMDX_SKIN_BDEF4);
    std::memcpy(ids, p.ids.data(), size_t(p.nv) * 16);
    std::memcpy(weights, p.wts.data(), size_t(p.nv) * 16);
    return MMDX_OK;
}

mmdx_status mmdx_model_slot_weights(mmdx_model_t m, const float *rates, float *out) {
    if (!m || (m->plan.ns && (!rates || !out))) return fail(MMDX_ERR_INVALID_ARGUMENT, "NULL argument");
    flatten_slot_weights(m->plan, rates, out);
    return MMDX_OK;
}

mmdx_status mmdx_model_set_stream(mmdx_model_t m, void *hip_stream) {
    if (!m) return fail(MMDX_ERR_INVALID_ARGUMENT, "model is NULL");
    if (m->device < 0) return fail(MMDX_ERR_NO_DEVICE, "host-only model");
    if (m->capturing)
        return fail(MMDX_ERR_INVALID_ARGUMENT, "this model's stream is recording a graph: end the recording (mmdx_graph_end) before "
                                               "switching streams");
    hipStream_t next = hip_stream ? static_cast<hipStream_t>(hip_stream) : m->own_stream;
    if (next == m->stream) return MMDX_OK;
    HIP_TRY(hipSetDevice(m->device));
    if (hip_stream) {
        hipDevice_t dev = -1;
        if (hipStreamGetDevice(next, &dev) != hipSuccess) {
            (void)hipGetLastError();
            return fail(MMDX_ERR_INVALID_ARGUMENT, "hip_stream is not a HIP stream the runtime knows");
        }
        if (int(dev) != m->device)
            return fail(MMDX_ERR_INVALID_ARGUMENT, "hip_stream belongs to device " + std::to_string(int(dev)) + ", the model lives on device " +
                                                   std::to_string(m->device));
    }
    // The model's device state (morphed positions, the RatesSeen record, every scratch buffer) goes with it from one stream to the
    // next: whatever is enqueued from now on starts after everything enqueued so far.  An event, not a wait: the host never blocks.
    HIP_TRY(hipEventRecord(m->ev_switch, m->stream));
    HIP_TRY(hipStreamWaitEvent(next, m->ev_switch, 0));
    m->stream = next;
    return MMDX_OK;
}

// ---- mmdx_deform_batched, _bounds (out_bounds != nullptr) and _select (sel != nullptr; out_bounds optional there) ------------------
// deform_batched() at the end of this section reads as the list of steps; each step is one function here.

// What validation learns about the call's host pointers, for the steps that stage and route them
struct CallPointers {
    PtrKind kind_pal = PtrKind::Pageable, kind_w = PtrKind::Pageable;
    void *map_a = nullptr, *map_b = nullptr;    // device-side addresses of page-locked host outputs (nullptr: pageable)
    uint32_t sel_live_host = 0;                 // host lists: how many leading ids are in use
    uint32_t pitch = 0;                         // instance pitch of the outputs (vertices from one instance to the next); dense outputs: NV
};

// Where the kernel writes and how the results reach the caller's arrays
struct OutputRoute {
    bool out_dev = false;                       // the caller's device arrays
    bool direct = false, bounce = false;        // page-locked host memory: the caller's own, or the handle's bounce buffer
    size_t bytes_a = 0, bytes_b = 0, off_b = 0; // the two arrays; the second one's offset in the bounce buffer
};

// the instance list of a select call: validated in full before anything is enqueued.  The shared cuts (host_runtime.hpp), with this
// call's own checks between them.
static mmdx_status validate_select(mmdx_model_t m, const mmdx_deform_args *a, const mmdx_instance_select *sel, uint32_t &live_host) {
    const Plan &p = m->plan;
    if (mmdx_status st = list_header_check(sel)) return st;
    // the GPU-resident crowd form only: a staging or bounce copy of the outputs moves whole arrays and cannot leave the
    // instances outside a list untouched
    const uint32_t need = MMDX_PALETTE_ON_DEVICE | MMDX_OUT_ON_DEVICE |
                          (p.ns && a->morph_weights ? uint32_t(MMDX_WEIGHTS_ON_DEVICE) : 0u);
    if ((a->flags & need) != need)
        return fail(MMDX_ERR_INVALID_ARGUMENT, "mmdx_deform_batched_select takes device operands only: pass MMDX_PALETTE_ON_DEVICE | "
                                               "MMDX_OUT_ON_DEVICE, and MMDX_WEIGHTS_ON_DEVICE with morph_weights");
    if (mmdx_status st = list_placement_check(sel, m->capturing)) return st;
    void *unused = nullptr;
    if (!(sel->flags & MMDX_SELECT_ON_DEVICE) && ((sel->n_ids && classify_pointer(sel->ids, &unused) == PtrKind::Device) ||
                                                  (sel->count && classify_pointer(sel->count, &unused) == PtrKind::Device)))
        return fail(MMDX_ERR_INVALID_ARGUMENT, "ids / count of mmdx_instance_select point to device memory: pass "
                                               "MMDX_SELECT_ON_DEVICE");
    return host_list_check(sel, a->n_instances, live_host);
}

static mmdx_status validate_call(mmdx_model_t m, const mmdx_deform_args *a, const float *out_bounds, const mmdx_instance_select *sel,
                                 CallPointers &cp) {
    if (!m || !a) return fail(MMDX_ERR_INVALID_ARGUMENT, "model / args is NULL");
    if (a->struct_size != sizeof(mmdx_deform_args))
        return fail(MMDX_ERR_INVALID_ARGUMENT, "mmdx_deform_args.struct_size mismatch");
    if (mmdx_status st = refuse_host_only(m)) return st;
    const Plan &p = m->plan;
    const uint32_t ni = a->n_instances, layout = a->out_layout;
    if (ni == 0) return fail(MMDX_ERR_INVALID_ARGUMENT, "n_instances must be >= 1");
    if (a->flags & ~uint32_t(MMDX_PALETTE_ON_DEVICE | MMDX_WEIGHTS_ON_DEVICE | MMDX_OUT_ON_DEVICE | MMDX_WEIGHTS_SHARED | MMDX_MORPH_UNCHANGED |
                             MMDX_OUT_STORES_WRITE_THROUGH | MMDX_OUT_STORES_CACHED | MMDX_OUT_PITCHED))
        return fail(MMDX_ERR_INVALID_ARGUMENT, "unknown bits in mmdx_deform_args.flags");
    if ((a->flags & MMDX_OUT_STORES_WRITE_THROUGH) && (a->flags & MMDX_OUT_STORES_CACHED))
        return fail(MMDX_ERR_INVALID_ARGUMENT, "MMDX_OUT_STORES_WRITE_THROUGH and MMDX_OUT_STORES_CACHED exclude each other");
    if (layout > MMDX_OUT_SOA_POS16) return fail(MMDX_ERR_INVALID_ARGUMENT, "unknown out_layout");
    if (p.f16 != (layout == MMDX_OUT_SOA_POS16))
        return fail(MMDX_ERR_UNSUPPORTED, "MMDX_OUT_SOA_POS16 goes with MMDX_CREATE_F16_POSITIONS models "
                                          "(and only with them)");
    if (!a->palettes || !a->out_a || (layout != MMDX_OUT_VERTEX32 && !a->out_b))
        return fail(MMDX_ERR_INVALID_ARGUMENT, "palettes / out_a / out_b is NULL");
    if (p.ns && !a->morph_weights && !(a->flags & MMDX_MORPH_UNCHANGED))
        return fail(MMDX_ERR_INVALID_ARGUMENT, "morph_weights is NULL");
    if (sel)
        if (mmdx_status sst = validate_select(m, a, sel, cp.sel_live_host)) return sst;
    const bool pitched = (a->flags & MMDX_OUT_PITCHED) != 0;
    const uint32_t pitch = cp.pitch = pitched ? a->out_instance_pitch : p.nv;
    if (pitched && pitch < p.nv)
        return fail(MMDX_ERR_INVALID_ARGUMENT, "mmdx_deform_args.out_instance_pitch is smaller than the model's vertex count");
    if (pitched && (uint64_t(ni) - 1) * pitch + p.nv > uint64_t(SIZE_MAX) / 32)
        return fail(MMDX_ERR_INVALID_ARGUMENT, "mmdx_deform_args.out_instance_pitch: the output span overflows");
    // host arguments: what kind of memory they are (device memory without its *_ON_DEVICE flag is a caller's
    // mistake that would otherwise end in a CPU memcpy from / to a device address)
    void *map_unused = nullptr;
    if (!(a->flags & MMDX_PALETTE_ON_DEVICE) && (cp.kind_pal = classify_pointer(a->palettes, &map_unused)) == PtrKind::Device)
        return fail(MMDX_ERR_INVALID_ARGUMENT, "palettes points to device memory: pass MMDX_PALETTE_ON_DEVICE");
    if (p.ns && !(a->flags & MMDX_WEIGHTS_ON_DEVICE) &&
        (cp.kind_w = classify_pointer(a->morph_weights, &map_unused)) == PtrKind::Device)
        return fail(MMDX_ERR_INVALID_ARGUMENT, "morph_weights points to device memory: pass MMDX_WEIGHTS_ON_DEVICE");
    if (!(a->flags & MMDX_OUT_ON_DEVICE)) {
        PtrKind kind_b = PtrKind::Pageable;
        const PtrKind kind_a = classify_pointer(a->out_a, &cp.map_a);
        if (layout != MMDX_OUT_VERTEX32) kind_b = classify_pointer(a->out_b, &cp.map_b);
        if (kind_a == PtrKind::Device || kind_b == PtrKind::Device)
            return fail(MMDX_ERR_INVALID_ARGUMENT, "out_a / out_b points to device memory: pass MMDX_OUT_ON_DEVICE");
        if (!host_direct_enabled()) cp.map_a = cp.map_b = nullptr;
    }
    // bounds live where the outputs live
    if (out_bounds && (a->flags & MMDX_OUT_ON_DEVICE) && (reinterpret_cast<uintptr_t>(out_bounds) & 3))
        return fail(MMDX_ERR_INVALID_ARGUMENT, "device out_bounds must be 4-byte aligned");
    if (out_bounds && !(a->flags & MMDX_OUT_ON_DEVICE) && classify_pointer(out_bounds, &map_unused) == PtrKind::Device)
        return fail(MMDX_ERR_INVALID_ARGUMENT, "out_bounds points to device memory: pass MMDX_OUT_ON_DEVICE");
    // (the host-only refusal answered further up, where this call has always had it.  Only a recording of THIS model's stream
    // refuses host operands here: a thread that records another model's graph may still deform this one from the host.)
    const uint32_t need = MMDX_PALETTE_ON_DEVICE | MMDX_OUT_ON_DEVICE | (p.ns ? uint32_t(MMDX_WEIGHTS_ON_DEVICE) : 0u);
    if (mmdx_status st = model_call_begin(m, a->flags, m->capturing ? need : 0u,
                                          "while a graph is being recorded every operand must be in device memory"))
        return st;
    if (m->capturing && m->profile) return fail(MMDX_ERR_INVALID_ARGUMENT, "mmdx_profile_enable and graph recording exclude each other");
    return MMDX_OK;
}

// `pev`: {skin0, skin1, morph0, morph1} of this call when it is one of the profiled ones, else nullptr
static mmdx_status profile_events(mmdx_model_t m, hipEvent_t *&pev) {
    pev = nullptr;
    // a full recording (kMaxProfiledCalls without mmdx_profile_collect) stops recording; it never fails the call
    if (m->profile && m->prof_calls < kMaxProfiledCalls && m->prof_seen++ % m->profile_stride == 0) {
        while (m->prof_events.size() < 4 * (m->prof_calls + 1)) {
            hipEvent_t ev;
            HIP_TRY(hipEventCreate(&ev));
            m->prof_events.push_back(ev);
        }
        pev = m->prof_events.data() + 4 * m->prof_calls;
    }
    return MMDX_OK;
}

// The kernel arguments that depend on the model alone; every per-call field zero
static DeformParams static_params(const mmdx_model_s &m) {
    const Plan &p = m.plan;
    DeformParams dp;
    std::memset(&dp, 0, sizeof(dp));
    dp.tiles = static_cast<const TileHdr *>(m.tiles.ptr);
    dp.spos = m.spos.ptr;
    dp.snrm = static_cast<const float *>(m.snrm.ptr);
    dp.suv = static_cast<const float *>(m.suv.ptr);
    dp.perm = static_cast<const uint16_t *>(m.perm.ptr);
    dp.skin1 = static_cast<const uint16_t *>(m.skin1.ptr);
    dp.skin2_ids = static_cast<const uint32_t *>(m.skin2_ids.ptr);
    dp.skin2_w = static_cast<const float *>(m.skin2_w.ptr);
    dp.skin4_ids = static_cast<const uint2 *>(m.skin4_ids.ptr);
    dp.skin4_w = static_cast<const float4 *>(m.skin4_w.ptr);
    dp.bone_list = static_cast<const uint32_t *>(m.bone_list.ptr);
    dp.ell = static_cast<const uint2 *>(m.ell.ptr);
    dp.entries = m.entries.ptr;
    dp.nv = p.nv; dp.nb = p.nb; dp.ns = p.ns;
    dp.pal_stride = p.max_tile_bones * 3;
    dp.finite_offsets = p.finite_offsets ? 1u : 0u;
    dp.interleave = uint32_t(launch_overrides().interleave);
    dp.tile_order = (p.flags & MMDX_CREATE_TILE_ORDER) ? 1u : 0u;
    return dp;
}

// The instance list of a select call: device lists are used in place -- a recorded graph reads them afresh at every replay; host
// lists go to a scratch of the handle in stream order, count word first
static mmdx_status stage_select(mmdx_model_t m, const mmdx_instance_select *sel, uint32_t live_host, DeformParams &dp) {
    dp.sel_n = sel->n_ids;
    dp.sel_interleave = launch_overrides().select_interleave != 0 ? 1u : 0u;
    if (sel->flags & MMDX_SELECT_ON_DEVICE) {
        dp.sel_ids = sel->ids; dp.sel_count = sel->count;
    } else if (sel->n_ids) {                    // all n_ids ids travel: the kernel is sized from the capacity
        return stage_list(m->sel, m->sel_host, sel->ids, sel->n_ids, live_host, m->stream, &dp.sel_count, &dp.sel_ids);
    }
    return MMDX_OK;
}

static mmdx_status stage_palettes(mmdx_model_t m, const mmdx_deform_args *a, PtrKind kind_pal, DeformParams &dp) {
    const size_t pal_bytes = size_t(a->n_instances) * m->plan.nb * 64;
    if (a->flags & MMDX_PALETTE_ON_DEVICE) {
        if (reinterpret_cast<uintptr_t>(a->palettes) & 15)
            return fail(MMDX_ERR_INVALID_ARGUMENT, "device palettes must be 16-byte aligned");
        dp.palettes = a->palettes;
    } else {
        HIP_TRY(m->pal.ensure(pal_bytes));
        HIP_TRY(copy_in(m, m->pal.ptr, a->palettes, kind_pal, pal_bytes, 0, m->stream));
        dp.palettes = static_cast<const float *>(m->pal.ptr);
    }
    return MMDX_OK;
}

// The morph step: takes a replay's news into the handle's record, plans (plan_morph_pass, launch_shape.hpp: the morph mode, the pass
// in front of the deform kernel, what becomes of the records), then does what the plan says -- uploads the rates, launches the pass,
// fills the morph fields of `dp`.  The handle's record of what `morphed` holds (morphed_valid, host_rates) is written in one block
// behind the last launch: a call that fails in here leaves the record it found.
static mmdx_status run_morph_pass(mmdx_model_t m, const mmdx_deform_args *a, const mmdx_instance_select *sel, PtrKind kind_w,
                                  hipEvent_t *pev, DeformParams &dp, MorphPlan &pl) {
    const Plan &p = m->plan;
    const KernelSet &ks = kernel_set((p.flags & MMDX_CREATE_FAST_MATH) != 0);
    hipStream_t st = m->stream;
    if (m->pin.replayed.exchange(false, std::memory_order_acq_rel)) m->host_rates_valid = false;   // a graph replay ran a morph pass
    const LaunchOverrides &ov = launch_overrides();
    const MorphCall call{p.ns, p.nm, a->n_instances, a->flags, sel != nullptr, sel ? sel->n_ids : 0u, ov.shared_fused, ov.morph_autoskip,
                         a->morph_weights};
    std::string err;
    if (mmdx_status s = plan_morph_pass(call, {m->morphed_valid, m->host_rates_valid, m->host_rates.data(), m->host_rates.size()}, pl, err))
        return fail(s, err);
    if (pl.host_skip) ++m->host_skips;
    if (pl.morph == kMorphNone) return MMDX_OK;
    const float *rates_dev = a->morph_weights;            // (a pass that is left out never reads them)
    if (pl.upload) {
        HIP_TRY(m->rates.ensure(size_t(pl.niw) * p.nm * 4));
        HIP_TRY(copy_in(m, m->rates.ptr, a->morph_weights, kind_w, size_t(pl.niw) * p.nm * 4, kBounceInBytes / 2, st));
        rates_dev = static_cast<const float *>(m->rates.ptr);
    }
    FlattenParams f{};
    f.rates = rates_dev;
    f.slot_top = static_cast<const uint32_t *>(m->slot_top.ptr);
    f.chain_off = static_cast<const uint32_t *>(m->chain_off.ptr);
    f.chain_rate = static_cast<const float *>(m->chain_rate.ptr);
    f.nm = p.nm; f.ns = p.ns; f.niw = pl.niw;
    f.quad = pl.quad ? 1u : 0u;
    if (pl.select_rows) f.list = {dp.sel_ids, dp.sel_count, a->n_instances};
    HIP_TRY(m->wslot.ensure(pl.wslot_rows * (size_t(p.ns) + 1) * 4));
    f.out = static_cast<float *>(m->wslot.ptr);
    uint32_t *seen = static_cast<uint32_t *>(m->seen.ptr);
    if (pl.seen == MorphPlan::kSeenCompared) f.seen = seen;
    if (pl.seen == MorphPlan::kSeenClearedByDeform) dp.morph_seen = seen;
    if (pev) HIP_TRY(hipEventRecord(pev[2], st));
    dp.wslot = f.out;
    dp.morphed = pl.withhold_morphed ? nullptr : static_cast<float *>(m->morphed.ptr);
    switch (pl.pass) {
    case MorphPlan::kNoPass:
        break;
    case MorphPlan::kFusedApply:
        HIP_TRY(ks.launch_morph_apply(p.f16, dp, &f, st));
        break;
    case MorphPlan::kFlattenApply:
        HIP_TRY(launch_flatten(f, st));
        HIP_TRY(ks.launch_morph_apply(p.f16, dp, nullptr, st));
        HIP_TRY(hipMemsetAsync(seen, 0, 4, st));
        break;
    case MorphPlan::kFlatten:
        HIP_TRY(launch_flatten(f, st));
        break;
    case MorphPlan::kGather:                              // flatten inside the deform kernel
        dp.fused_rates = rates_dev;
        dp.slot_top = f.slot_top; dp.chain_off = f.chain_off; dp.chain_rate = f.chain_rate;
        dp.nm = p.nm;
        break;
    }
    if (pev) HIP_TRY(hipEventRecord(pev[3], st));
    m->morphed_valid = pl.morphed_valid;
    if (pl.host_rates == MorphPlan::kRatesStored) m->host_rates.assign(a->morph_weights, a->morph_weights + p.nm);
    if (pl.host_rates != MorphPlan::kRatesKept) m->host_rates_valid = pl.host_rates == MorphPlan::kRatesStored;
    return MMDX_OK;
}

// Where the kernel writes (dp.out_a / out_b / out_aligned / pitch) and how the results reach the caller (`r`).
// Host outputs in page-locked, device-mapped memory (mmdx_host_malloc / hipHostMalloc / hipHostRegister): the
// kernel stores straight into them over PCIe -- 16-byte coalesced stores, overlapped with the skinning -- and
// the staging buffer plus the device-to-host copy command (~10 us of fixed cost per frame) drop out.
// Anything else goes through the staging buffer as before.
// Small outputs bound for pageable memory (a frame of one model) take the same route into a page-locked
// bounce buffer of the model's and are copied out by the CPU after the wait: the copy command into pageable
// memory is the one piece of the per-frame call whose cost varies by 100 us between hosts.
// Pitched outputs: the kernel writes them pitched where it writes the caller's arrays (device, page-locked host); the
// staging and bounce buffers stay dense and the copy out of them spreads the instances (the gap is never written).
static mmdx_status route_outputs(mmdx_model_t m, const mmdx_deform_args *a, const CallPointers &cp, DeformParams &dp, OutputRoute &r) {
    const Plan &p = m->plan;
    const uint64_t nvi = uint64_t(a->n_instances) * p.nv;
    const size_t bytes_a = r.bytes_a = out_bytes_a(a->out_layout, nvi), bytes_b = r.bytes_b = out_bytes_b(a->out_layout, nvi);
    r.out_dev = (a->flags & MMDX_OUT_ON_DEVICE) != 0;
    constexpr size_t kBounceMax = size_t(4) << 20;
    const size_t off_b = r.off_b = (bytes_a + 63) & ~size_t(63);
    if (r.out_dev) {
        dp.out_a = a->out_a; dp.out_b = a->out_b;
    } else {
        void *da = cp.map_a, *db = bytes_b ? cp.map_b : nullptr;
        r.direct = da && (!bytes_b || db);
        if (!r.direct && off_b + bytes_b <= kBounceMax && host_direct_enabled()) {
            if (m->bounce_bytes < off_b + bytes_b) {
                if (m->bounce) (void)hipHostFree(m->bounce);
                m->bounce = nullptr; m->bounce_bytes = 0; m->bounce_dev = nullptr;
                if (hipHostMalloc(&m->bounce, kBounceMax, hipHostMallocDefault) == hipSuccess) m->bounce_bytes = kBounceMax;
                else (void)hipGetLastError();
            }
            if (m->bounce) {
                if (!m->bounce_dev) m->bounce_dev = mapped_host_pointer(m->bounce);
                da = m->bounce_dev;
                r.bounce = da != nullptr;
                if (r.bounce) db = static_cast<unsigned char *>(da) + off_b;
            }
        }
        if (r.direct || r.bounce) {
            dp.out_a = da; dp.out_b = bytes_b ? db : nullptr;
        } else {
            HIP_TRY(m->out_a.ensure(bytes_a));
            if (bytes_b) HIP_TRY(m->out_b.ensure(bytes_b));
            dp.out_a = m->out_a.ptr; dp.out_b = m->out_b.ptr;
        }
    }
    dp.out_aligned = ((reinterpret_cast<uintptr_t>(dp.out_a) | reinterpret_cast<uintptr_t>(dp.out_b)) & 15) == 0;
    dp.pitch = r.out_dev || r.direct ? cp.pitch : p.nv;
    return MMDX_OK;
}

// The planned launch: the shape's fields into `dp`, the bounds scratch, the deform kernel of the shape's kind, the bounds reduce.
// bounds: the kernel's partials, then the reduce into the caller's device array -- or into the tail of the same scratch
// (`bounds_dev`), copied out to the host array next to the outputs
static mmdx_status launch_planned(mmdx_model_t m, const DeformCall &c, const LaunchShape &s, float *out_bounds, hipEvent_t *pev,
                                  DeformParams &dp, float *&bounds_dev) {
    const Plan &p = m->plan;
    const KernelSet &ks = kernel_set((p.flags & MMDX_CREATE_FAST_MATH) != 0);      // contracted multiply-adds: this model opted out of bit-exactness
    const uint32_t ni = c.ni;
    const int layout = int(c.layout), morph = c.morph;
    hipStream_t st = m->stream;
    dp.write_through = s.write_through ? 1u : 0u;
    dp.group = s.group;
    dp.stage_off = s.stage_off; dp.w_off = s.w_off; dp.mp_off = s.mp_off; dp.bounds_off = s.bounds_off;
    dp.stagger = s.stagger; dp.slots_per_cu = s.slots_per_cu;
    if (c.bounds) {
        const size_t part = size_t(c.nwork) * s.bounds_units * 24;         // (select: partials by list position)
        HIP_TRY(m->bnd.ensure(part + (c.out_dev ? 0 : size_t(ni) * 24)));
        dp.bounds = static_cast<float *>(m->bnd.ptr);
        bounds_dev = c.out_dev ? out_bounds : reinterpret_cast<float *>(static_cast<unsigned char *>(m->bnd.ptr) + part);
    }
    if (pev) HIP_TRY(hipEventRecord(pev[0], st));
    switch (s.kernel) {
    case LaunchShape::kFrame:
        dp.morphed = nullptr;                                  // nothing reads a single frame's morphed positions later
        HIP_TRY(ks.launch_frame(launch_overrides().frame_threads, layout, morph, p.f16, dp, p.ntiles, s.lds, st));
        break;
    case LaunchShape::kPack:
        HIP_TRY(ks.launch_pack(layout, p.f16, dp, p.ntiles, s.lds, st));
        break;
    case LaunchShape::kNone:
        // an empty list: no instance to write (the shared morph pass has run as in the plain call)
        break;
    case LaunchShape::kDeform:
        HIP_TRY(ks.launch_deform({s.threads, layout, morph, p.f16, dp.tile_order != 0, s.write_through, c.bounds, c.select},
                                 dp, p.ntiles, s.lds, st));
        if (c.bounds && c.select)
            HIP_TRY(launch_bounds_reduce_select(dp.bounds, s.bounds_units, ni, bounds_dev, dp.sel_ids, dp.sel_count, dp.sel_n, st));
        else if (c.bounds) HIP_TRY(launch_bounds_reduce(dp.bounds, s.bounds_units, ni, bounds_dev, st));
        break;
    }
    if (pev) {
        HIP_TRY(hipEventRecord(pev[1], st));
        if (m->prof_has_morph.size() <= m->prof_calls) m->prof_has_morph.resize(m->prof_calls + 1);
        m->prof_has_morph[m->prof_calls] = morph != kMorphNone;
        ++m->prof_calls;
    }
    return MMDX_OK;
}

// Results that the kernel did not write into the caller's arrays go there now; then the wait that a call with host operands ends in.
static mmdx_status copy_out(mmdx_model_t m, const mmdx_deform_args *a, const OutputRoute &r, uint32_t pitch, const DeformParams &dp,
                            float *out_bounds, const float *bounds_dev, bool host_inputs) {
    const Plan &p = m->plan;
    const uint32_t ni = a->n_instances, layout = a->out_layout;
    hipStream_t st = m->stream;
    if (r.out_dev) {
        if (host_inputs) HIP_TRY(wait_stream(st));      // borrowed host inputs must be consumed before we return
        return MMDX_OK;
    }
    // one instance's bytes in the dense staging / bounce buffer and in the caller's pitched arrays
    const size_t row_a = out_bytes_a(layout, p.nv), row_b = out_bytes_b(layout, p.nv);
    const size_t pitch_a = out_bytes_a(layout, pitch), pitch_b = out_bytes_b(layout, pitch);
    const bool spread = pitch != p.nv && ni > 1;
    if (!r.direct && !r.bounce) {
        if (spread) {
            HIP_TRY(hipMemcpy2DAsync(a->out_a, pitch_a, dp.out_a, row_a, row_a, ni, hipMemcpyDeviceToHost, st));
            if (r.bytes_b) HIP_TRY(hipMemcpy2DAsync(a->out_b, pitch_b, dp.out_b, row_b, row_b, ni, hipMemcpyDeviceToHost, st));
        } else {
            HIP_TRY(hipMemcpyAsync(a->out_a, dp.out_a, r.bytes_a, hipMemcpyDeviceToHost, st));
            if (r.bytes_b) HIP_TRY(hipMemcpyAsync(a->out_b, dp.out_b, r.bytes_b, hipMemcpyDeviceToHost, st));
        }
    }
    if (out_bounds) HIP_TRY(hipMemcpyAsync(out_bounds, bounds_dev, size_t(ni) * 24, hipMemcpyDeviceToHost, st));
    HIP_TRY(wait_stream(st));
    if (r.bounce && spread) {
        const unsigned char *sa = static_cast<const unsigned char *>(m->bounce), *sb = sa + r.off_b;
        for (uint32_t i = 0; i < ni; ++i) {
            std::memcpy(static_cast<unsigned char *>(a->out_a) + i * pitch_a, sa + i * row_a, row_a);
            if (r.bytes_b) std::memcpy(static_cast<unsigned char *>(a->out_b) + i * pitch_b, sb + i * row_b, row_b);
        }
    } else if (r.bounce) {
        std::memcpy(a->out_a, m->bounce, r.bytes_a);
        if (r.bytes_b) std::memcpy(a->out_b, static_cast<unsigned char *>(m->bounce) + r.off_b, r.bytes_b);
    }
    return MMDX_OK;
}

// What mmdx_debug_last_launch_shape reports: the planned shape and what launch_planned handed to the kernel of its kind
static void record_launch_shape(mmdx_model_t m, const DeformCall &c, const LaunchShape &s, const DeformParams &dp) {
    mmdx_debug_launch_shape &r = m->last_shape;
    r = mmdx_debug_launch_shape{};
    r.kernel = uint32_t(s.kernel);
    const bool tiles = s.kernel == LaunchShape::kDeform || s.kernel == LaunchShape::kPack;
    r.threads = s.kernel == LaunchShape::kFrame ? (launch_overrides().frame_threads == 128 ? 128u : 256u)
                                                : (s.kernel == LaunchShape::kPack ? 512u /* kernels.hip kPkThreads */ : uint32_t(s.threads));
    r.group = s.group;
    // launch_deform's and launch_pack's grid: a select call covers the list's capacity (c.nwork)
    r.ngroups = tiles ? ((s.kernel == LaunchShape::kPack ? c.ni : c.nwork) + s.group - 1) / s.group : 0u;
    r.lds = uint32_t(s.lds);
    r.morph = uint32_t(c.morph);
    r.layout = c.layout;
    r.f16 = m->plan.f16 ? 1u : 0u;
    r.tile_order = dp.tile_order;
    r.bounds = c.bounds ? 1u : 0u;
    r.select = c.select ? 1u : 0u;
    r.write_through = s.write_through ? 1u : 0u;
    r.interleave = dp.interleave;
    r.sel_interleave = dp.sel_interleave;
}

static mmdx_status deform_batched(mmdx_model_t m, const mmdx_deform_args *a, float *out_bounds,
                                  const mmdx_instance_select *sel = nullptr) {
    CallPointers cp;
    if (mmdx_status s = validate_call(m, a, out_bounds, sel, cp)) return s;       // ends in model_call_begin: the device is selected
    hipEvent_t *pev;
    if (mmdx_status s = profile_events(m, pev)) return s;
    DeformParams dp = static_params(*m);
    dp.ni = a->n_instances;
    dp.pos_scale = a->pos_scale;
    if (sel)
        if (mmdx_status s = stage_select(m, sel, cp.sel_live_host, dp)) return s;
    if (mmdx_status s = stage_palettes(m, a, cp.kind_pal, dp)) return s;
    MorphPlan mp;
    if (mmdx_status s = run_morph_pass(m, a, sel, cp.kind_w, pev, dp, mp)) return s;
    OutputRoute route;
    if (mmdx_status s = route_outputs(m, a, cp, dp, route)) return s;
    const DeformCall call{a->out_layout, a->n_instances, sel ? sel->n_ids : a->n_instances, a->flags, mp.morph, out_bounds != nullptr,
                          sel != nullptr, route.out_dev, route.direct || route.bounce, route.bytes_a + route.bytes_b};
    LaunchShape shape;
    std::string err;
    if (mmdx_status s = plan_deform_launch(m->plan, call, launch_overrides(), shape, err)) return fail(s, err);
    m->last_write_through = shape.write_through;
    float *bounds_dev = nullptr;
    if (mmdx_status s = launch_planned(m, call, shape, out_bounds, pev, dp, bounds_dev)) return s;
    record_launch_shape(m, call, shape, dp);
    const bool host_inputs = !(a->flags & MMDX_PALETTE_ON_DEVICE) || (mp.morph != kMorphNone && !(a->flags & MMDX_WEIGHTS_ON_DEVICE)) ||
                             (sel && !(sel->flags & MMDX_SELECT_ON_DEVICE) && sel->n_ids);
    return copy_out(m, a, route, cp.pitch, dp, out_bounds, bounds_dev, host_inputs);
}

mmdx_status mmdx_deform_batched(mmdx_model_t m, const mmdx_deform_args *a) { return deform_batched(m, a, nullptr); }

mmdx_status mmdx_deform_batched_bounds(mmdx_model_t m, const mmdx_deform_args *a, float *out_bounds) {
    if (!out_bounds) return fail(MMDX_ERR_INVALID_ARGUMENT, "out_bounds is NULL");
    return deform_batched(m, a, out_bounds);
}

mmdx_status mmdx_deform_batched_select(mmdx_model_t m, const mmdx_deform_args *a, const mmdx_instance_select *select, float *out_bounds) {
    if (!select) return fail(MMDX_ERR_INVALID_ARGUMENT, "select is NULL (mmdx_deform_batched / mmdx_deform_batched_bounds deform every instance)");
    return deform_batched(m, a, out_bounds, select);
}

mmdx_status mmdx_deform(mmdx_model_t m, const float *w, const float *palette, float *out_pos,
                        float *out_nrm) {
    mmdx_deform_args a;
    std::memset(&a, 0, sizeof(a));
    a.struct_size = sizeof(a);
    a.n_instances = 1;
    a.out_layout = MMDX_OUT_SOA;
    a.morph_weights = w; a.palettes = palette;
    a.out_a = out_pos; a.out_b = out_nrm;
    a.pos_scale = 1.0f;
    return mmdx_deform_batched(m, &a);
}

mmdx_status mmdx_deform_vertex32(mmdx_model_t m, const float *w, const float *palette,
                                 float pos_scale, void *out_vertices) {
    mmdx_deform_args a;
    std::memset(&a, 0, sizeof(a));
    a.struct_size = sizeof(a);
    a.n_instances = 1;
    a.out_layout = MMDX_OUT_VERTEX32;
    a.morph_weights = w; a.palettes = palette;
    a.out_a = out_vertices;
    a.pos_scale = pos_scale;
    return mmdx_deform_batched(m, &a);
}

mmdx_status mmdx_sync(mmdx_model_t m) {
    if (!m) return fail(MMDX_ERR_INVALID_ARGUMENT, "model is NULL");
    if (m->device < 0) return fail(MMDX_ERR_NO_DEVICE, "host-only model");
    HIP_TRY(hipSetDevice(m->device));
    HIP_TRY(wait_stream(m->stream));
    return MMDX_OK;
}


// ---- VMD morph motion: device-side evaluation ----------------------------------------------------
// the tables of a motion -> the device it is about to run on (once per device)
static mmdx_status morph_to_device(MorphMotionDevice &d, const MorphMotionHost &h, int device) {
    if (d.device == device) return MMDX_OK;
    if (graph_pinned(&d.pin)) return fail(MMDX_ERR_INVALID_ARGUMENT, "this motion's device tables are held by a recorded graph: destroy the graph before moving it to another device");
    for (DevBuf *b : d.all()) b->release();
    HIP_TRY(d.key_off.upload(h.key_off, size_t(h.nm) + 1));
    HIP_TRY(d.frames.upload(h.frames, h.nkeys));
    HIP_TRY(d.weights.upload(h.weights, h.nkeys));
    d.device = device;
    return MMDX_OK;
}

// mmdx_morph_motion_eval / _eval_time: frames (uint32_t) or, with `time`, seconds (double).  The sequence of bone_motion_eval
// (rig_api.cpp), with this call's own two refusals of a recording, each in its own words and place: host operands ahead of
// resolve_stream, a motion that never ran on the device behind it.
static mmdx_status morph_motion_eval(mmdx_morph_motion_t mm, mmdx_model_t model, uint32_t n_instances, const void *clock, bool time,
                                     uint32_t flags, float *out_weights) {
    if (!mm || !clock || !out_weights || !n_instances)
        return fail(MMDX_ERR_INVALID_ARGUMENT, "NULL argument or n_instances == 0");
    if (mmdx_status r = refuse_recording(flags, MMDX_FRAMES_ON_DEVICE | MMDX_OUT_ON_DEVICE, 0, {},
                                         "while a graph is being recorded every operand must be in device memory"))
        return r;
    int device;
    hipStream_t st;
    if (mmdx_status r = resolve_stream(model, &device, &st)) return r;
    MorphMotionDevice *&dev = morph_motion_device(mm);
    if (!dev && !(dev = new (std::nothrow) MorphMotionDevice)) return fail(MMDX_ERR_OUT_OF_MEMORY, "host allocation failed");
    MorphMotionDevice &d = *dev;
    if (mmdx_status r = refuse_recording(0, 0, device, {d.device},
                                         "first use of this motion on the device: run the sequence once before recording it"))
        return r;
    const MorphMotionHost h = morph_motion_host(mm);
    if (mmdx_status r = morph_to_device(d, h, device)) return r;
    graph_note_handle(model, &d.pin);
    MorphTrackParams t;
    t.key_off = static_cast<const uint32_t *>(d.key_off.ptr);
    t.key_frames = static_cast<const uint32_t *>(d.frames.ptr);
    t.key_weights = static_cast<const float *>(d.weights.ptr);
    t.nm = h.nm; t.ni = n_instances;
    t.frames = nullptr; t.times = nullptr;
    if (mmdx_status r = clock_in(d.frames_in, "morph motion frame scratch", clock, time, n_instances, flags, st, &t.frames, &t.times)) return r;
    OutRoute o;
    if (mmdx_status r = route_out(flags, out_weights, size_t(n_instances) * h.nm * 4, d.out, &o, "morph motion output scratch")) return r;
    t.out = o.dev;
    HIP_TRY(launch_morph_track_eval(t, st));
    return finish(flags, !(flags & MMDX_FRAMES_ON_DEVICE), st, o);
}

mmdx_status mmdx_morph_motion_eval(mmdx_morph_motion_t mm, mmdx_model_t model, uint32_t n_instances,
                                   const uint32_t *frames, uint32_t flags, float *out_weights) {
    return morph_motion_eval(mm, model, n_instances, frames, false, flags, out_weights);
}

mmdx_status mmdx_morph_motion_eval_time(mmdx_morph_motion_t mm, mmdx_model_t model, uint32_t n_instances,
                                        const double *times, uint32_t flags, float *out_weights) {
    if (!mm || !times || !out_weights || !n_instances)
        return fail(MMDX_ERR_INVALID_ARGUMENT, "NULL argument or n_instances == 0");
    if (mmdx_status r = check_time_args(times, n_instances, flags, MMDX_TIMES_ON_DEVICE | MMDX_OUT_ON_DEVICE)) return r;
    return morph_motion_eval(mm, model, n_instances, times, true, flags, out_weights);
}

mmdx_status mmdx_graph_begin(mmdx_model_t m) {
    if (!m || m->device < 0) return fail(MMDX_ERR_INVALID_ARGUMENT, "model is NULL or host-only");
    if (m->capturing) return fail(MMDX_ERR_INVALID_ARGUMENT, "this model is already recording a graph");
    if (m->profile) return fail(MMDX_ERR_INVALID_ARGUMENT, "mmdx_profile_enable and graph recording exclude each other");
    HIP_TRY(hipSetDevice(m->device));
    if (tl_recording_depth > 0) {
        // a second recording on a thread that is already recording: drain this model's stream by polling (a blocking wait is one
        // of the calls a recording thread should not make)
        hipError_t q;
        while ((q = hipStreamQuery(m->stream)) == hipErrorNotReady) std::this_thread::yield();
        HIP_TRY(q);
    } else {
        HIP_TRY(hipStreamSynchronize(m->stream));
    }
    HIP_TRY(hipStreamBeginCapture(m->stream, hipStreamCaptureModeThreadLocal));
    m->capturing = true;
    m->capture_thread = std::this_thread::get_id();
    m->rec_poisoned = false;
    {
        std::lock_guard<std::mutex> lk(g_graph_mu);
        m->rec_pins.assign(1, &m->pin);
        m->pin.recorders.push_back(m);
    }
    ++tl_recording_depth;
    return MMDX_OK;
}

mmdx_status mmdx_graph_end(mmdx_model_t m, mmdx_graph_t *out) {
    if (!m || !out) return fail(MMDX_ERR_INVALID_ARGUMENT, "NULL argument");
    *out = nullptr;
    if (!m->capturing) return fail(MMDX_ERR_INVALID_ARGUMENT, "mmdx_graph_end without mmdx_graph_begin");
    // thread-local capture mode: the runtime wants the end on the thread that began, and the per-thread recording
    // state lives there -- refuse before anything is touched, so that the right thread can still end it
    if (m->capture_thread != std::this_thread::get_id())
        return fail(MMDX_ERR_INVALID_ARGUMENT, "mmdx_graph_end must be called on the thread that called mmdx_graph_begin");
    m->capturing = false;
    --tl_recording_depth;
    std::vector<GraphPin *> used;
    bool poisoned;
    {   // the recording is over either way: its handles no longer count this model as a recorder
        std::lock_guard<std::mutex> lk(g_graph_mu);
        used.swap(m->rec_pins);
        for (GraphPin *p : used) p->recorders.erase(std::remove(p->recorders.begin(), p->recorders.end(), m), p->recorders.end());
        poisoned = m->rec_poisoned;
    }
    hipGraph_t g = nullptr;
    hipError_t e = hipStreamEndCapture(m->stream, &g);
    if (tl_recording_depth == 0) {                      // handles destroyed while this thread was recording, and their blocks
        std::vector<mmdx_model_s *> models;
        models.swap(tl_deferred_models);
        for (mmdx_model_s *dm : models) {
            if (dm->device >= 0) {
                (void)hipSetDevice(dm->device);
                (void)hipStreamSynchronize(dm->stream);
            }
            free_model(dm);
        }
        for (void *p : tl_deferred_free) (void)hipFree(p);
        tl_deferred_free.clear();
        (void)hipSetDevice(m->device);
    }
    if (poisoned) {
        if (g) (void)hipGraphDestroy(g);
        (void)hipGetLastError();
        return fail(MMDX_ERR_INVALID_ARGUMENT, "a skeleton or motion used by this recording was destroyed before mmdx_graph_end: "
                                               "the recording holds freed device addresses and is discarded");
    }
    if (e != hipSuccess || !g) return hip_fail(e != hipSuccess ? e : hipErrorUnknown, "hipStreamEndCapture (a recorded call failed?)");
    hipGraphExec_t exec = nullptr;
    e = hipGraphInstantiate(&exec, g, nullptr, nullptr, 0);
    (void)hipGraphDestroy(g);
    if (e != hipSuccess) return hip_fail(e, "hipGraphInstantiate");
    mmdx_graph_s *gr = new (std::nothrow) mmdx_graph_s;
    if (!gr) { (void)hipGraphExecDestroy(exec); return fail(MMDX_ERR_OUT_OF_MEMORY, "host allocation failed"); }
    gr->exec = exec; gr->stream = m->stream; gr->device = m->device;
    {   // pin every handle whose buffers the recorded calls referred to
        std::lock_guard<std::mutex> lk(g_graph_mu);
        gr->pins = used;
        for (GraphPin *p : gr->pins) {
            p->graphs.push_back(gr);
            p->pins.fetch_add(1, std::memory_order_acq_rel);
        }
    }
    *out = gr;
    return MMDX_OK;
}

mmdx_status mmdx_graph_launch(mmdx_graph_t g) {
    if (!g) return fail(MMDX_ERR_INVALID_ARGUMENT, "graph is NULL");
    if (!g->valid.load(std::memory_order_acquire))
        return fail(MMDX_ERR_INVALID_ARGUMENT, "a model, skeleton or motion this graph was recorded from has been destroyed: "
                                               "the graph holds freed device addresses and cannot be replayed");
    {   // a replay may recompute a model's morphed positions from rates the host never saw: its host-side record of them is void
        std::lock_guard<std::mutex> lk(g_graph_mu);
        for (GraphPin *p : g->pins) p->replayed.store(true, std::memory_order_release);
    }
    HIP_TRY(hipSetDevice(g->device));
    HIP_TRY(hipGraphLaunch(static_cast<hipGraphExec_t>(g->exec), static_cast<hipStream_t>(g->stream)));
    return MMDX_OK;
}

void mmdx_graph_destroy(mmdx_graph_t g) {
    if (!g) return;
    {
        std::lock_guard<std::mutex> lk(g_graph_mu);
        for (GraphPin *p : g->pins) {
            p->graphs.erase(std::remove(p->graphs.begin(), p->graphs.end(), g), p->graphs.end());
            p->pins.fetch_sub(1, std::memory_order_acq_rel);
        }
        g->pins.clear();
    }
    (void)hipSetDevice(g->device);
    (void)hipGraphExecDestroy(static_cast<hipGraphExec_t>(g->exec));
    delete g;
}

mmdx_status mmdx_device_malloc(void **ptr, size_t bytes) {
    if (!ptr) return fail(MMDX_ERR_INVALID_ARGUMENT, "ptr is NULL");
    HIP_TRY(hipSetDevice(current_device()));
    HIP_TRY(hipMalloc(ptr, bytes ? bytes : 16));
    return MMDX_OK;
}

mmdx_status mmdx_host_malloc(void **ptr, size_t bytes) {
    if (!ptr) return fail(MMDX_ERR_INVALID_ARGUMENT, "ptr is NULL");
    HIP_TRY(hipSetDevice(current_device()));
    HIP_TRY(hipHostMalloc(ptr, bytes ? bytes : 16, hipHostMallocDefault));
    return MMDX_OK;
}

mmdx_status mmdx_host_free(void *ptr) {
    if (ptr) HIP_TRY(hipHostFree(ptr));
    return MMDX_OK;
}

mmdx_status mmdx_device_free(void *ptr) {
    if (ptr) HIP_TRY(hipFree(ptr));
    return MMDX_OK;
}

mmdx_status mmdx_memcpy_h2d(void *dst, const void *src, size_t bytes) {
    HIP_TRY(hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice));
    return MMDX_OK;
}

mmdx_status mmdx_memcpy_d2h(void *dst, const void *src, size_t bytes) {
    HIP_TRY(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
    return MMDX_OK;
}

mmdx_status mmdx_device_memset(void *dst, int value, size_t bytes) {
    // hipMemset of device memory is asynchronous to the host and runs on the null stream, which the models'
    // non-blocking streams do not wait for: complete it here, so that whatever the caller launches next (on any
    // stream) is ordered after it.
    HIP_TRY(hipMemset(dst, value, bytes));
    HIP_TRY(hipStreamSynchronize(nullptr));
    return MMDX_OK;
}



mmdx_status mmdx_device_synchronize(void) {
    HIP_TRY(hipDeviceSynchronize());
    return MMDX_OK;
}




mmdx_status mmdx_model_output_pitch(mmdx_model_t m, int32_t out_layout, uint32_t *pitch) {
    if (!m || !pitch) return fail(MMDX_ERR_INVALID_ARGUMENT, "model / pitch is NULL");
    if (out_layout < MMDX_OUT_SOA || out_layout > MMDX_OUT_SOA_POS16) return fail(MMDX_ERR_INVALID_ARGUMENT, "unknown out_layout");
    if (m->plan.f16 != (out_layout == MMDX_OUT_SOA_POS16))
        return fail(MMDX_ERR_UNSUPPORTED, "MMDX_OUT_SOA_POS16 goes with MMDX_CREATE_F16_POSITIONS models (and only with them)");
    // Every instance of every array of the layout starts on a 64-byte boundary: 12-byte SoA rows need a multiple of 16 vertices,
    // the 6-byte f16 rows 32, 32-byte vertices 2.  (16-byte boundaries -- multiples of 4 / 8 / 1 -- already give the kernel its
    // 16-byte copy-out, but measured on the config-3 crowd at NV = 50 003 in one pair of arrays: 0.935 of dense NV = 50 000's rate
    // at a 16-byte pitch, 1.005 at a 64-byte one, 0.990 at 128; with write-through stores 0.755 against 0.941 --
    // profiles/pitch/pitch_ab.txt.  Stores of an instance that starts inside a 64-byte line split that line with its neighbour.)
    const uint64_t align = out_layout == MMDX_OUT_SOA ? 16u : (out_layout == MMDX_OUT_SOA_POS16 ? 32u : 2u);
    const uint64_t pv = (uint64_t(m->plan.nv) + align - 1) / align * align;
    if (pv > UINT32_MAX) return fail(MMDX_ERR_INVALID_ARGUMENT, "the aligned pitch does not fit in 32 bits");
    *pitch = uint32_t(pv);
    return MMDX_OK;
}

namespace {
// mmdx_crowd_output_alloc(_pitched): [n_instances][pitch] vertices, the probe replays the (pitched) store pattern
mmdx_status crowd_output_alloc(mmdx_model_t m, uint32_t n_instances, int32_t out_layout, uint32_t pitch, uint32_t max_tries,
                               void **out_a, void **out_b, mmdx_placement_info *info) {
    if (!m || !out_a || !out_b || !n_instances) return fail(MMDX_ERR_INVALID_ARGUMENT, "NULL argument or n_instances == 0");
    if (m->device < 0) return fail(MMDX_ERR_NO_DEVICE, "host-only model");
    if (info && info->struct_size != sizeof(mmdx_placement_info))
        return fail(MMDX_ERR_INVALID_ARGUMENT, "mmdx_placement_info.struct_size mismatch");
    uint32_t bpva, bpvb;
    switch (out_layout) {
    case MMDX_OUT_SOA: bpva = 12; bpvb = 12; break;
    case MMDX_OUT_VERTEX32: bpva = 32; bpvb = 0; break;
    case MMDX_OUT_SOA_POS16: bpva = 6; bpvb = 12; break;
    default: return fail(MMDX_ERR_INVALID_ARGUMENT, "unknown out_layout");
    }
    const uint32_t nv = m->plan.nv;
    if (pitch < nv) return fail(MMDX_ERR_INVALID_ARGUMENT, "pitch is smaller than the model's vertex count");
    if (uint64_t(n_instances) * pitch > uint64_t(SIZE_MAX) / 32)
        return fail(MMDX_ERR_INVALID_ARGUMENT, "n_instances * pitch overflows");
    *out_a = *out_b = nullptr;
    HIP_TRY(hipSetDevice(m->device));
    const size_t bytes_a = std::max<size_t>(size_t(n_instances) * pitch * bpva, 16);
    const size_t bytes_b = bpvb ? std::max<size_t>(size_t(n_instances) * pitch * bpvb, 16) : 0;
    // bytes the replay (and a crowd call) actually writes: NV vertices per instance, never the gap of a pitched layout
    const size_t written = size_t(n_instances) * nv * (bpva + bpvb);
    // the replay needs every instance's piece 16-byte aligned; otherwise (odd dense vertex counts) allocate without probing
    const bool can_probe = max_tries > 1 && nv && (size_t(pitch) * bpva) % 16 == 0 && (size_t(pitch) * bpvb) % 16 == 0;
    struct Cand { void *a = nullptr, *b = nullptr; float gbs = 0.f; };
    std::vector<Cand> parked;
    Cand best;
    float fill_gbs = 0.f;
    uint32_t tries = 0, slow_in_a_row = 0;
    mmdx_status st = MMDX_OK;
    auto release = [](Cand &c) { if (c.a) (void)hipFree(c.a); if (c.b) (void)hipFree(c.b); c.a = c.b = nullptr; };
    for (; tries < std::max(max_tries, 1u); ) {
        Cand c;
        hipError_t e = hipMalloc(&c.a, bytes_a);
        if (e == hipSuccess && bytes_b) e = hipMalloc(&c.b, bytes_b);
        if (e != hipSuccess) {
            release(c);
            (void)hipGetLastError();
            if (best.a) break;                       // out of memory while shopping: keep what we have
            st = hip_fail(e, "hipMalloc of the crowd output arrays");
            break;
        }
        ++tries;
        if (!can_probe) { best = c; break; }
        float ms = 0.f;
        if (fill_gbs == 0.f) {                       // the yardstick: a linear fill of array a
            hipEvent_t e0, e1;
            e = hipEventCreate(&e0);
            if (e == hipSuccess) e = hipEventCreate(&e1);
            if (e == hipSuccess) e = launch_fill(c.a, bytes_a & ~size_t(15), nullptr);
            if (e == hipSuccess) e = hipEventRecord(e0, nullptr);
            for (int i = 0; i < 5 && e == hipSuccess; ++i) e = launch_fill(c.a, bytes_a & ~size_t(15), nullptr);
            if (e == hipSuccess) e = hipEventRecord(e1, nullptr);
            if (e == hipSuccess) e = hipEventSynchronize(e1);
            if (e == hipSuccess) e = hipEventElapsedTime(&ms, e0, e1);
            (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
            if (e == hipSuccess && ms > 0.f) fill_gbs = float(double(bytes_a) * 5 / (ms * 1e-3) / 1e9);
        }
        if (e == hipSuccess) e = time_store_pattern(c.a, c.b, nv, n_instances, bpva, bpvb, 5, &ms, pitch);
        if (e != hipSuccess) { release(c); st = hip_fail(e, "probing a placement of the crowd output arrays"); break; }
        c.gbs = float(double(written) / (ms * 1e-3) / 1e9);
        if (launch_overrides().placement_log)
            std::fprintf(stderr, "mmdx placement try %u: a=%p b=%p store %.0f GB/s (fill %.0f)\n", tries, c.a, c.b, c.gbs, fill_gbs);
        // measured (tools/archive/probes/shop_probe.py): about one placement in seven is fast either way; freeing a rejected
        // candidate at once needs a few tries less on average than keeping it parked, and no extra memory.  But a process can
        // get STUCK that way -- freed blocks come straight back, 128 tries in a row in the same slow backing (seen once in the
        // round-2 profile runs: 0.279 instead of 0.227 ms per step) -- so after 8 slow tries in a row the rejected candidates
        // are kept until the end (up to 48 pairs, ~60 GB of the 288): every further try then draws fresh physical memory.
        if (c.gbs < 0.92f * fill_gbs) ++slow_in_a_row; else slow_in_a_row = 0;
        const bool park = launch_overrides().placement_park != 0 || (slow_in_a_row >= 8 && parked.size() < 48);
        if (c.gbs > best.gbs) {
            if (best.a) { if (park) parked.push_back(best); else release(best); }
            best = c;
        } else if (park) {
            parked.push_back(c);
        } else {
            release(c);
        }
        if (best.gbs >= 0.92f * fill_gbs) break;     // the fast mode sits at 0.96-0.99 of the fill rate, the slow ones at 0.72-0.8
    }
    const bool freed_any = tries > 1;
    for (Cand &c : parked) release(c);
    if (st != MMDX_OK) { release(best); return st; }
    // The driver wipes freed VRAM in the background (gigabytes per rejected try), which steals HBM bandwidth
    // from whatever runs next: replay the pattern on the chosen arrays until its rate is back where it was
    // measured, so the caller's first launches already see a quiet memory system (bounded: ~0.25 s).
    for (int i = 0; freed_any && can_probe && i < 150; ++i) {
        float ms = 0.f;
        if (time_store_pattern(best.a, best.b, nv, n_instances, bpva, bpvb, 5, &ms, pitch) != hipSuccess) break;
        if (double(written) / (ms * 1e-3) / 1e9 >= 0.98 * best.gbs) break;
    }
    HIP_TRY(hipDeviceSynchronize());
    *out_a = best.a;
    *out_b = best.b;
    if (info) {
        info->tries = tries;
        info->probed = can_probe ? 1u : 0u;
        info->store_GBs = best.gbs;
        info->fill_GBs = fill_gbs;
        // the probe's verdict, for the caller to pass on in mmdx_deform_args.flags (nothing is remembered here)
        info->store_flags = can_probe && fill_gbs > 0.f ? (best.gbs >= 0.92f * fill_gbs ? uint32_t(MMDX_OUT_STORES_CACHED)
                                                                                         : uint32_t(MMDX_OUT_STORES_WRITE_THROUGH))
                                                        : 0u;
    }
    return MMDX_OK;
}
}  // namespace

mmdx_status mmdx_crowd_output_alloc(mmdx_model_t m, uint32_t n_instances, int32_t out_layout, uint32_t max_tries,
                                    void **out_a, void **out_b, mmdx_placement_info *info) {
    return crowd_output_alloc(m, n_instances, out_layout, m ? m->plan.nv : 0u, max_tries, out_a, out_b, info);
}

mmdx_status mmdx_crowd_output_alloc_pitched(mmdx_model_t m, uint32_t n_instances, int32_t out_layout, uint32_t pitch,
                                            uint32_t max_tries, void **out_a, void **out_b, mmdx_placement_info *info) {
    return crowd_output_alloc(m, n_instances, out_layout, pitch, max_tries, out_a, out_b, info);
}

}  // extern "C"

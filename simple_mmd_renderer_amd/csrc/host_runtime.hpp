// host_runtime.hpp -- the host plumbing every C-ABI file (api.cpp, rig_api.cpp, anim_api.cpp, place_api.cpp, pbounds_api.cpp,
// cull_api.cpp, row_blend_api.cpp, bench_api.cpp) takes from one place: the runtime services api.cpp defines, HIP_TRY, the device buffer, and the
// named steps a call is built from -- what a recording refuses, the preamble of a call on a model, the instance-list checks and
// stager, the host round trip (stage_in / clock_in / route_out / finish).  No device code, no launch declarations.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <initializer_list>
#include <string>
#include <vector>

#include "../../include/mmdx.h"
#include "error.hpp"
#include "graph_pin.hpp"

namespace mmdx {

// ---- runtime services (api.cpp) --------------------------------------------------------------------------------------------------
// HIP error -> status + message (also clears the runtime's sticky error)
mmdx_status hip_fail(hipError_t e, const char *what);

#define HIP_TRY(expr)                                          \
    do {                                                       \
        hipError_t e_ = (expr);                                \
        if (e_ != hipSuccess) return hip_fail(e_, #expr);      \
    } while (0)

// the device and stream a motion / rig / animator call runs on -- the model's own when a (device) model is given, so that the
// deform call that follows is ordered after it; else the selected device's default stream.  Refuses a model whose stream records
// on another thread; fails with MMDX_ERR_NO_DEVICE when there is no GPU (no CPU fallback).  Selects the device.
mmdx_status resolve_stream(mmdx_model_t model, int *device, hipStream_t *stream);
// the same for a call ON a model handle, at the end of its argument checks: refuses a MMDX_CREATE_HOST_ONLY model, a model whose
// stream records on another thread and -- while the calling thread records -- `flags` without every *_ON_DEVICE bit of `need`
// (`text`: the call's own wording; need == 0: the call has no host operand to refuse).  Selects the model's device.
mmdx_status model_call_begin(mmdx_model_t m, uint32_t flags, uint32_t need, const char *text);
// the calling thread is between mmdx_graph_begin and mmdx_graph_end (nothing may allocate, copy from the host or wait)
bool graph_recording();
// hipFree, or -- while this thread records a graph, when the runtime refuses frees -- parked until mmdx_graph_end
void device_free_or_defer(void *ptr);
// host-visible completion of the work queued on `stream` (polls before it blocks: api.cpp)
hipError_t wait_stream(hipStream_t stream);

// ---- the device buffer -----------------------------------------------------------------------------------------------------------
// One allocation a handle owns and grows on demand.  It never grows while the thread records a graph and never while a recorded
// graph holds its address (`pin`: the owning handle's); hip_fail turns both refusals into a clear message.
// `floor`: the smallest allocation.  The 16-byte floor is a property of the buffer, not of the call: the handles of rig_api.cpp
// and a morph motion's output scratch set 16, so their kernels never see a null pointer, and ensure(0) on them allocates (and so
// refuses under a recording or a pin); a model's scratch keeps 0, where ensure(0) on an empty buffer succeeds and leaves the
// pointer null.  Both are what these buffers did as two types.  upload() floors at 16 for every buffer: a table pointer is never null.
struct DevBuf {
    void *ptr = nullptr;
    size_t bytes = 0;
    const GraphPin *pin = nullptr;
    size_t floor = 0;
    hipError_t ensure(size_t need) {
        need = std::max(need, floor);
        if (need <= bytes) return hipSuccess;
        if (graph_recording()) return hipErrorStreamCaptureUnsupported;   // run the sequence once un-captured first
        if (graph_pinned(pin)) return hipErrorIllegalState;
        release();
        hipError_t e = hipMalloc(&ptr, need);
        if (e == hipSuccess) bytes = need;
        return e;
    }
    template <typename T>
    hipError_t upload(const T *data, size_t n) {
        hipError_t e = ensure(std::max<size_t>(n * sizeof(T), 16));
        if (e != hipSuccess || !n) return e;
        return hipMemcpy(ptr, data, n * sizeof(T), hipMemcpyHostToDevice);
    }
    template <typename T>
    hipError_t upload(const std::vector<T> &v) { return upload(v.data(), v.size()); }
    void release() {
        device_free_or_defer(ptr);
        ptr = nullptr; bytes = 0;
    }
};

// ---- what a recording cannot hold ------------------------------------------------------------------------------------------------
// While a graph is being recorded a call may neither copy from the host nor allocate: `flags` must hold every *_ON_DEVICE bit in
// `need`, and the static tables of every handle must be on `device` already (`ran_on`: the handles' device fields).
inline mmdx_status refuse_recording(uint32_t flags, uint32_t need, int device, std::initializer_list<int> ran_on, const char *text) {
    if (!graph_recording()) return MMDX_OK;
    bool recordable = (flags & need) == need;
    for (int d : ran_on) recordable = recordable && d == device;
    return recordable ? MMDX_OK : fail(MMDX_ERR_INVALID_ARGUMENT, text);
}

// ---- the instance list of a select call (mmdx_instance_select), decided without the device ---------------------------------------
// Three cuts, always in this order; an entry point may put checks of its own between them (mmdx_deform_batched_select does, twice).
// 1. the header
inline mmdx_status list_header_check(const mmdx_instance_select *sel) {
    if (sel->struct_size != sizeof(mmdx_instance_select))
        return fail(MMDX_ERR_INVALID_ARGUMENT, "mmdx_instance_select.struct_size mismatch");
    if (sel->flags & ~uint32_t(MMDX_SELECT_ON_DEVICE))
        return fail(MMDX_ERR_INVALID_ARGUMENT, "unknown bits in mmdx_instance_select.flags");
    if (sel->reserved0 != 0) return fail(MMDX_ERR_INVALID_ARGUMENT, "mmdx_instance_select.reserved0 must be 0");
    if (sel->n_ids && !sel->ids) return fail(MMDX_ERR_INVALID_ARGUMENT, "mmdx_instance_select.ids is NULL");
    return MMDX_OK;
}
// 2. where the list lives: a device list must be aligned, a host list cannot be recorded.  `recording` is the caller's to say:
//    the deform call asks whether ITS MODEL's stream records (m->capturing: it answers ahead of its other-thread refusal), the rig
//    calls, which may have no model, whether the CALLING THREAD records (graph_recording()).
inline mmdx_status list_placement_check(const mmdx_instance_select *sel, bool recording) {
    if (sel->flags & MMDX_SELECT_ON_DEVICE) {
        if ((reinterpret_cast<uintptr_t>(sel->ids) | reinterpret_cast<uintptr_t>(sel->count)) & 3)
            return fail(MMDX_ERR_INVALID_ARGUMENT, "device ids / count of mmdx_instance_select must be 4-byte aligned");
        return MMDX_OK;
    }
    if (recording)
        return fail(MMDX_ERR_INVALID_ARGUMENT, "while a graph is being recorded the instance list must be in device memory "
                                               "(MMDX_SELECT_ON_DEVICE)");
    return MMDX_OK;
}
// 3. a host list's ids: `live_host` = how many leading ids are in use (a device list: untouched)
inline mmdx_status host_list_check(const mmdx_instance_select *sel, uint32_t n_instances, uint32_t &live_host) {
    if (sel->flags & MMDX_SELECT_ON_DEVICE) return MMDX_OK;
    live_host = sel->count ? std::min(*sel->count, sel->n_ids) : sel->n_ids;
    for (uint32_t j = 0; j < live_host; ++j)
        if (sel->ids[j] >= n_instances)
            return fail(MMDX_ERR_INVALID_ARGUMENT, "mmdx_instance_select.ids[" + std::to_string(j) + "] = " +
                                                   std::to_string(sel->ids[j]) + " is not below n_instances");
    return MMDX_OK;
}

// A host list -> a handle's scratch in stream order, count word first: {live, ids[n_copy]}.  `image` is the source of the copy and
// stays alive in the handle until the copy has left it.  How many ids travel is the caller's: mmdx_deform_batched_select sends the
// list's whole capacity, the rig calls the `live` prefix.
inline mmdx_status stage_list(DevBuf &scratch, std::vector<uint32_t> &image, const uint32_t *ids, uint32_t n_copy, uint32_t live,
                              hipStream_t st, const uint32_t **dev_count, const uint32_t **dev_ids) {
    HIP_TRY(scratch.ensure((size_t(n_copy) + 1) * 4));
    image.resize(size_t(n_copy) + 1);
    image[0] = live;
    std::copy(ids, ids + n_copy, image.begin() + 1);
    HIP_TRY(hipMemcpyAsync(scratch.ptr, image.data(), image.size() * 4, hipMemcpyHostToDevice, st));
    *dev_count = static_cast<const uint32_t *>(scratch.ptr);
    *dev_ids = *dev_count + 1;
    return MMDX_OK;
}

// ---- the host round trip: host operands in through handle-owned scratch, results out, the wait -----------------------------------
// one host operand -> `scratch`, in stream order; the kernel reads scratch.ptr
inline mmdx_status stage_in(DevBuf &scratch, const void *src, size_t bytes, hipStream_t st) {
    HIP_TRY(scratch.ensure(bytes));
    if (bytes) HIP_TRY(hipMemcpyAsync(scratch.ptr, src, bytes, hipMemcpyHostToDevice, st));
    return MMDX_OK;
}

// the instant of every instance -> the clock fields of a parameter block: frame numbers (uint32_t) in `*frames` or, with `time`,
// seconds (double) in `*times`.  A host clock goes through `scratch`, sized 8 bytes per instance whenever it grows (room for
// either); `what` names that scratch in a refusal to grow.
inline mmdx_status clock_in(DevBuf &scratch, const char *what, const void *clock, bool time, uint32_t n_instances, uint32_t flags,
                            hipStream_t st, const uint32_t **frames, const double **times) {
    if (!(flags & MMDX_FRAMES_ON_DEVICE)) {                  // (MMDX_TIMES_ON_DEVICE is the same bit)
        const size_t bytes = size_t(n_instances) * (time ? 8 : 4);
        if (scratch.bytes < bytes)
            if (hipError_t e = scratch.ensure(size_t(n_instances) * 8)) return hip_fail(e, what);
        HIP_TRY(hipMemcpyAsync(scratch.ptr, clock, bytes, hipMemcpyHostToDevice, st));
        clock = scratch.ptr;
    }
    if (time) *times = static_cast<const double *>(clock);
    else *frames = static_cast<const uint32_t *>(clock);
    return MMDX_OK;
}

// where the results go
struct OutRoute {
    float *dev = nullptr;        // what the kernel writes: the caller's array (MMDX_OUT_ON_DEVICE) or a handle's scratch
    float *host = nullptr;       // the caller's host array `finish` copies the scratch to
    size_t bytes = 0;
};

inline mmdx_status route_out(uint32_t flags, float *caller_out, size_t bytes, DevBuf &scratch, OutRoute *o,
                             const char *what = "output scratch") {
    *o = OutRoute{caller_out, nullptr, bytes};
    if (flags & MMDX_OUT_ON_DEVICE) return MMDX_OK;
    if (hipError_t e = scratch.ensure(bytes)) return hip_fail(e, what);
    *o = OutRoute{static_cast<float *>(scratch.ptr), caller_out, bytes};
    return MMDX_OK;
}

// the end of a call: results bound for the host are copied out and waited for; results that stay on the device are waited for
// only when the call `borrowed` a host operand or a host list, which must be consumed before returning
inline mmdx_status finish(uint32_t flags, bool borrowed, hipStream_t st, const OutRoute &o) {
    if (!(flags & MMDX_OUT_ON_DEVICE)) {
        if (o.bytes) HIP_TRY(hipMemcpyAsync(o.host, o.dev, o.bytes, hipMemcpyDeviceToHost, st));
        HIP_TRY(wait_stream(st));
    } else if (borrowed) {
        HIP_TRY(wait_stream(st));
    }
    return MMDX_OK;
}

}  // namespace mmdx

// place_api.cpp -- mmdx_palette_place (include/mmdx.h): argument validation on the host, host operands through the model's scratch
// the way mmdx_skeleton_solve takes them, and the launch (place_kernels.hip) on the handle's stream.
#include <string>
#include <thread>

#include "api_internal.hpp"
#include "place_kernels.hpp"

using namespace mmdx;

namespace {

bool overlap(const void *a, size_t a_bytes, const void *b, size_t b_bytes) {
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
    return a0 < b0 + b_bytes && b0 < a0 + a_bytes;
}

}  // namespace

extern "C" mmdx_status mmdx_palette_place(mmdx_model_t m, const mmdx_place_args *a) {
    if (!m || !a) return fail(MMDX_ERR_INVALID_ARGUMENT, "model / args is NULL");
    if (a->struct_size != sizeof(mmdx_place_args)) return fail(MMDX_ERR_INVALID_ARGUMENT, "mmdx_place_args.struct_size mismatch");
    const uint32_t on_device = MMDX_PALETTE_ON_DEVICE | MMDX_PLACE_ON_DEVICE | MMDX_OUT_ON_DEVICE;
    if (a->flags & ~(on_device | uint32_t(MMDX_PLACE_MATRIX)))
        return fail(MMDX_ERR_INVALID_ARGUMENT, "unknown flag bits in mmdx_place_args.flags");
    if (a->reserved0 != 0) return fail(MMDX_ERR_INVALID_ARGUMENT, "mmdx_place_args.reserved0 must be 0");
    const uint32_t ni = a->n_instances, nb = m->plan.nb;
    if (!ni) return MMDX_OK;
    if (!a->palettes || !a->placements || !a->out_palettes)
        return fail(MMDX_ERR_INVALID_ARGUMENT, "palettes / placements / out_palettes is NULL");
    const bool matrix = (a->flags & MMDX_PLACE_MATRIX) != 0;
    const size_t pal_bytes = size_t(ni) * nb * 16 * sizeof(float);
    const size_t place_bytes = size_t(ni) * (matrix ? 16 : MMDX_POSE_FLOATS) * sizeof(float);
    if (a->palettes != a->out_palettes && overlap(a->palettes, pal_bytes, a->out_palettes, pal_bytes))
        return fail(MMDX_ERR_INVALID_ARGUMENT, "palettes and out_palettes overlap without being the same array (in place is "
                                               "out_palettes == palettes)");
    if (overlap(a->placements, place_bytes, a->out_palettes, pal_bytes))
        return fail(MMDX_ERR_INVALID_ARGUMENT, "placements overlaps out_palettes");
    uintptr_t align16 = 0;
    if (a->flags & MMDX_PALETTE_ON_DEVICE) align16 |= reinterpret_cast<uintptr_t>(a->palettes);
    if (a->flags & MMDX_OUT_ON_DEVICE) align16 |= reinterpret_cast<uintptr_t>(a->out_palettes);
    if (align16 & 15) return fail(MMDX_ERR_INVALID_ARGUMENT, "device palettes / out_palettes must be 16-byte aligned");
    if ((a->flags & MMDX_PLACE_ON_DEVICE) && (reinterpret_cast<uintptr_t>(a->placements) & 3))
        return fail(MMDX_ERR_INVALID_ARGUMENT, "device placements must be 4-byte aligned");
    if (ni > kPlaceMaxInstances || place_chunks(nb) > 65535u)
        return fail(MMDX_ERR_UNSUPPORTED, "mmdx_palette_place: more than 2^23 instances or 2^22 bones in one call");
    if (m->device < 0)
        return fail(MMDX_ERR_NO_DEVICE, "model was created with MMDX_CREATE_HOST_ONLY: nothing to run on (this engine has no CPU fallback)");
    if (m->capturing && m->capture_thread != std::this_thread::get_id())
        return fail(MMDX_ERR_INVALID_ARGUMENT, "this model's stream is recording a graph on another thread: recorded calls must come "
                                               "from the thread that called mmdx_graph_begin");
    if (graph_recording() && (a->flags & on_device) != on_device)
        return fail(MMDX_ERR_INVALID_ARGUMENT, "while a graph is being recorded palettes, placements and out_palettes must all be in "
                                               "device memory");
    HIP_TRY(hipSetDevice(m->device));
    if (!nb) return MMDX_OK;
    hipStream_t st = m->stream;
    PlaceLaunch p{a->palettes, a->placements, a->out_palettes, ni, nb, matrix};
    if (!(a->flags & MMDX_PALETTE_ON_DEVICE)) {
        HIP_TRY(m->place_in.ensure(pal_bytes));
        HIP_TRY(hipMemcpyAsync(m->place_in.ptr, a->palettes, pal_bytes, hipMemcpyHostToDevice, st));
        p.palettes = static_cast<const float *>(m->place_in.ptr);
    }
    if (!(a->flags & MMDX_PLACE_ON_DEVICE)) {
        HIP_TRY(m->place_w.ensure(place_bytes));
        HIP_TRY(hipMemcpyAsync(m->place_w.ptr, a->placements, place_bytes, hipMemcpyHostToDevice, st));
        p.placements = static_cast<const float *>(m->place_w.ptr);
    }
    if (!(a->flags & MMDX_OUT_ON_DEVICE)) {
        HIP_TRY(m->place_out.ensure(pal_bytes));
        p.out = static_cast<float *>(m->place_out.ptr);
    }
    HIP_TRY(launch_palette_place(p, st));
    if (!(a->flags & MMDX_OUT_ON_DEVICE)) {
        HIP_TRY(hipMemcpyAsync(a->out_palettes, p.out, pal_bytes, hipMemcpyDeviceToHost, st));
        HIP_TRY(wait_stream(st));
    } else if ((a->flags & on_device) != on_device) {
        HIP_TRY(wait_stream(st));   // borrowed host palettes / placements must be consumed before returning
    }
    return MMDX_OK;
}

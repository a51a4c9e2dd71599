// place_api.cpp -- mmdx_palette_place (include/mmdx.h): argument validation on the host, host operands through the model's scratch
// the way mmdx_skeleton_solve takes them, and the launch (place_kernels.hip) on the handle's stream.
#include <string>

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
    if (mmdx_status r = model_call_begin(m, a->flags, on_device, "while a graph is being recorded palettes, placements and "
                                                                 "out_palettes must all be in device memory"))
        return r;
    if (!nb) return MMDX_OK;
    hipStream_t st = m->stream;
    PlaceLaunch p{a->palettes, a->placements, a->out_palettes, ni, nb, matrix};
    if (!(a->flags & MMDX_PALETTE_ON_DEVICE)) {
        if (mmdx_status r = stage_in(m->place_in, a->palettes, pal_bytes, st)) return r;
        p.palettes = static_cast<const float *>(m->place_in.ptr);
    }
    if (!(a->flags & MMDX_PLACE_ON_DEVICE)) {
        if (mmdx_status r = stage_in(m->place_w, a->placements, place_bytes, st)) return r;
        p.placements = static_cast<const float *>(m->place_w.ptr);
    }
    OutRoute o;
    if (mmdx_status r = route_out(a->flags, a->out_palettes, pal_bytes, m->place_out, &o)) return r;
    p.out = o.dev;
    HIP_TRY(launch_palette_place(p, st));
    return finish(a->flags, (a->flags & on_device) != on_device, st, o);   // borrowed: host palettes / placements
}

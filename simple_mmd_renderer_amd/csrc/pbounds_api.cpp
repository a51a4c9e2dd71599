// pbounds_api.cpp -- mmdx_model_get_bone_boxes and mmdx_palette_bounds (include/mmdx.h): the table as the plan built it, argument
// validation on the host, host operands through the model's scratch the way mmdx_palette_place takes them, and the launch
// (pbounds_kernels.hip) on the handle's stream.
#include <cmath>
#include <cstring>
#include <string>

#include "api_internal.hpp"
#include "pbounds_kernels.hpp"

using namespace mmdx;

namespace {

bool overlap(const void *a, size_t a_bytes, const void *b, size_t b_bytes) {
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
    return a0 < b0 + b_bytes && b0 < a0 + a_bytes;
}

}  // namespace

// The table in the kernel's layout: three 16-byte groups per row, the bone in the fourth word of the first
std::vector<float> mmdx::bone_box_device_table(const Plan &p) {
    std::vector<float> t(p.box_bone.size() * kPBoundsRowFloats, 0.0f);
    for (size_t r = 0; r < p.box_bone.size(); ++r)
        for (int g = 0; g < 3; ++g) {
            std::memcpy(&t[r * kPBoundsRowFloats + 4 * g], &p.box[r * 9 + 3 * g], 3 * sizeof(float));
            if (g == 0) std::memcpy(&t[r * kPBoundsRowFloats + 3], &p.box_bone[r], 4);
        }
    return t;
}

extern "C" mmdx_status mmdx_model_get_bone_boxes(mmdx_model_t m, mmdx_bone_box_info *info, uint32_t *bones, float *boxes) {
    if (!m || !info) return fail(MMDX_ERR_INVALID_ARGUMENT, "model / info is NULL");
    if (info->struct_size != sizeof(mmdx_bone_box_info)) return fail(MMDX_ERR_INVALID_ARGUMENT, "mmdx_bone_box_info.struct_size mismatch");
    const Plan &p = m->plan;
    info->n_boxes = uint32_t(p.box_bone.size());
    info->n_nonconvex = p.n_nonconvex;
    info->max_vertex_entries = p.box_r_max;
    info->eps = p.box_eps;
    info->weight_sum_dev = p.box_wdev;
    info->reserved0[0] = info->reserved0[1] = 0;
    if (bones && !p.box_bone.empty()) std::memcpy(bones, p.box_bone.data(), p.box_bone.size() * sizeof(uint32_t));
    if (boxes && !p.box.empty()) std::memcpy(boxes, p.box.data(), p.box.size() * sizeof(float));
    return MMDX_OK;
}

extern "C" mmdx_status mmdx_palette_bounds(mmdx_model_t m, const mmdx_palette_bounds_args *a) {
    if (!m || !a) return fail(MMDX_ERR_INVALID_ARGUMENT, "model / args is NULL");
    if (a->struct_size != sizeof(mmdx_palette_bounds_args))
        return fail(MMDX_ERR_INVALID_ARGUMENT, "mmdx_palette_bounds_args.struct_size mismatch");
    const uint32_t on_device = MMDX_PALETTE_ON_DEVICE | MMDX_OUT_ON_DEVICE;
    if (a->flags & ~on_device) return fail(MMDX_ERR_INVALID_ARGUMENT, "unknown flag bits in mmdx_palette_bounds_args.flags");
    if (a->reserved0 != 0) return fail(MMDX_ERR_INVALID_ARGUMENT, "mmdx_palette_bounds_args.reserved0 must be 0");
    const uint32_t ni = a->n_instances, nb = m->plan.nb;
    if (!ni) return MMDX_OK;
    if (!a->palettes || !a->out_bounds) return fail(MMDX_ERR_INVALID_ARGUMENT, "palettes / out_bounds is NULL");
    if (!(std::isfinite(a->pos_scale) && a->pos_scale > 0.0f))
        return fail(MMDX_ERR_INVALID_ARGUMENT, "mmdx_palette_bounds_args.pos_scale must be finite and > 0");
    if (!(std::isfinite(a->morph_scale) && a->morph_scale >= 0.0f))
        return fail(MMDX_ERR_INVALID_ARGUMENT, "mmdx_palette_bounds_args.morph_scale must be finite and >= 0");
    const size_t pal_bytes = size_t(ni) * nb * 16 * sizeof(float), out_bytes = size_t(ni) * 6 * sizeof(float);
    if (overlap(a->palettes, pal_bytes, a->out_bounds, out_bytes)) return fail(MMDX_ERR_INVALID_ARGUMENT, "palettes overlaps out_bounds");
    if ((a->flags & MMDX_PALETTE_ON_DEVICE) && (reinterpret_cast<uintptr_t>(a->palettes) & 15))
        return fail(MMDX_ERR_INVALID_ARGUMENT, "device palettes must be 16-byte aligned");
    if ((a->flags & MMDX_OUT_ON_DEVICE) && (reinterpret_cast<uintptr_t>(a->out_bounds) & 3))
        return fail(MMDX_ERR_INVALID_ARGUMENT, "device out_bounds must be 4-byte aligned");
    if (ni > kPBoundsMaxInstances) return fail(MMDX_ERR_UNSUPPORTED, "mmdx_palette_bounds: more than 2^23 instances in one call");
    if (m->plan.n_nonconvex)
        return fail(MMDX_ERR_UNSUPPORTED, "mmdx_palette_bounds: " + std::to_string(m->plan.n_nonconvex) +
                                              " vertices of this model have a negative skin weight (n_nonconvex): a box of bone boxes "
                                              "does not contain them");
    if (mmdx_status r = model_call_begin(m, a->flags, on_device,
                                         "while a graph is being recorded palettes and out_bounds must both be in device memory"))
        return r;
    hipStream_t st = m->stream;
    PBoundsLaunch p{a->palettes, static_cast<const float *>(m->bone_boxes.ptr), a->out_bounds, ni, nb, uint32_t(m->plan.box_bone.size()),
                    m->plan.box_eps, a->morph_scale, a->pos_scale};
    if (!(a->flags & MMDX_PALETTE_ON_DEVICE)) {
        if (mmdx_status r = stage_in(m->pbounds_in, a->palettes, pal_bytes, st)) return r;
        p.palettes = static_cast<const float *>(m->pbounds_in.ptr);
    }
    OutRoute o;
    if (mmdx_status r = route_out(a->flags, a->out_bounds, out_bytes, m->pbounds_out, &o)) return r;
    p.out = o.dev;
    HIP_TRY(launch_palette_bounds(p, st));
    return finish(a->flags, (a->flags & on_device) != on_device, st, o);   // borrowed: host palettes
}

// row_blend_api.cpp -- mmdx_pose_blend / mmdx_rate_blend (include/mmdx.h): argument validation on the host, host operands through
// the model's scratch the way mmdx_palette_place takes them, the instance list of the select form, and the launch
// (row_blend_kernels.hip) on the handle's stream.
#include <cmath>
#include <string>

#include "api_internal.hpp"
#include "row_blend_kernels.hpp"

using namespace mmdx;

namespace {

bool overlap(const void *a, size_t a_bytes, const void *b, size_t b_bytes) {
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
    return a0 < b0 + b_bytes && b0 < a0 + a_bytes;
}

// `item_floats`: MMDX_POSE_FLOATS (poses) or 1 (rates); `name`: the entry point, for the messages
mmdx_status row_blend(mmdx_model_t m, const mmdx_row_blend_args *a, const mmdx_instance_select *sel, uint32_t item_floats,
                      const char *name) {
    if (!m || !a) return fail(MMDX_ERR_INVALID_ARGUMENT, "model / args is NULL");
    if (a->struct_size != sizeof(mmdx_row_blend_args))
        return fail(MMDX_ERR_INVALID_ARGUMENT, "mmdx_row_blend_args.struct_size mismatch");
    const uint32_t on_device = MMDX_BLEND_A_ON_DEVICE | MMDX_BLEND_B_ON_DEVICE | MMDX_BLEND_PARAMS_ON_DEVICE | MMDX_OUT_ON_DEVICE;
    if (a->flags & ~on_device) return fail(MMDX_ERR_INVALID_ARGUMENT, "unknown flag bits in mmdx_row_blend_args.flags");
    if (a->reserved0 != 0) return fail(MMDX_ERR_INVALID_ARGUMENT, "mmdx_row_blend_args.reserved0 must be 0");
    if (sel)
        if (mmdx_status r = list_header_check(sel)) return r;
    const uint32_t ni = a->n_instances, items = a->row_items;
    if (!ni || !items) return MMDX_OK;
    if (!a->a || !a->b || !a->weights || !a->out) return fail(MMDX_ERR_INVALID_ARGUMENT, "a / b / weights / out is NULL");
    const bool masked = a->mask_ids != nullptr;
    if (masked && a->n_masks && !a->masks) return fail(MMDX_ERR_INVALID_ARGUMENT, "n_masks > 0 but masks is NULL");
    const size_t row_bytes = size_t(ni) * items * item_floats * sizeof(float);
    const size_t mask_bytes = masked ? size_t(a->n_masks) * items * sizeof(float) : 0;
    if ((a->a != a->out && overlap(a->a, row_bytes, a->out, row_bytes)) || (a->b != a->out && overlap(a->b, row_bytes, a->out, row_bytes)))
        return fail(MMDX_ERR_INVALID_ARGUMENT, "a / b and out overlap without being the same array (in place is out == a or out == b)");
    if (overlap(a->a, row_bytes, a->b, row_bytes)) return fail(MMDX_ERR_INVALID_ARGUMENT, "a and b overlap");
    if (overlap(a->weights, size_t(ni) * 4, a->out, row_bytes) || (masked && overlap(a->mask_ids, size_t(ni) * 4, a->out, row_bytes)) ||
        (mask_bytes && overlap(a->masks, mask_bytes, a->out, row_bytes)))
        return fail(MMDX_ERR_INVALID_ARGUMENT, "weights / mask_ids / masks overlaps out");
    uintptr_t rows = 0, params = 0;
    if (a->flags & MMDX_BLEND_A_ON_DEVICE) rows |= reinterpret_cast<uintptr_t>(a->a);
    if (a->flags & MMDX_BLEND_B_ON_DEVICE) rows |= reinterpret_cast<uintptr_t>(a->b);
    if (a->flags & MMDX_OUT_ON_DEVICE) rows |= reinterpret_cast<uintptr_t>(a->out);
    if (rows & (item_floats == 1 ? 3 : 15))
        return fail(MMDX_ERR_INVALID_ARGUMENT, item_floats == 1 ? "device a / b / out of mmdx_rate_blend must be 4-byte aligned"
                                                                : "device a / b / out of mmdx_pose_blend must be 16-byte aligned");
    if (a->flags & MMDX_BLEND_PARAMS_ON_DEVICE) {
        params = reinterpret_cast<uintptr_t>(a->weights) | reinterpret_cast<uintptr_t>(a->mask_ids);
        if (mask_bytes) params |= reinterpret_cast<uintptr_t>(a->masks);
    }
    if (params & 3) return fail(MMDX_ERR_INVALID_ARGUMENT, "device weights / mask_ids / masks must be 4-byte aligned");
    if (ni > kRowBlendMaxCells || (sel && sel->n_ids > kRowBlendMaxCells) || row_blend_chunks(items) > 65535u)
        return fail(MMDX_ERR_UNSUPPORTED, std::string(name) + ": more than 2^23 instances or list positions, or 2^24 items in a row");
    uint32_t live_host = 0;
    if (sel) {
        if (mmdx_status r = list_placement_check(sel, m->capturing)) return r;
        const uint32_t need = MMDX_BLEND_A_ON_DEVICE | MMDX_BLEND_B_ON_DEVICE | MMDX_OUT_ON_DEVICE;
        if ((a->flags & need) != need)
            return fail(MMDX_ERR_INVALID_ARGUMENT, std::string(name) + " with a select list takes a, b and out in device memory only "
                                                   "(the staging copies of host rows move whole arrays)");
        if (mmdx_status r = host_list_check(sel, ni, live_host)) return r;
    }
    if (!(a->flags & MMDX_BLEND_PARAMS_ON_DEVICE)) {
        for (uint32_t i = 0; i < ni; ++i)
            if (std::isnan(a->weights[i]))
                return fail(MMDX_ERR_INVALID_ARGUMENT, "weights[" + std::to_string(i) + "] is NaN");
        if (masked)
            for (uint32_t i = 0; i < ni; ++i)
                if (a->mask_ids[i] >= a->n_masks && a->mask_ids[i] != MMDX_MASK_NONE)
                    return fail(MMDX_ERR_BAD_INDEX, "mask_ids[" + std::to_string(i) + "] = " + std::to_string(a->mask_ids[i]) +
                                                    " is neither below n_masks nor MMDX_MASK_NONE");
        for (size_t k = 0; k < mask_bytes / sizeof(float); ++k)
            if (std::isnan(a->masks[k])) return fail(MMDX_ERR_INVALID_ARGUMENT, "masks holds a NaN (value " + std::to_string(k) + ")");
    }
    if (mmdx_status r = model_call_begin(m, a->flags, on_device, "while a graph is being recorded a, b, weights, mask_ids, masks and "
                                                                 "out must all be in device memory"))
        return r;
    hipStream_t st = m->stream;
    RowBlendLaunch p{a->a, a->b, a->weights, a->mask_ids, a->masks, a->out, ni, items, masked ? a->n_masks : 0u};
    InstanceList list{nullptr, nullptr, ni};
    uint32_t cells = ni;
    if (sel) {
        list = InstanceList{sel->ids, sel->count, ni};
        cells = sel->n_ids;
        if (!(sel->flags & MMDX_SELECT_ON_DEVICE)) {
            cells = live_host;
            if (live_host)
                if (mmdx_status r = stage_list(m->blend_sel, m->blend_sel_host, sel->ids, live_host, live_host, st, &list.count, &list.ids))
                    return r;
        }
        if (!cells) return MMDX_OK;
    }
    if (!(a->flags & MMDX_BLEND_A_ON_DEVICE)) {
        if (mmdx_status r = stage_in(m->blend_a, a->a, row_bytes, st)) return r;
        p.a = static_cast<const float *>(m->blend_a.ptr);
    }
    if (!(a->flags & MMDX_BLEND_B_ON_DEVICE)) {
        if (mmdx_status r = stage_in(m->blend_b, a->b, row_bytes, st)) return r;
        p.b = static_cast<const float *>(m->blend_b.ptr);
    }
    if (!(a->flags & MMDX_BLEND_PARAMS_ON_DEVICE)) {           // weights, mask ids, masks laid end to end
        const size_t w_bytes = size_t(ni) * 4, id_bytes = masked ? w_bytes : 0;
        HIP_TRY(m->blend_p.ensure(w_bytes + id_bytes + mask_bytes));
        char *base = static_cast<char *>(m->blend_p.ptr);
        HIP_TRY(hipMemcpyAsync(base, a->weights, w_bytes, hipMemcpyHostToDevice, st));
        p.weights = reinterpret_cast<const float *>(base);
        if (masked) {
            HIP_TRY(hipMemcpyAsync(base + w_bytes, a->mask_ids, id_bytes, hipMemcpyHostToDevice, st));
            p.mask_ids = reinterpret_cast<const uint32_t *>(base + w_bytes);
        }
        if (mask_bytes) {
            HIP_TRY(hipMemcpyAsync(base + w_bytes + id_bytes, a->masks, mask_bytes, hipMemcpyHostToDevice, st));
            p.masks = reinterpret_cast<const float *>(base + w_bytes + id_bytes);
        }
    }
    OutRoute o;
    if (mmdx_status r = route_out(a->flags, a->out, row_bytes, m->blend_out, &o)) return r;
    p.out = o.dev;
    // in place in host memory: the staged copy of that operand is separate scratch, the kernel then copies the untouched items
    if (item_floats == 1) HIP_TRY(launch_rate_blend(p, sel ? &list : nullptr, cells, st));
    else HIP_TRY(launch_pose_blend(p, sel ? &list : nullptr, cells, st));
    const bool borrowed = (a->flags & on_device) != on_device || (sel && !(sel->flags & MMDX_SELECT_ON_DEVICE));
    return finish(a->flags, borrowed, st, o);
}

}  // namespace

extern "C" mmdx_status mmdx_pose_blend(mmdx_model_t m, const mmdx_row_blend_args *a, const mmdx_instance_select *sel) {
    return row_blend(m, a, sel, MMDX_POSE_FLOATS, "mmdx_pose_blend");
}

extern "C" mmdx_status mmdx_rate_blend(mmdx_model_t m, const mmdx_row_blend_args *a, const mmdx_instance_select *sel) {
    return row_blend(m, a, sel, 1, "mmdx_rate_blend");
}

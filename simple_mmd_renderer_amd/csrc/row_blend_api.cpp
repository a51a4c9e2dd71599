// row_blend_api.cpp -- mmdx_pose_blend / mmdx_rate_blend and mmdx_pose_add / mmdx_rate_add (include/mmdx.h): argument validation on
// the host, host operands through the model's scratch the way mmdx_palette_place takes them, the instance list of the select form,
// and the launch (row_blend_kernels.hip; pose_add_kernel: rig_kernels.hip) on the handle's stream.  The four calls share one body:
// the add calls are the blend calls plus the reference rows, and mmdx_row_add_args is mmdx_row_blend_args plus three fields.
#include <cmath>
#include <string>

#include "api_internal.hpp"
#include "rig_kernels.hpp"
#include "row_blend_kernels.hpp"

using namespace mmdx;

namespace {

bool overlap(const void *a, size_t a_bytes, const void *b, size_t b_bytes) {
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
    return a0 < b0 + b_bytes && b0 < a0 + a_bytes;
}

// which of the four calls: `item_floats` MMDX_POSE_FLOATS (poses) or 1 (rates); `name` / `args_name`: the entry point and its
// structure, for the messages; `add`: the reference fields of the structure are read
struct RowCall {
    uint32_t item_floats;
    bool add;
    const char *name, *args_name;
};

// `a`: the caller's structure (struct_size checked), or the blend's copied into the larger one with no reference
mmdx_status row_call(mmdx_model_t m, const mmdx_row_add_args *a, const mmdx_instance_select *sel, const RowCall &c) {
    const uint32_t item_floats = c.item_floats;
    const std::string name = c.name, args_name = c.args_name;
    const uint32_t on_device = MMDX_BLEND_A_ON_DEVICE | MMDX_BLEND_B_ON_DEVICE | MMDX_BLEND_PARAMS_ON_DEVICE | MMDX_OUT_ON_DEVICE;
    if (a->flags & ~on_device) return fail(MMDX_ERR_INVALID_ARGUMENT, "unknown flag bits in " + args_name + ".flags");
    if (a->reserved0 != 0) return fail(MMDX_ERR_INVALID_ARGUMENT, args_name + ".reserved0 must be 0");
    if (a->reserved1 != 0) return fail(MMDX_ERR_INVALID_ARGUMENT, args_name + ".reserved1 must be 0");
    if (sel)
        if (mmdx_status r = list_header_check(sel)) return r;
    const uint32_t ni = a->n_instances, items = a->row_items;
    if (!ni || !items) return MMDX_OK;
    if (!a->a || !a->b || !a->weights || !a->out) return fail(MMDX_ERR_INVALID_ARGUMENT, "a / b / weights / out is NULL");
    const bool masked = a->mask_ids != nullptr, referenced = c.add && a->ref_ids != nullptr;
    if (masked && a->n_masks && !a->masks) return fail(MMDX_ERR_INVALID_ARGUMENT, "n_masks > 0 but masks is NULL");
    if (referenced && a->n_refs && !a->refs) return fail(MMDX_ERR_INVALID_ARGUMENT, "n_refs > 0 but refs is NULL");
    const size_t row_bytes = size_t(ni) * items * item_floats * sizeof(float);
    const size_t mask_bytes = masked ? size_t(a->n_masks) * items * sizeof(float) : 0;
    const size_t ref_bytes = referenced ? size_t(a->n_refs) * items * item_floats * sizeof(float) : 0;
    if ((a->a != a->out && overlap(a->a, row_bytes, a->out, row_bytes)) || (a->b != a->out && overlap(a->b, row_bytes, a->out, row_bytes)))
        return fail(MMDX_ERR_INVALID_ARGUMENT, "a / b and out overlap without being the same array (in place is out == a or out == b)");
    if (overlap(a->a, row_bytes, a->b, row_bytes)) return fail(MMDX_ERR_INVALID_ARGUMENT, "a and b overlap");
    if (overlap(a->weights, size_t(ni) * 4, a->out, row_bytes) || (masked && overlap(a->mask_ids, size_t(ni) * 4, a->out, row_bytes)) ||
        (mask_bytes && overlap(a->masks, mask_bytes, a->out, row_bytes)))
        return fail(MMDX_ERR_INVALID_ARGUMENT, "weights / mask_ids / masks overlaps out");
    if ((referenced && overlap(a->ref_ids, size_t(ni) * 4, a->out, row_bytes)) || (ref_bytes && overlap(a->refs, ref_bytes, a->out, row_bytes)))
        return fail(MMDX_ERR_INVALID_ARGUMENT, "ref_ids / refs overlaps out");
    uintptr_t rows = 0, params = 0;
    if (a->flags & MMDX_BLEND_A_ON_DEVICE) rows |= reinterpret_cast<uintptr_t>(a->a);
    if (a->flags & MMDX_BLEND_B_ON_DEVICE) rows |= reinterpret_cast<uintptr_t>(a->b);
    if (a->flags & MMDX_OUT_ON_DEVICE) rows |= reinterpret_cast<uintptr_t>(a->out);
    if (rows & (item_floats == 1 ? 3 : 15))
        return fail(MMDX_ERR_INVALID_ARGUMENT, "device a / b / out of " + name + (item_floats == 1 ? " must be 4-byte aligned" : " must be 16-byte aligned"));
    if (a->flags & MMDX_BLEND_PARAMS_ON_DEVICE) {
        params = reinterpret_cast<uintptr_t>(a->weights) | reinterpret_cast<uintptr_t>(a->mask_ids);
        if (mask_bytes) params |= reinterpret_cast<uintptr_t>(a->masks);
    }
    if (params & 3) return fail(MMDX_ERR_INVALID_ARGUMENT, "device weights / mask_ids / masks must be 4-byte aligned");
    if ((a->flags & MMDX_BLEND_PARAMS_ON_DEVICE) && referenced) {
        if (reinterpret_cast<uintptr_t>(a->ref_ids) & 3) return fail(MMDX_ERR_INVALID_ARGUMENT, "device ref_ids must be 4-byte aligned");
        if (ref_bytes && (reinterpret_cast<uintptr_t>(a->refs) & (item_floats == 1 ? 3 : 15)))
            return fail(MMDX_ERR_INVALID_ARGUMENT, "device refs of " + name + (item_floats == 1 ? " must be 4-byte aligned" : " must be 16-byte aligned"));
    }
    if (ni > kRowBlendMaxCells || (sel && sel->n_ids > kRowBlendMaxCells) || row_blend_chunks(items) > 65535u)
        return fail(MMDX_ERR_UNSUPPORTED, name + ": more than 2^23 instances or list positions, or 2^24 items in a row");
    uint32_t live_host = 0;
    if (sel) {
        if (mmdx_status r = list_placement_check(sel, m->capturing)) return r;
        const uint32_t need = MMDX_BLEND_A_ON_DEVICE | MMDX_BLEND_B_ON_DEVICE | MMDX_OUT_ON_DEVICE;
        if ((a->flags & need) != need)
            return fail(MMDX_ERR_INVALID_ARGUMENT, name + " with a select list takes a, b and out in device memory only "
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
        if (referenced)
            for (uint32_t i = 0; i < ni; ++i)
                if (a->ref_ids[i] >= a->n_refs && a->ref_ids[i] != MMDX_REF_NONE)
                    return fail(MMDX_ERR_BAD_INDEX, "ref_ids[" + std::to_string(i) + "] = " + std::to_string(a->ref_ids[i]) +
                                                    " is neither below n_refs nor MMDX_REF_NONE");
    }
    if (mmdx_status r = model_call_begin(m, a->flags, on_device,
                                         c.add ? "while a graph is being recorded a, b, weights, mask_ids, masks, ref_ids, refs and out "
                                                 "must all be in device memory"
                                               : "while a graph is being recorded a, b, weights, mask_ids, masks and "
                                                 "out must all be in device memory"))
        return r;
    hipStream_t st = m->stream;
    RowBlendLaunch p{a->a, a->b, a->weights, a->mask_ids, a->masks, a->out, ni, items, masked ? a->n_masks : 0u};
    RowAddLaunch q{p, referenced ? a->ref_ids : nullptr, referenced ? a->refs : nullptr, referenced ? a->n_refs : 0u};
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
    if (!(a->flags & MMDX_BLEND_PARAMS_ON_DEVICE)) {           // weights, mask ids, masks, ref ids laid end to end; refs 16-byte aligned
        const size_t w_bytes = size_t(ni) * 4, id_bytes = masked ? w_bytes : 0, rid_bytes = referenced ? w_bytes : 0;
        const size_t refs_at = (w_bytes + id_bytes + mask_bytes + rid_bytes + 15) / 16 * 16;
        HIP_TRY(m->blend_p.ensure(refs_at + ref_bytes));
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
        if (referenced) {
            HIP_TRY(hipMemcpyAsync(base + w_bytes + id_bytes + mask_bytes, a->ref_ids, rid_bytes, hipMemcpyHostToDevice, st));
            q.ref_ids = reinterpret_cast<const uint32_t *>(base + w_bytes + id_bytes + mask_bytes);
        }
        if (ref_bytes) {
            HIP_TRY(hipMemcpyAsync(base + refs_at, a->refs, ref_bytes, hipMemcpyHostToDevice, st));
            q.refs = reinterpret_cast<const float *>(base + refs_at);
        }
    }
    OutRoute o;
    if (mmdx_status r = route_out(a->flags, a->out, row_bytes, m->blend_out, &o)) return r;
    p.out = o.dev;
    q.rows = p;
    // in place in host memory: the staged copy of that operand is separate scratch, the kernel then copies the untouched items
    const InstanceList *lp = sel ? &list : nullptr;
    if (c.add) HIP_TRY(item_floats == 1 ? launch_rate_add(q, lp, cells, st) : launch_pose_add(q, lp, cells, st));
    else HIP_TRY(item_floats == 1 ? launch_rate_blend(p, lp, cells, st) : launch_pose_blend(p, lp, cells, st));
    const bool borrowed = (a->flags & on_device) != on_device || (sel && !(sel->flags & MMDX_SELECT_ON_DEVICE));
    return finish(a->flags, borrowed, st, o);
}

mmdx_status row_blend(mmdx_model_t m, const mmdx_row_blend_args *a, const mmdx_instance_select *sel, uint32_t item_floats,
                      const char *name) {
    if (!m || !a) return fail(MMDX_ERR_INVALID_ARGUMENT, "model / args is NULL");
    if (a->struct_size != sizeof(mmdx_row_blend_args))
        return fail(MMDX_ERR_INVALID_ARGUMENT, "mmdx_row_blend_args.struct_size mismatch");
    mmdx_row_add_args x{};
    x.flags = a->flags; x.n_instances = a->n_instances; x.row_items = a->row_items;
    x.a = a->a; x.b = a->b; x.weights = a->weights; x.mask_ids = a->mask_ids; x.masks = a->masks;
    x.n_masks = a->n_masks; x.reserved0 = a->reserved0; x.out = a->out;
    return row_call(m, &x, sel, RowCall{item_floats, false, name, "mmdx_row_blend_args"});
}

mmdx_status row_add(mmdx_model_t m, const mmdx_row_add_args *a, const mmdx_instance_select *sel, uint32_t item_floats, const char *name) {
    if (!m || !a) return fail(MMDX_ERR_INVALID_ARGUMENT, "model / args is NULL");
    if (a->struct_size != sizeof(mmdx_row_add_args)) return fail(MMDX_ERR_INVALID_ARGUMENT, "mmdx_row_add_args.struct_size mismatch");
    return row_call(m, a, sel, RowCall{item_floats, true, name, "mmdx_row_add_args"});
}

}  // namespace

extern "C" mmdx_status mmdx_pose_blend(mmdx_model_t m, const mmdx_row_blend_args *a, const mmdx_instance_select *sel) {
    return row_blend(m, a, sel, MMDX_POSE_FLOATS, "mmdx_pose_blend");
}

extern "C" mmdx_status mmdx_rate_blend(mmdx_model_t m, const mmdx_row_blend_args *a, const mmdx_instance_select *sel) {
    return row_blend(m, a, sel, 1, "mmdx_rate_blend");
}

extern "C" mmdx_status mmdx_pose_add(mmdx_model_t m, const mmdx_row_add_args *a, const mmdx_instance_select *sel) {
    return row_add(m, a, sel, MMDX_POSE_FLOATS, "mmdx_pose_add");
}

extern "C" mmdx_status mmdx_rate_add(mmdx_model_t m, const mmdx_row_add_args *a, const mmdx_instance_select *sel) {
    return row_add(m, a, sel, 1, "mmdx_rate_add");
}

// reach_api.cpp -- the reach set handle and mmdx_palette_reach (include/mmdx.h): the table of reach_table.hpp built and validated at
// creation without a device, the table's device copy on the first call that needs it, host targets and a host instance list through
// scratch of the set, the planner's shape and the launch (reach_kernels.hip) on the model's stream.  The skeleton is reached through
// skeleton_rest (rig_api.cpp) only, and only at creation.
#include <cstring>
#include <memory>
#include <new>
#include <string>
#include <vector>

#include "api_internal.hpp"
#include "reach_kernels.hpp"
#include "reach_table.hpp"

using namespace mmdx;

static_assert(kReachMaxReaches == MMDX_REACH_MAX_REACHES && kReachKeepEndRotation == MMDX_REACH_KEEP_END_ROTATION,
              "reach_math.hpp restates mmdx.h");
static_assert((MMDX_REACH_TARGETS_ON_DEVICE &
               (MMDX_ANIM_DT_ON_DEVICE | MMDX_ROOT_NORMALIZE | MMDX_EVENTS_DOMINANT_SIDE | MMDX_BLEND_A_ON_DEVICE | MMDX_BLEND_B_ON_DEVICE |
                MMDX_BLEND_PARAMS_ON_DEVICE | MMDX_PLACE_ON_DEVICE | MMDX_PLACE_MATRIX | MMDX_SPRING_RESET | MMDX_SPRING_DT_ON_DEVICE |
                MMDX_AIM_TARGETS_ON_DEVICE | 0xFFu)) == 0,
              "the reach flag shares a bit");

struct mmdx_reach_set_s {
    ReachTable t;
    int device = -1;                              // where the copy lives, -1 = not made yet
    DevBuf table;                                 // static: reaches, then subtree rows
    DevBuf tgt;                                   // host targets
    DevBuf sel;                                   // a host list: {live count, ids[live]}
    std::vector<uint32_t> sel_host;               // ... its source, alive until the copy has left it
    GraphPin pin;                                 // recorded graphs that hold these addresses
    mmdx_reach_set_s() { table.pin = tgt.pin = sel.pin = &pin; }
    size_t reach_bytes() const { return t.reaches.size() * sizeof(ReachReach); }
};

namespace {

// The table goes to the device of the first call that needs it and stays there.
mmdx_status set_to_device(mmdx_reach_set_t s, int device) {
    if (s->device == device) return MMDX_OK;
    if (s->device >= 0)
        return fail(MMDX_ERR_INVALID_ARGUMENT, "this reach set lives on device " + std::to_string(s->device) + ", the call runs on device " +
                                               std::to_string(device));
    if (graph_recording())
        return fail(MMDX_ERR_INVALID_ARGUMENT, "while a graph is being recorded the reach set must have run on this device before");
    const size_t row_bytes = s->t.rows.size() * sizeof(ReachRow);
    std::vector<char> image(s->reach_bytes() + row_bytes);
    std::memcpy(image.data(), s->t.reaches.data(), s->reach_bytes());
    std::memcpy(image.data() + s->reach_bytes(), s->t.rows.data(), row_bytes);
    if (hipError_t e = s->table.upload(image)) {
        s->table.release();
        return hip_fail(e, "reach table upload");
    }
    s->device = device;
    return MMDX_OK;
}

}  // namespace

extern "C" {

mmdx_status mmdx_reach_set_create(mmdx_skeleton_t skeleton, const mmdx_reach_set_desc *desc, mmdx_reach_set_t *out_set) {
    if (!out_set) return fail(MMDX_ERR_INVALID_ARGUMENT, "out_set is NULL");
    *out_set = nullptr;
    if (!skeleton || !desc) return fail(MMDX_ERR_INVALID_ARGUMENT, "skeleton / desc is NULL");
    try {
        const SkeletonRest sk = skeleton_rest(skeleton);
        std::vector<float> rest(size_t(sk.nb) * 3);
        for (uint32_t b = 0; b < sk.nb; ++b)
            for (int k = 0; k < 3; ++k) rest[size_t(b) * 3 + k] = -sk.neg_rest[size_t(b) * 4 + k];
        std::unique_ptr<mmdx_reach_set_s> s(new mmdx_reach_set_s);
        if (mmdx_status r = reach_table_build(desc, sk.nb, sk.parent, rest.data(), &s->t)) return r;
        *out_set = s.release();
    } catch (const std::bad_alloc &) {
        return fail(MMDX_ERR_OUT_OF_MEMORY, "host allocation failed");
    }
    return MMDX_OK;
}

void mmdx_reach_set_destroy(mmdx_reach_set_t set) {
    if (!set) return;
    graph_drop_handle(&set->pin);
    if (set->device >= 0) (void)hipSetDevice(set->device);
    set->table.release();
    set->tgt.release();
    set->sel.release();
    delete set;
}

mmdx_status mmdx_reach_set_get_info(mmdx_reach_set_t set, mmdx_reach_set_info *info) {
    if (!set || !info || info->struct_size != sizeof(mmdx_reach_set_info))
        return fail(MMDX_ERR_INVALID_ARGUMENT, "NULL argument or mmdx_reach_set_info.struct_size mismatch");
    info->n_reaches = uint32_t(set->t.reaches.size());
    info->n_subtree_rows = uint32_t(set->t.rows.size());
    info->n_bones = set->t.nb;
    info->device_ordinal = set->device;
    info->reserved0 = 0;
    return MMDX_OK;
}

mmdx_status mmdx_palette_reach(mmdx_reach_set_t set, mmdx_model_t model, const mmdx_reach_args *a) {
    if (!set || !a) return fail(MMDX_ERR_INVALID_ARGUMENT, "set / args is NULL");
    if (a->struct_size != sizeof(mmdx_reach_args)) return fail(MMDX_ERR_INVALID_ARGUMENT, "mmdx_reach_args.struct_size mismatch");
    if (a->flags & ~uint32_t(MMDX_PALETTE_ON_DEVICE | MMDX_REACH_TARGETS_ON_DEVICE))
        return fail(MMDX_ERR_INVALID_ARGUMENT, "unknown flag bits in mmdx_reach_args.flags");
    if (!(a->flags & MMDX_PALETTE_ON_DEVICE))
        return fail(MMDX_ERR_INVALID_ARGUMENT, "mmdx_palette_reach rewrites palettes in place: they must be in device memory (MMDX_PALETTE_ON_DEVICE)");
    const mmdx_instance_select *sel = a->select;
    if (sel)
        if (mmdx_status r = list_header_check(sel)) return r;
    const uint32_t ni = a->n_instances, stride = a->target_stride;
    if (stride && (stride < 4 || (stride & 3)))
        return fail(MMDX_ERR_INVALID_ARGUMENT, "mmdx_reach_args.target_stride = " + std::to_string(stride) + ": 0, or a multiple of 4 floats");
    if (!ni) return MMDX_OK;
    if (!a->palettes || !a->targets) return fail(MMDX_ERR_INVALID_ARGUMENT, "palettes / targets is NULL");
    if (reinterpret_cast<uintptr_t>(a->palettes) & 15) return fail(MMDX_ERR_INVALID_ARGUMENT, "palettes must be 16-byte aligned");
    const bool tgt_on_device = (a->flags & MMDX_REACH_TARGETS_ON_DEVICE) != 0;
    if (tgt_on_device && (reinterpret_cast<uintptr_t>(a->targets) & 15))
        return fail(MMDX_ERR_INVALID_ARGUMENT, "device targets must be 16-byte aligned");
    if (ni > kReachMaxCells || (sel && sel->n_ids > kReachMaxCells))
        return fail(MMDX_ERR_UNSUPPORTED, "mmdx_palette_reach: more than 2^23 instances or list positions in one call");
    uint32_t live_host = 0;
    if (sel) {
        if (mmdx_status r = list_placement_check(sel, graph_recording())) return r;
        if (mmdx_status r = host_list_check(sel, ni, live_host)) return r;
    }
    if (!tgt_on_device && graph_recording())
        return fail(MMDX_ERR_INVALID_ARGUMENT, "while a graph is being recorded targets must be in device memory (MMDX_REACH_TARGETS_ON_DEVICE)");
    int device;
    hipStream_t st;
    if (mmdx_status r = resolve_stream(model, &device, &st)) return r;
    if (mmdx_status r = set_to_device(set, device)) return r;
    graph_note_handle(model, &set->pin);
    const char *tb = static_cast<const char *>(set->table.ptr);
    ReachLaunch p{};
    p.palettes = a->palettes;
    p.targets = a->targets;
    p.reaches = reinterpret_cast<const ReachReach *>(tb);
    p.rows = reinterpret_cast<const ReachRow *>(tb + set->reach_bytes());
    p.ni = ni; p.nb = set->t.nb; p.n_reaches = uint32_t(set->t.reaches.size());
    p.target_stride = stride;
    InstanceList list{nullptr, nullptr, ni};
    uint32_t cells = ni;
    bool borrowed = false;
    if (sel) {
        list = InstanceList{sel->ids, sel->count, ni};
        cells = sel->n_ids;
        if (!(sel->flags & MMDX_SELECT_ON_DEVICE)) {
            cells = live_host;
            if (live_host) {
                if (mmdx_status r = stage_list(set->sel, set->sel_host, sel->ids, live_host, live_host, st, &list.count, &list.ids)) return r;
                borrowed = true;
            }
        }
        if (!cells) return MMDX_OK;
    }
    if (!tgt_on_device) {
        if (mmdx_status r = stage_in(set->tgt, a->targets, (size_t(ni - 1) * stride + 4) * sizeof(float), st)) return r;
        p.targets = static_cast<const float *>(set->tgt.ptr);
        borrowed = true;
    }
    const ReachShape shape = plan_reach_launch(cells);
    HIP_TRY(launch_reach(p, shape, sel ? &list : nullptr, cells, st));
    if (model) {
        mmdx_debug_launch_shape &r = model->last_shape;
        r = mmdx_debug_launch_shape{};
        r.kernel = MMDX_DEBUG_KERNEL_REACH;
        r.threads = shape.threads;
        r.group = shape.block;
        r.ngroups = shape.nblocks;
        r.lds = shape.lds;
        r.select = sel ? 1u : 0u;
    }
    if (borrowed) HIP_TRY(wait_stream(st));
    return MMDX_OK;
}

}  // extern "C"

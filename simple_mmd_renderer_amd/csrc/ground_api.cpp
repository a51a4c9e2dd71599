// ground_api.cpp -- the ground handle, mmdx_ground_place and mmdx_ground_targets (include/mmdx.h): the table of ground_table.hpp
// built and validated at creation without a device, the heights' device copy on the first call that needs it, a host instance list
// through scratch of the ground, the planner's shape and the launches (ground_kernels.hip) on the model's stream.
#include <memory>
#include <new>
#include <string>
#include <vector>

#include "api_internal.hpp"
#include "ground_kernels.hpp"
#include "ground_table.hpp"

using namespace mmdx;

static_assert(kGroundMaxFeet == MMDX_GROUND_MAX_FEET && kGroundMinSamples == MMDX_GROUND_MIN_SAMPLES &&
              kGroundMaxSamples == MMDX_GROUND_MAX_SAMPLES && kGroundPoseFloats == MMDX_POSE_FLOATS,
              "ground_math.hpp restates mmdx.h");

struct mmdx_ground_s {
    GroundTable t;
    int device = -1;                              // where the copy lives, -1 = not made yet
    DevBuf table;                                 // static: heights [nz][nx]
    DevBuf sel;                                   // a host list: {live count, ids[live]}
    std::vector<uint32_t> sel_host;               // ... its source, alive until the copy has left it
    GraphPin pin;                                 // recorded graphs that hold these addresses
    mmdx_ground_s() { table.pin = sel.pin = &pin; }
};

namespace {

// The heights go to the device of the first call that needs them and stay there.
mmdx_status ground_to_device(mmdx_ground_t s, int device) {
    if (s->device == device) return MMDX_OK;
    if (s->device >= 0)
        return fail(MMDX_ERR_INVALID_ARGUMENT, "this ground lives on device " + std::to_string(s->device) + ", the call runs on device " +
                                               std::to_string(device));
    if (graph_recording())
        return fail(MMDX_ERR_INVALID_ARGUMENT, "while a graph is being recorded the ground must have run on this device before");
    if (hipError_t e = s->table.upload(s->t.heights)) {
        s->table.release();
        return hip_fail(e, "ground table upload");
    }
    s->device = device;
    return MMDX_OK;
}

// What both calls do between their own argument checks and their launch: the list's checks, the stream, the table, the list's
// device form.  *cells == 0 on return: nothing to launch.
struct GroundCall {
    hipStream_t st = nullptr;
    InstanceList list{nullptr, nullptr, 0};
    uint32_t cells = 0;
    bool borrowed = false;
};
mmdx_status ground_call_begin(mmdx_ground_t ground, mmdx_model_t model, const mmdx_instance_select *sel, uint32_t ni, const char *what,
                              GroundCall *c) {
    if (sel && sel->n_ids > kGroundMaxCells)
        return fail(MMDX_ERR_UNSUPPORTED, std::string(what) + ": more than 2^23 instances or list positions in one call");
    uint32_t live_host = 0;
    if (sel) {
        if (mmdx_status r = list_placement_check(sel, graph_recording())) return r;
        if (mmdx_status r = host_list_check(sel, ni, live_host)) return r;
    }
    if (model && model->device < 0)
        return fail(MMDX_ERR_NO_DEVICE, std::string(what) + ": the model was created with MMDX_CREATE_HOST_ONLY: nothing to run on");
    int device;
    if (mmdx_status r = resolve_stream(model, &device, &c->st)) return r;
    if (mmdx_status r = ground_to_device(ground, device)) return r;
    graph_note_handle(model, &ground->pin);
    c->list = InstanceList{nullptr, nullptr, ni};
    c->cells = ni;
    if (sel) {
        c->list = InstanceList{sel->ids, sel->count, ni};
        c->cells = sel->n_ids;
        if (!(sel->flags & MMDX_SELECT_ON_DEVICE)) {
            c->cells = live_host;
            if (live_host) {
                if (mmdx_status r = stage_list(ground->sel, ground->sel_host, sel->ids, live_host, live_host, c->st, &c->list.count, &c->list.ids))
                    return r;
                c->borrowed = true;
            }
        }
    }
    return MMDX_OK;
}

}  // namespace

extern "C" {

mmdx_status mmdx_ground_create(const mmdx_ground_desc *desc, mmdx_ground_t *out_ground) {
    if (!out_ground) return fail(MMDX_ERR_INVALID_ARGUMENT, "out_ground is NULL");
    *out_ground = nullptr;
    if (!desc) return fail(MMDX_ERR_INVALID_ARGUMENT, "desc is NULL");
    try {
        std::unique_ptr<mmdx_ground_s> s(new mmdx_ground_s);
        if (mmdx_status r = ground_table_build(desc, &s->t)) return r;
        *out_ground = s.release();
    } catch (const std::bad_alloc &) {
        return fail(MMDX_ERR_OUT_OF_MEMORY, "host allocation failed");
    }
    return MMDX_OK;
}

void mmdx_ground_destroy(mmdx_ground_t ground) {
    if (!ground) return;
    graph_drop_handle(&ground->pin);
    if (ground->device >= 0) (void)hipSetDevice(ground->device);
    ground->table.release();
    ground->sel.release();
    delete ground;
}

mmdx_status mmdx_ground_get_info(mmdx_ground_t ground, mmdx_ground_info *info) {
    if (!ground || !info || info->struct_size != sizeof(mmdx_ground_info))
        return fail(MMDX_ERR_INVALID_ARGUMENT, "NULL argument or mmdx_ground_info.struct_size mismatch");
    const GroundField &g = ground->t.g;
    info->nx = g.nx; info->nz = g.nz;
    info->origin_x = g.origin_x; info->origin_z = g.origin_z;
    info->cell_x = g.cell_x; info->cell_z = g.cell_z;
    info->min_height = ground->t.min_height;
    info->max_height = ground->t.max_height;
    info->device_ordinal = ground->device;
    info->reserved0 = 0;
    return MMDX_OK;
}

mmdx_status mmdx_ground_place(mmdx_ground_t ground, mmdx_model_t model, const mmdx_ground_place_args *a) {
    if (!ground || !a) return fail(MMDX_ERR_INVALID_ARGUMENT, "ground / args is NULL");
    if (mmdx_status r = ground_place_check(a)) return r;
    const mmdx_instance_select *sel = a->select;
    if (sel)
        if (mmdx_status r = list_header_check(sel)) return r;
    if (!a->n_instances) return MMDX_OK;
    GroundCall c;
    if (mmdx_status r = ground_call_begin(ground, model, sel, a->n_instances, "mmdx_ground_place", &c)) return r;
    if (!c.cells) return MMDX_OK;
    GroundPlaceLaunch p{};
    p.g = ground->t.g;
    p.heights = static_cast<const float *>(ground->table.ptr);
    p.placements = a->placements;
    p.drop = a->drop;
    p.y_offset = a->y_offset;
    p.ni = a->n_instances;
    HIP_TRY(launch_ground_place(p, plan_ground_launch(c.cells), sel ? &c.list : nullptr, c.cells, c.st));
    if (c.borrowed) HIP_TRY(wait_stream(c.st));
    return MMDX_OK;
}

mmdx_status mmdx_ground_targets(mmdx_ground_t ground, mmdx_model_t model, const mmdx_ground_targets_args *a) {
    if (!ground || !a) return fail(MMDX_ERR_INVALID_ARGUMENT, "ground / args is NULL");
    if (mmdx_status r = ground_targets_check(a)) return r;
    const mmdx_instance_select *sel = a->select;
    if (sel)
        if (mmdx_status r = list_header_check(sel)) return r;
    if (!a->n_instances) return MMDX_OK;
    GroundCall c;
    if (mmdx_status r = ground_call_begin(ground, model, sel, a->n_instances, "mmdx_ground_targets", &c)) return r;
    if (!c.cells) return MMDX_OK;
    GroundTargetsLaunch p{};
    p.g = ground->t.g;
    p.heights = static_cast<const float *>(ground->table.ptr);
    p.placements = a->placements;
    p.points = a->points;
    p.out_targets = a->out_targets;
    p.out_drop = a->out_drop;
    p.ni = a->n_instances; p.n_feet = a->n_feet;
    p.point_stride = a->point_stride; p.slab_stride = a->slab_stride;
    p.max_step = a->max_step; p.max_drop = a->max_drop;
    HIP_TRY(launch_ground_targets(p, plan_ground_launch(c.cells), sel ? &c.list : nullptr, c.cells, c.st));
    if (c.borrowed) HIP_TRY(wait_stream(c.st));
    return MMDX_OK;
}

}  // extern "C"

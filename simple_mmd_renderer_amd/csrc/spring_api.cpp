// spring_api.cpp -- the spring set handle and mmdx_spring_step / _get_state / _set_state (include/mmdx.h): the table of
// spring_table.hpp built and validated at creation without a device, the table's device copy and the state (NaN: the first step is
// a reset) on the first call that needs them, the instance list of the select form, and the launch (spring_kernels.hip) on the
// model's stream.  The skeleton is reached through skeleton_rest (rig_api.cpp) only, and only at creation.
#include <cstring>
#include <memory>
#include <new>
#include <string>
#include <vector>

#include "api_internal.hpp"
#include "spring_kernels.hpp"
#include "spring_table.hpp"

using namespace mmdx;

static_assert(kSpringMaxJoints == MMDX_SPRING_MAX_JOINTS && kSpringMaxColliders == MMDX_SPRING_MAX_COLLIDERS,
              "spring_math.hpp restates mmdx.h");
static_assert(((MMDX_SPRING_RESET | MMDX_SPRING_DT_ON_DEVICE) &
               (MMDX_ANIM_DT_ON_DEVICE | MMDX_ROOT_NORMALIZE | MMDX_EVENTS_DOMINANT_SIDE | MMDX_BLEND_A_ON_DEVICE | MMDX_BLEND_B_ON_DEVICE |
                MMDX_BLEND_PARAMS_ON_DEVICE | MMDX_PLACE_ON_DEVICE | MMDX_PLACE_MATRIX | 0xFFu)) == 0,
              "the spring flags share a bit");

struct mmdx_spring_set_s {
    SpringTable t;
    int device = -1;                              // where the copies live, -1 = not made yet
    DevBuf table;                                 // static: chains, then joints, then colliders
    DevBuf state;                                 // [n_joints][6][max_instances]
    DevBuf sel;                                   // a host list: {live count, ids[live]}
    std::vector<uint32_t> sel_host;               // ... its source, alive until the copy has left it
    GraphPin pin;                                 // recorded graphs that hold these addresses
    mmdx_spring_set_s() { table.pin = state.pin = sel.pin = &pin; }
    size_t state_floats() const { return t.joints.size() * kSpringStateFloats * size_t(t.max_instances); }
};

namespace {

// The table and the state go to the device of the first call that needs them and stay there.
mmdx_status set_to_device(mmdx_spring_set_t s, int device, hipStream_t st) {
    if (s->device == device) return MMDX_OK;
    if (s->device >= 0)
        return fail(MMDX_ERR_INVALID_ARGUMENT, "this spring set lives on device " + std::to_string(s->device) + ", the call runs on device " +
                                               std::to_string(device));
    if (graph_recording())
        return fail(MMDX_ERR_INVALID_ARGUMENT, "while a graph is being recorded the spring set must have run on this device before");
    const size_t chain_bytes = s->t.chains.size() * sizeof(SpringChain), joint_bytes = s->t.joints.size() * sizeof(SpringJoint),
                 col_bytes = s->t.colliders.size() * sizeof(SpringCollider);
    std::vector<char> image(chain_bytes + joint_bytes + col_bytes);
    std::memcpy(image.data(), s->t.chains.data(), chain_bytes);
    std::memcpy(image.data() + chain_bytes, s->t.joints.data(), joint_bytes);
    if (col_bytes) std::memcpy(image.data() + chain_bytes + joint_bytes, s->t.colliders.data(), col_bytes);
    hipError_t e = s->table.upload(image);
    if (e == hipSuccess) e = s->state.ensure(s->state_floats() * sizeof(float));
    if (e == hipSuccess) e = hipMemsetAsync(s->state.ptr, 0xFF, s->state_floats() * sizeof(float), st);      // NaN everywhere
    if (e != hipSuccess) {
        s->table.release();
        s->state.release();
        return hip_fail(e, "spring table upload / state allocation");
    }
    s->device = device;
    return MMDX_OK;
}

mmdx_status state_call_begin(mmdx_spring_set_t set, mmdx_model_t model, uint32_t n, const void *host, int *device, hipStream_t *st) {
    if (!set || !host) return fail(MMDX_ERR_INVALID_ARGUMENT, "set / state is NULL");
    if (n > set->t.max_instances)
        return fail(MMDX_ERR_INVALID_ARGUMENT, "n_instances = " + std::to_string(n) + " is above the set's max_instances = " +
                                               std::to_string(set->t.max_instances));
    if (graph_recording()) return fail(MMDX_ERR_INVALID_ARGUMENT, "the state of a spring set cannot be copied while a graph is being recorded");
    if (mmdx_status r = resolve_stream(model, device, st)) return r;
    return set_to_device(set, *device, *st);
}

}  // namespace

extern "C" {

mmdx_status mmdx_spring_set_create(mmdx_skeleton_t skeleton, const mmdx_spring_set_desc *desc, mmdx_spring_set_t *out_set) {
    if (!out_set) return fail(MMDX_ERR_INVALID_ARGUMENT, "out_set is NULL");
    *out_set = nullptr;
    if (!skeleton || !desc) return fail(MMDX_ERR_INVALID_ARGUMENT, "skeleton / desc is NULL");
    try {
        const SkeletonRest sk = skeleton_rest(skeleton);
        std::vector<float> rest(size_t(sk.nb) * 3);
        for (uint32_t b = 0; b < sk.nb; ++b)
            for (int k = 0; k < 3; ++k) rest[size_t(b) * 3 + k] = -sk.neg_rest[size_t(b) * 4 + k];
        std::unique_ptr<mmdx_spring_set_s> s(new mmdx_spring_set_s);
        if (mmdx_status r = spring_table_build(desc, sk.nb, sk.parent, rest.data(), &s->t)) return r;
        *out_set = s.release();
    } catch (const std::bad_alloc &) {
        return fail(MMDX_ERR_OUT_OF_MEMORY, "host allocation failed");
    }
    return MMDX_OK;
}

void mmdx_spring_set_destroy(mmdx_spring_set_t set) {
    if (!set) return;
    graph_drop_handle(&set->pin);
    if (set->device >= 0) (void)hipSetDevice(set->device);
    set->table.release();
    set->state.release();
    set->sel.release();
    delete set;
}

mmdx_status mmdx_spring_set_get_info(mmdx_spring_set_t set, mmdx_spring_set_info *info) {
    if (!set || !info || info->struct_size != sizeof(mmdx_spring_set_info))
        return fail(MMDX_ERR_INVALID_ARGUMENT, "NULL argument or mmdx_spring_set_info.struct_size mismatch");
    info->n_chains = uint32_t(set->t.chains.size());
    info->n_joints = uint32_t(set->t.joints.size());
    info->n_colliders = uint32_t(set->t.colliders.size());
    info->max_instances = set->t.max_instances;
    info->n_bones = set->t.nb;
    info->device_ordinal = set->device;
    info->reserved0 = 0;
    return MMDX_OK;
}

mmdx_status mmdx_spring_step(mmdx_spring_set_t set, mmdx_model_t model, const mmdx_spring_args *a) {
    if (!set || !a) return fail(MMDX_ERR_INVALID_ARGUMENT, "set / args is NULL");
    if (a->struct_size != sizeof(mmdx_spring_args)) return fail(MMDX_ERR_INVALID_ARGUMENT, "mmdx_spring_args.struct_size mismatch");
    if (a->flags & ~uint32_t(MMDX_PALETTE_ON_DEVICE | MMDX_SPRING_RESET | MMDX_SPRING_DT_ON_DEVICE))
        return fail(MMDX_ERR_INVALID_ARGUMENT, "unknown flag bits in mmdx_spring_args.flags");
    if (!(a->flags & MMDX_PALETTE_ON_DEVICE))
        return fail(MMDX_ERR_INVALID_ARGUMENT, "mmdx_spring_step rewrites palettes in place: they must be in device memory (MMDX_PALETTE_ON_DEVICE)");
    if (a->reserved0 != 0) return fail(MMDX_ERR_INVALID_ARGUMENT, "mmdx_spring_args.reserved0 must be 0");
    const mmdx_instance_select *sel = a->select;
    if (sel)
        if (mmdx_status r = list_header_check(sel)) return r;
    const uint32_t ni = a->n_instances;
    if (ni > set->t.max_instances)
        return fail(MMDX_ERR_INVALID_ARGUMENT, "n_instances = " + std::to_string(ni) + " is above the set's max_instances = " +
                                               std::to_string(set->t.max_instances));
    if (!ni) return MMDX_OK;
    if (!a->palettes || !a->dt) return fail(MMDX_ERR_INVALID_ARGUMENT, "palettes / dt is NULL");
    if (reinterpret_cast<uintptr_t>(a->palettes) & 15) return fail(MMDX_ERR_INVALID_ARGUMENT, "palettes must be 16-byte aligned");
    const bool dt_on_device = (a->flags & MMDX_SPRING_DT_ON_DEVICE) != 0;
    if (dt_on_device && (reinterpret_cast<uintptr_t>(a->dt) & 3)) return fail(MMDX_ERR_INVALID_ARGUMENT, "a device dt must be 4-byte aligned");
    if (ni > kSpringMaxCells || (sel && sel->n_ids > kSpringMaxCells))
        return fail(MMDX_ERR_UNSUPPORTED, "mmdx_spring_step: more than 2^24 instances or list positions in one call");
    uint32_t live_host = 0;
    if (sel) {
        if (mmdx_status r = list_placement_check(sel, graph_recording())) return r;
        if (mmdx_status r = host_list_check(sel, ni, live_host)) return r;
    }
    if (!dt_on_device && graph_recording())
        return fail(MMDX_ERR_INVALID_ARGUMENT, "while a graph is being recorded dt must be in device memory (MMDX_SPRING_DT_ON_DEVICE)");
    int device;
    hipStream_t st;
    if (mmdx_status r = resolve_stream(model, &device, &st)) return r;
    if (mmdx_status r = set_to_device(set, device, st)) return r;
    graph_note_handle(model, &set->pin);
    const char *tb = static_cast<const char *>(set->table.ptr);
    SpringLaunch p{};
    p.palettes = a->palettes;
    p.state = static_cast<float *>(set->state.ptr);
    p.chains = reinterpret_cast<const SpringChain *>(tb);
    p.joints = reinterpret_cast<const SpringJoint *>(tb + set->t.chains.size() * sizeof(SpringChain));
    p.colliders = reinterpret_cast<const SpringCollider *>(tb + set->t.chains.size() * sizeof(SpringChain) +
                                                           set->t.joints.size() * sizeof(SpringJoint));
    p.ni = ni; p.nb = set->t.nb; p.n_chains = uint32_t(set->t.chains.size()); p.nc = uint32_t(set->t.colliders.size());
    p.max_instances = set->t.max_instances;
    for (int k = 0; k < 3; ++k) p.gravity[k] = set->t.gravity[k];
    p.reset = (a->flags & MMDX_SPRING_RESET) ? 1u : 0u;
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
    HIP_TRY(launch_spring_step(p, sel ? &list : nullptr, cells, dt_on_device ? 0.0f : *a->dt, dt_on_device ? a->dt : nullptr, st));
    if (borrowed) HIP_TRY(wait_stream(st));
    return MMDX_OK;
}

mmdx_status mmdx_spring_get_state(mmdx_spring_set_t set, mmdx_model_t model, uint32_t n, float *out_state) {
    int device;
    hipStream_t st;
    if (mmdx_status r = state_call_begin(set, model, n, out_state, &device, &st)) return r;
    if (!n) return MMDX_OK;
    const size_t rows = set->t.joints.size() * kSpringStateFloats;
    try {
        std::vector<float> slab(rows * n);
        HIP_TRY(hipMemcpy2DAsync(slab.data(), size_t(n) * 4, set->state.ptr, size_t(set->t.max_instances) * 4, size_t(n) * 4, rows,
                                 hipMemcpyDeviceToHost, st));
        HIP_TRY(wait_stream(st));
        for (size_t r = 0; r < rows; ++r)
            for (uint32_t i = 0; i < n; ++i) out_state[size_t(i) * rows + r] = slab[r * n + i];
    } catch (const std::bad_alloc &) {
        return fail(MMDX_ERR_OUT_OF_MEMORY, "host allocation failed");
    }
    return MMDX_OK;
}

mmdx_status mmdx_spring_set_state(mmdx_spring_set_t set, mmdx_model_t model, uint32_t n, const float *state) {
    int device;
    hipStream_t st;
    if (mmdx_status r = state_call_begin(set, model, n, state, &device, &st)) return r;
    if (!n) return MMDX_OK;
    const size_t rows = set->t.joints.size() * kSpringStateFloats;
    try {
        std::vector<float> slab(rows * n);
        for (size_t r = 0; r < rows; ++r)
            for (uint32_t i = 0; i < n; ++i) slab[r * n + i] = state[size_t(i) * rows + r];
        HIP_TRY(hipMemcpy2DAsync(set->state.ptr, size_t(set->t.max_instances) * 4, slab.data(), size_t(n) * 4, size_t(n) * 4, rows,
                                 hipMemcpyHostToDevice, st));
        HIP_TRY(wait_stream(st));
    } catch (const std::bad_alloc &) {
        return fail(MMDX_ERR_OUT_OF_MEMORY, "host allocation failed");
    }
    return MMDX_OK;
}

}  // extern "C"

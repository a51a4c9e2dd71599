// cull_api.cpp -- mmdx_cull_bounds and mmdx_cull_planes_from_matrix (include/mmdx.h): argument and view validation on the host, the
// planner (cull_shape.cpp), the handle's count scratch and the launches (cull_kernels.hip) on the handle's stream.
#include <cmath>
#include <cstring>
#include <string>

#include "api_internal.hpp"
#include "cull_kernels.hpp"

using namespace mmdx;

namespace {

CullOverrides read_cull_overrides() { return {env_int("MMDX_CULL_FORM", 0), env_int("MMDX_CULL_CHUNK", 0)}; }
CullOverrides &cull_overrides() {
    static CullOverrides o = read_cull_overrides();
    return o;
}

// A view in host memory: everything the header promises to reject, before anything touches the device
mmdx_status validate_view(const mmdx_cull_view &v) {
    if (v.n_planes > MMDX_CULL_MAX_PLANES)
        return fail(MMDX_ERR_INVALID_ARGUMENT, "mmdx_cull_view.n_planes = " + std::to_string(v.n_planes) + " (at most 16)");
    if (v.n_lods < 1 || v.n_lods > MMDX_CULL_MAX_LODS)
        return fail(MMDX_ERR_INVALID_ARGUMENT, "mmdx_cull_view.n_lods = " + std::to_string(v.n_lods) + " (1..4)");
    if (!(v.margin >= 0.0f)) return fail(MMDX_ERR_INVALID_ARGUMENT, "mmdx_cull_view.margin is negative or NaN");
    for (uint32_t k = 0; k + 1 < v.n_lods; ++k) {
        if (std::isnan(v.lod_distance[k])) return fail(MMDX_ERR_INVALID_ARGUMENT, "mmdx_cull_view.lod_distance holds a NaN");
        if (k && v.lod_distance[k] < v.lod_distance[k - 1])
            return fail(MMDX_ERR_INVALID_ARGUMENT, "mmdx_cull_view.lod_distance must ascend");
    }
    if (v.reserved0 != 0) return fail(MMDX_ERR_INVALID_ARGUMENT, "mmdx_cull_view.reserved0 must be 0");
    return MMDX_OK;
}

}  // namespace

void mmdx::reload_cull_overrides() { cull_overrides() = read_cull_overrides(); }

extern "C" {

mmdx_status mmdx_cull_bounds(mmdx_model_t m, const mmdx_cull_args *a) {
    if (!m || !a) return fail(MMDX_ERR_INVALID_ARGUMENT, "model / args is NULL");
    if (a->struct_size != sizeof(mmdx_cull_args)) return fail(MMDX_ERR_INVALID_ARGUMENT, "mmdx_cull_args.struct_size mismatch");
    if (a->flags & ~uint32_t(MMDX_CULL_VIEW_ON_DEVICE)) return fail(MMDX_ERR_INVALID_ARGUMENT, "unknown bits in mmdx_cull_args.flags");
    const bool view_dev = (a->flags & MMDX_CULL_VIEW_ON_DEVICE) != 0;
    const uint32_t ni = a->n_instances;
    if (!a->view || !a->out_counts || (ni && (!a->bounds || !a->out_ids)))
        return fail(MMDX_ERR_INVALID_ARGUMENT, "bounds / view / out_ids / out_counts is NULL");
    if (a->list_stride < ni) return fail(MMDX_ERR_INVALID_ARGUMENT, "mmdx_cull_args.list_stride is smaller than n_instances");
    uintptr_t dev_bits = reinterpret_cast<uintptr_t>(a->bounds) | reinterpret_cast<uintptr_t>(a->out_ids) |
                         reinterpret_cast<uintptr_t>(a->out_counts) | reinterpret_cast<uintptr_t>(a->out_levels);
    if (view_dev) dev_bits |= reinterpret_cast<uintptr_t>(a->view);
    if (dev_bits & 3) return fail(MMDX_ERR_INVALID_ARGUMENT, "device pointers of mmdx_cull_args must be 4-byte aligned");
    if (!view_dev)
        if (mmdx_status s = validate_view(*a->view)) return s;
    if (mmdx_status r = model_call_begin(m, 0, 0, nullptr)) return r;      // (a host view is read here, at the call: recordable)
    const CullShape shape = plan_cull_launch(ni, cull_overrides());
    if (shape.scratch_bytes) HIP_TRY(m->cull.ensure(shape.scratch_bytes));
    const CullLaunch call{a->bounds, view_dev ? a->view : nullptr, view_dev ? nullptr : a->view, a->out_ids, a->out_counts, a->out_levels,
                          ni, a->list_stride, static_cast<uint32_t *>(m->cull.ptr)};
    HIP_TRY(launch_cull(call, shape, m->stream));
    mmdx_debug_launch_shape &r = m->last_shape;
    r = mmdx_debug_launch_shape{};
    r.kernel = MMDX_DEBUG_KERNEL_CULL;
    r.threads = shape.threads;
    r.group = shape.chunk;
    r.ngroups = shape.nchunks;
    r.select = shape.form;
    return MMDX_OK;
}

mmdx_status mmdx_cull_planes_from_matrix(const float m[16], uint32_t depth_zero_to_one, float out_planes[6][4]) {
    if (!m || !out_planes) return fail(MMDX_ERR_INVALID_ARGUMENT, "m / out_planes is NULL");
    for (int k = 0; k < 4; ++k) {
        const float r0 = m[4 * k + 0], r1 = m[4 * k + 1], r2 = m[4 * k + 2], r3 = m[4 * k + 3];   // component k of row_0 .. row_3
        out_planes[0][k] = r3 + r0;
        out_planes[1][k] = r3 - r0;
        out_planes[2][k] = r3 + r1;
        out_planes[3][k] = r3 - r1;
        out_planes[4][k] = depth_zero_to_one ? r2 : r3 + r2;
        out_planes[5][k] = r3 - r2;
    }
    return MMDX_OK;
}

}  // extern "C"

// ground_table.hpp -- a ground's table and its host builder: what mmdx_ground_create (ground_api.cpp) validates and uploads, the
// argument checks of mmdx_ground_place and mmdx_ground_targets that need no device, and the planner of the kernels' launch.  No HIP
// here: tests/ground_math_driver.cpp compiles these lines with g++ (and under ASan + UBSan).
#pragma once

#include <cstdint>
#include <string>
#include <vector>

#include "../../include/mmdx.h"
#include "error.hpp"
#include "ground_math.hpp"

namespace mmdx {

// One lane per instance (list position), one wave per workgroup: a launch-bound kernel spreads over the CUs soonest that way, and
// the gathers of 64 instances are in flight together.
constexpr uint32_t kGroundThreads = 64;
constexpr uint32_t kGroundMaxCells = 1u << 23;     // instances or list positions in one call

struct GroundShape {
    uint32_t threads;         // lanes per workgroup = instances per workgroup
    uint32_t nblocks;         // ceil(cells / threads)
};

// cells: instances, or list positions of a select call (> 0)
inline GroundShape plan_ground_launch(uint32_t cells) {
    GroundShape s{};
    s.threads = kGroundThreads;
    s.nblocks = (cells + s.threads - 1) / s.threads;
    return s;
}

struct GroundTable {
    GroundField g{};
    std::vector<float> heights;                    // [nz][nx]
    float min_height = 0.0f, max_height = 0.0f;
};

// The table `d` describes, validated.
inline mmdx_status ground_table_build(const mmdx_ground_desc *d, GroundTable *out) {
    const auto bad = [](const std::string &m) { return fail(MMDX_ERR_INVALID_ARGUMENT, "mmdx_ground_desc: " + m); };
    if (!d) return fail(MMDX_ERR_INVALID_ARGUMENT, "desc is NULL");
    if (d->struct_size != sizeof(mmdx_ground_desc)) return bad("struct_size mismatch");
    if (d->flags != 0) return bad("unknown flag bits (none are defined)");
    if (d->reserved0 != 0) return bad("reserved0 must be 0");
    if (d->nx < kGroundMinSamples || d->nx > kGroundMaxSamples || d->nz < kGroundMinSamples || d->nz > kGroundMaxSamples)
        return bad("nx = " + std::to_string(d->nx) + ", nz = " + std::to_string(d->nz) + ": 2 to 8192 each");
    if (!ground_finite(d->cell_x) || !ground_finite(d->cell_z) || !(d->cell_x > 0.0f) || !(d->cell_z > 0.0f))
        return bad("cell_x / cell_z must be finite and > 0");
    if (!ground_finite(d->origin_x) || !ground_finite(d->origin_z)) return bad("origin_x / origin_z must be finite");
    if (!d->heights) return bad("heights is NULL");
    const size_t n = size_t(d->nx) * d->nz;
    float lo = d->heights[0], hi = d->heights[0];
    for (size_t k = 0; k < n; ++k) {
        const float v = d->heights[k];
        if (!ground_finite(v)) return bad("heights[" + std::to_string(k / d->nx) + "][" + std::to_string(k % d->nx) + "] is not finite");
        lo = v < lo ? v : lo;
        hi = v > hi ? v : hi;
    }
    GroundTable t;
    t.g = GroundField{d->nx, d->nz, d->origin_x, d->origin_z, d->cell_x, d->cell_z};
    t.heights.assign(d->heights, d->heights + n);
    t.min_height = lo;
    t.max_height = hi;
    *out = std::move(t);
    return MMDX_OK;
}

// [a, a + na) and [b, b + nb) floats share a byte
inline bool ground_overlap(const float *a, size_t na, const float *b, size_t nb) {
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
    return a0 < b0 + nb * 4 && b0 < a0 + na * 4;
}

// What mmdx_ground_place refuses before it looks for a device (the list's checks are host_runtime.hpp's).
inline mmdx_status ground_place_check(const mmdx_ground_place_args *a) {
    if (!a) return fail(MMDX_ERR_INVALID_ARGUMENT, "args is NULL");
    if (a->struct_size != sizeof(mmdx_ground_place_args)) return fail(MMDX_ERR_INVALID_ARGUMENT, "mmdx_ground_place_args.struct_size mismatch");
    if (a->flags != 0) return fail(MMDX_ERR_INVALID_ARGUMENT, "unknown flag bits in mmdx_ground_place_args.flags (none are defined)");
    if (!a->n_instances) return MMDX_OK;
    if (!a->placements) return fail(MMDX_ERR_INVALID_ARGUMENT, "placements is NULL");
    if ((reinterpret_cast<uintptr_t>(a->placements) | reinterpret_cast<uintptr_t>(a->drop)) & 3)
        return fail(MMDX_ERR_INVALID_ARGUMENT, "placements / drop must be 4-byte aligned");
    if (a->n_instances > kGroundMaxCells)
        return fail(MMDX_ERR_UNSUPPORTED, "mmdx_ground_place: more than 2^23 instances or list positions in one call");
    if (a->drop && ground_overlap(a->drop, a->n_instances, a->placements, size_t(a->n_instances) * kGroundPoseFloats))
        return fail(MMDX_ERR_INVALID_ARGUMENT, "drop overlaps placements");
    return MMDX_OK;
}

// What mmdx_ground_targets refuses before it looks for a device.
inline mmdx_status ground_targets_check(const mmdx_ground_targets_args *a) {
    const auto bad = [](const std::string &m) { return fail(MMDX_ERR_INVALID_ARGUMENT, "mmdx_ground_targets_args: " + m); };
    if (!a) return fail(MMDX_ERR_INVALID_ARGUMENT, "args is NULL");
    if (a->struct_size != sizeof(mmdx_ground_targets_args)) return bad("struct_size mismatch");
    if (a->flags != 0) return bad("unknown flag bits (none are defined)");
    if (!a->n_feet || a->n_feet > kGroundMaxFeet) return bad("n_feet = " + std::to_string(a->n_feet) + ": 1 to MMDX_GROUND_MAX_FEET (8)");
    if (a->point_stride < 3 || a->slab_stride < 3)
        return bad("point_stride = " + std::to_string(a->point_stride) + ", slab_stride = " + std::to_string(a->slab_stride) +
                   ": a point is three floats");
    if (!ground_finite(a->max_step) || !ground_finite(a->max_drop) || !(a->max_step >= 0.0f) || !(a->max_drop >= 0.0f))
        return bad("max_step / max_drop must be finite and >= 0");
    const size_t ni = a->n_instances, nf = a->n_feet;
    if (!ni) return MMDX_OK;
    if (!a->placements || !a->points || !a->out_targets) return bad("placements / points / out_targets is NULL");
    if ((reinterpret_cast<uintptr_t>(a->placements) | reinterpret_cast<uintptr_t>(a->points) | reinterpret_cast<uintptr_t>(a->out_drop)) & 3)
        return bad("placements / points / out_drop must be 4-byte aligned");
    if (reinterpret_cast<uintptr_t>(a->out_targets) & 15) return bad("out_targets must be 16-byte aligned");
    if (ni > kGroundMaxCells) return fail(MMDX_ERR_UNSUPPORTED, "mmdx_ground_targets: more than 2^23 instances or list positions in one call");
    const size_t n_points = (nf - 1) * a->slab_stride + (ni - 1) * a->point_stride + 3, n_place = ni * kGroundPoseFloats, n_out = nf * ni * 4;
    if (ground_overlap(a->out_targets, n_out, a->points, n_points) || ground_overlap(a->out_targets, n_out, a->placements, n_place))
        return bad("out_targets overlaps points or placements");
    if (a->out_drop && (ground_overlap(a->out_drop, ni, a->points, n_points) || ground_overlap(a->out_drop, ni, a->placements, n_place) ||
                        ground_overlap(a->out_drop, ni, a->out_targets, n_out)))
        return bad("out_drop overlaps points, placements or out_targets");
    return MMDX_OK;
}

}  // namespace mmdx

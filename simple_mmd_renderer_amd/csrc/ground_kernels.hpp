// ground_kernels.hpp -- launch interface between ground_api.cpp (mmdx_ground_place, mmdx_ground_targets) and the gfx950 kernels of
// ground_kernels.hip (the field is ground_math.hpp's, the shape of the launch is ground_table.hpp's planner's).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "ground_math.hpp"
#include "ground_table.hpp"
#include "instance_list.hpp"

namespace mmdx {

struct GroundPlaceLaunch {
    GroundField g;
    const float *heights;            // device [nz][nx]
    float *placements;               // device [ni][8]; [i][0] and [i][2] are read, [i][1] is written
    const float *drop;               // device [ni] or nullptr; never overlaps placements
    float y_offset;
    uint32_t ni;
};

struct GroundTargetsLaunch {
    GroundField g;
    const float *heights;            // device [nz][nx]
    const float *placements;         // device [ni][8]
    const float *points;             // device: foot f of instance i at f * slab_stride + i * point_stride, three floats
    float *out_targets;              // device [n_feet][ni][4], 16-byte aligned; overlaps no input
    float *out_drop;                 // device [ni] or nullptr; overlaps no input and not out_targets
    uint32_t ni, n_feet;             // n_feet 1 .. 8
    uint32_t point_stride, slab_stride;
    float max_step, max_drop;
};

// One launch each on `stream`: shape.nblocks workgroups of shape.threads lanes, no LDS.  list == nullptr: every instance (cells =
// ni); else `cells` list positions, list->n_rows == ni.  shape = plan_ground_launch(cells).
hipError_t launch_ground_place(const GroundPlaceLaunch &p, const GroundShape &shape, const InstanceList *list, uint32_t cells, hipStream_t stream);
hipError_t launch_ground_targets(const GroundTargetsLaunch &p, const GroundShape &shape, const InstanceList *list, uint32_t cells,
                                 hipStream_t stream);

}  // namespace mmdx

// reach_kernels.hpp -- launch interface between reach_api.cpp (mmdx_palette_reach) and the gfx950 kernel of reach_kernels.hip (the
// rows of a reach set's device table are reach_math.hpp's, the shape of the launch is reach_table.hpp's planner's).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "instance_list.hpp"
#include "reach_math.hpp"
#include "reach_table.hpp"

namespace mmdx {

struct ReachLaunch {
    float *palettes;                 // device [ni][nb][16], 16-byte aligned, rewritten in place
    const float *targets;            // device, 16-byte aligned: 4 floats per instance at i * target_stride, or 4 floats for all
    const ReachReach *reaches;       // device [n_reaches]; a, b, c < nb
    const ReachRow *rows;            // device [n_rows]; every bone < nb, every depth < 3
    uint32_t ni, nb, n_reaches;
    uint32_t target_stride;          // floats; 0 = one target for everyone
};

// One launch on `stream`: grid (shape.nblocks, n_reaches), shape.threads lanes, shape.lds bytes of LDS.  list == nullptr: every
// instance (cells = ni); else `cells` list positions, list->n_rows == ni.  shape = plan_reach_launch(cells).
hipError_t launch_reach(const ReachLaunch &p, const ReachShape &shape, const InstanceList *list, uint32_t cells, hipStream_t stream);

}  // namespace mmdx

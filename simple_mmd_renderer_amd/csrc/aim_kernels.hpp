// aim_kernels.hpp -- launch interface between aim_api.cpp (mmdx_palette_aim) and the gfx950 kernel of aim_kernels.hip (the rows of
// an aim set's device table are aim_math.hpp's, the shape of the launch is aim_table.hpp's planner's).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "aim_math.hpp"
#include "aim_table.hpp"
#include "instance_list.hpp"

namespace mmdx {

struct AimLaunch {
    float *palettes;                 // device [ni][nb][16], 16-byte aligned, rewritten in place
    const float *targets;            // device, 16-byte aligned: 4 floats per instance at i * target_stride, or 4 floats for all
    const AimAim *aims;              // device [n_aims]
    const AimLink *links;            // device [n_links]; every bone < nb
    const AimRow *rows;              // device [n_rows]; every bone < nb, every depth < its aim's n_links
    uint32_t ni, nb, n_aims, max_links;
    uint32_t target_stride;          // floats; 0 = one target for everyone
};

// One launch on `stream`: grid (shape.nblocks, n_aims), shape.threads lanes, shape.lds bytes of LDS.  list == nullptr: every instance
// (cells = ni); else `cells` list positions, list->n_rows == ni.  shape = plan_aim_launch(cells, p.max_links, ...).
hipError_t launch_aim(const AimLaunch &p, const AimShape &shape, const InstanceList *list, uint32_t cells, hipStream_t stream);

}  // namespace mmdx

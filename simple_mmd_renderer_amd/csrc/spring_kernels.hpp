// spring_kernels.hpp -- launch interface between spring_api.cpp (mmdx_spring_step) and the gfx950 kernel of spring_kernels.hip (the
// rows of a spring set's device table are spring_math.hpp's).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "instance_list.hpp"
#include "spring_math.hpp"

namespace mmdx {

constexpr uint32_t kSpringThreads = 64;             // one wave per workgroup: (64 list positions, one chain)
constexpr uint32_t kSpringMaxCells = 1u << 24;      // instances or list positions in one call

struct SpringLaunch {
    float *palettes;                 // device [ni][nb][16], 16-byte aligned, rewritten in place
    float *state;                    // device [n_joints][6][max_instances], instance fastest
    const SpringChain *chains;       // device [n_chains]
    const SpringJoint *joints;       // device [n_joints]; every bone < nb
    const SpringCollider *colliders; // device [nc]; every bone < nb
    uint32_t ni, nb, n_chains, nc, max_instances;      // ni <= max_instances
    float gravity[3];
    uint32_t reset;                  // MMDX_SPRING_RESET
};

// One launch on `stream`: grid (ceil(cells / 64), n_chains).  list == nullptr: every instance (cells = ni); else `cells` list
// positions, list->n_rows == ni.  dt_dev != nullptr: the step is read from device memory when the kernel runs, `dt` is ignored.
hipError_t launch_spring_step(const SpringLaunch &p, const InstanceList *list, uint32_t cells, float dt, const float *dt_dev,
                              hipStream_t stream);

}  // namespace mmdx

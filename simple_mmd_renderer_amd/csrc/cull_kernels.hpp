// cull_kernels.hpp -- launch interface between cull_api.cpp (mmdx_cull_bounds) and the gfx950 kernels of cull_kernels.hip.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/mmdx.h"
#include "cull_shape.hpp"

namespace mmdx {

struct CullLaunch {
    const float *bounds;               // device [ni][6]
    const mmdx_cull_view *view_dev;    // the view in device memory, read by the kernels when they run; nullptr: view_host is used
    const mmdx_cull_view *view_host;   // ... else a validated view in host memory, handed to the kernels by value
    uint32_t *out_ids, *out_counts, *out_levels;   // device; out_levels may be nullptr
    uint32_t ni, list_stride;
    uint32_t *scratch;                 // form 2: [nchunks][4] counts, 16-byte aligned (the handle's scratch); form 1: unused
};

// One launch (form 1) or two (form 2) on `stream`, as `shape` says (cull_shape.hpp).
hipError_t launch_cull(const CullLaunch &c, const CullShape &shape, hipStream_t stream);

}  // namespace mmdx

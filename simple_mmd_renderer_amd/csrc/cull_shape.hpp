// cull_shape.hpp -- the shape of one mmdx_cull_bounds call (which of the two forms, instances per chunk, chunks), decided from values
// alone like launch_shape.hpp: no handle, no HIP call, no environment.  Pure C++17, swept on a machine without a GPU
// (tests/cull_shape_driver.cpp, tests/test_cull_bounds.py).
#pragma once

#include <cstddef>
#include <cstdint>

namespace mmdx {

// MMDX_CULL_FORM / MMDX_CULL_CHUNK (A/B runs and tests): read once per process, re-read by mmdx_debug_reload_env.  0 = not set.
struct CullOverrides {
    int form;     // 1 | 2 forces a form; anything else: the planner chooses
    int chunk;    // instances per chunk: rounded down to a multiple of 64 and clamped to [64, 1024]; <= 0: the planner chooses
};

constexpr uint32_t kCullMinChunk = 64, kCullMaxChunk = 1024;
// One workgroup walks crowds of up to this many instances; larger ones take the two launches.  UNMEASURED: the issue's starting figure,
// to be replaced by the smallest swept crowd at which form 2 is faster (tools/cull_ab.py).
constexpr uint32_t kCullCrossover = 4096;

struct CullShape {
    uint32_t form;            // 1: one workgroup walks the chunks and carries the running bases; 2: a count launch, then a scatter launch
    uint32_t chunk;           // instances per chunk = lanes per workgroup
    uint32_t threads;         // lanes per workgroup (= chunk)
    uint32_t nchunks;         // ceil(ni / chunk), at least 1: an empty crowd still writes its zero counts
    size_t scratch_bytes;     // form 2: nchunks x 4 counts of 4 bytes in the handle's scratch; form 1: 0
};

CullShape plan_cull_launch(uint32_t ni, const CullOverrides &ov);

}  // namespace mmdx

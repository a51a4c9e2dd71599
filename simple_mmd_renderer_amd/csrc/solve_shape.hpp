// solve_shape.hpp -- which compilation of the ordered bone solver a launch takes (plain, nested, or the two-workgroups-per-CU
// DENSE one), decided from values alone like launch_shape.hpp and cull_shape.hpp: no handle, no HIP call, no environment.
// Pure C++17, swept on a machine without a GPU (tests/solve_shape_driver.cpp, tests/test_solve_dense.py).
#pragma once

#include <cstddef>
#include <cstdint>

namespace mmdx {

// A CU has 160 KB of LDS: two workgroups are resident together only when twice a workgroup's dynamic LDS, plus 1 KB each for the
// kernel's static share and the allocation granule, fits.
constexpr size_t kSolveDenseLdsBudget = 160 * 1024, kSolveDenseLdsSlack = 1024;

// dense_env: MMDX_SOLVE_DENSE as read for this call: 0 never, 1 whenever it fits, anything else (unset: -1) by crowd size -- dense
// once the launch has more workgroups than the device has CUs, when a second resident workgroup is what hides the first one's stalls.
// Nested IK has no dense compilation (its 512 registers leave no room for a second workgroup).
inline bool plan_solve_dense(bool nested, size_t lds_bytes, uint32_t workgroups, uint32_t cus, int dense_env) {
    if (nested || 2 * (lds_bytes + kSolveDenseLdsSlack) > kSolveDenseLdsBudget) return false;
    if (dense_env == 1) return true;
    if (dense_env == 0) return false;
    return workgroups > cus;
}

// What one ordered solve launched (mmdx_debug_last_solve_shape); host state, recorded by the launcher.
struct SolveShape {
    uint32_t solver = 0;            // 0: no solve yet, 1: the ordered solver, 2: parallel FK (nothing below applies)
    uint32_t nested = 0, dense = 0, select = 0;
    uint32_t workgroups = 0;        // of every ordered-segment launch: ceil(state cells / 16)
    uint32_t lds = 0;               // bytes of dynamic LDS of those launches
    uint32_t segments = 0;          // ordered-segment launches of the call
    uint32_t coop_launches = 0;     // ik_coop launches of the call
};

}  // namespace mmdx

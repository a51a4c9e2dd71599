// row_blend_kernels.hpp -- launch interface between row_blend_api.cpp (mmdx_pose_blend, mmdx_rate_blend) and the gfx950 kernels of
// row_blend_kernels.hip.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "instance_list.hpp"

namespace mmdx {

constexpr uint32_t kRowBlendThreads = 256;           // lanes per workgroup when a row has that many items; else the row, rounded up to a wave
constexpr uint32_t kRowBlendMaxCells = 1u << 23;     // grid x = instances or list positions: cells * kRowBlendThreads stays below 2^32
constexpr uint32_t kMaskNone = 0xFFFFFFFFu;          // MMDX_MASK_NONE

struct RowBlendLaunch {
    const float *a, *b;              // device [ni][items][8] (poses, 16-byte aligned) or [ni][items] (rates)
    const float *weights;            // device [ni]
    const uint32_t *mask_ids;        // device [ni], or nullptr = kMaskNone for everyone
    const float *masks;              // device [n_masks][items]; not read when n_masks == 0
    float *out;                      // same shape as a; == a, == b or disjoint from both
    uint32_t ni, items, n_masks;
};

// Lanes per workgroup and workgroups per row of `items` items (pure: also what the tests state the shapes by)
inline uint32_t row_blend_threads(uint32_t items) {
    return items >= kRowBlendThreads ? kRowBlendThreads : (items + 63) / 64 * 64;
}
inline uint32_t row_blend_chunks(uint32_t items) {
    const uint32_t t = row_blend_threads(items);
    return uint32_t((uint64_t(items) + t - 1) / t);
}

// One launch on `stream`.  ni and items are non-zero and row_blend_chunks(items) <= 65535.  list == nullptr: every instance, ni <=
// kRowBlendMaxCells; else `cells` list positions (0 < cells <= kRowBlendMaxCells), list->n_rows == ni.
hipError_t launch_pose_blend(const RowBlendLaunch &p, const InstanceList *list, uint32_t cells, hipStream_t stream);
hipError_t launch_rate_blend(const RowBlendLaunch &p, const InstanceList *list, uint32_t cells, hipStream_t stream);

}  // namespace mmdx

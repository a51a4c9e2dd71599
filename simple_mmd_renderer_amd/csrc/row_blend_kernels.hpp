// row_blend_kernels.hpp -- launch interface between row_blend_api.cpp (mmdx_pose_blend, mmdx_rate_blend, mmdx_pose_add,
// mmdx_rate_add) and the gfx950 kernels of row_blend_kernels.hip; pose_add_kernel lives in rig_kernels.hip (rig_kernels.hpp) and
// takes the row and the effective weight from the two device helpers below, as the kernels here do.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "instance_list.hpp"

namespace mmdx {

constexpr uint32_t kRowBlendThreads = 256;           // lanes per workgroup when a row has that many items; else the row, rounded up to a wave
constexpr uint32_t kRowBlendMaxCells = 1u << 23;     // grid x = instances or list positions: cells * kRowBlendThreads stays below 2^32
constexpr uint32_t kMaskNone = 0xFFFFFFFFu;          // MMDX_MASK_NONE
constexpr uint32_t kRefNone = 0xFFFFFFFFu;           // MMDX_REF_NONE

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

// mmdx_pose_add / mmdx_rate_add: the blend's operands and the reference rows
struct RowAddLaunch {
    RowBlendLaunch rows;             // a, b, weights, mask_ids, masks, out, ni, items, n_masks as above
    const uint32_t *ref_ids;         // device [ni], or nullptr = kRefNone for everyone
    const float *refs;               // device [n_refs][items][8] (poses, 16-byte aligned) or [n_refs][items] (rates); not read when
    uint32_t n_refs;                 // n_refs == 0
};

// the row a workgroup works on: false = none (a dead list position, or an in-place row that already holds its result)
template <bool kSelect>
__device__ __forceinline__ bool blend_row(const InstanceList &list, const float *__restrict__ weights, bool in_place_a, uint32_t &i,
                                          float &w) {
    i = blockIdx.x;
    if (kSelect) {
        const ListedInstances li{list};
        const Lane ln = li.lane(blockIdx.x, li.used(gridDim.x));
        if (!ln.live) return false;
        i = ln.row;
    }
    w = weights[i];
    return !(in_place_a && (w == 0.0f || w != w));
}

// the effective weight of item j of instance i: one binary32 multiply (by 1.0f without a mask: exactly w)
__device__ __forceinline__ float effective_weight(float w, const uint32_t *__restrict__ mask_ids, const float *__restrict__ masks,
                                                  uint32_t n_masks, uint32_t items, uint32_t i, uint32_t j) {
    const uint32_t m = mask_ids ? mask_ids[i] : kMaskNone;
    float mv = 1.0f;
    if (m != kMaskNone) mv = m < n_masks ? masks[size_t(m) * items + j] : 0.0f;
    return w * mv;
}

// One launch on `stream`.  ni and items are non-zero and row_blend_chunks(items) <= 65535.  list == nullptr: every instance, ni <=
// kRowBlendMaxCells; else `cells` list positions (0 < cells <= kRowBlendMaxCells), list->n_rows == ni.
hipError_t launch_pose_blend(const RowBlendLaunch &p, const InstanceList *list, uint32_t cells, hipStream_t stream);
hipError_t launch_rate_blend(const RowBlendLaunch &p, const InstanceList *list, uint32_t cells, hipStream_t stream);
hipError_t launch_rate_add(const RowAddLaunch &p, const InstanceList *list, uint32_t cells, hipStream_t stream);

}  // namespace mmdx

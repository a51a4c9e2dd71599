// instance_list.hpp -- the device form of an mmdx_instance_select and which instance a lane of a kernel works on: shared by the
// kernels of rig_kernels.hip (mmdx_skeleton_solve_select, the bone side of the track calls) and of kernels.hip (the morph side,
// flatten, bounds), so every select call reads a list the same way and a select form is its plain form with another Instances.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace mmdx {

struct InstanceList {
    const uint32_t *ids;                        // [capacity], device memory
    const uint32_t *count;                      // device memory; the first min(*count, capacity) ids are used; nullptr = all
    uint32_t n_rows;                            // NI: rows of poses / rates / palettes; an id >= n_rows is skipped
};

// `cell` indexes what a call keeps per instance in its own scratch (the ordered solver's state, the bone-morph state: p.ni cells,
// instance fastest), `row` the caller's arrays (poses, rates, palettes).  The plain calls: cell k is instance k and so is its row.
// mmdx_skeleton_solve_select: cell k is LIST POSITION k -- an id listed twice gets two cells, two solves and the same bytes twice --
// and the row is ids[k]; positions behind min(*count, capacity) and ids that are no row of the arrays are dead.  p.ni is the number of
// cells: the instance count of a plain call, the list's capacity of a select call.  A kernel body shared by a plain and a select
// form takes either of the two below; the other plain kernels derive cell = row = instance themselves, as they always did.
struct Lane {
    uint32_t cell, row;
    bool live;
};
struct AllInstances {
    static constexpr bool kListed = false;
    __device__ __forceinline__ uint32_t used(uint32_t cells) const { return cells; }
    __device__ __forceinline__ Lane lane(uint32_t k, uint32_t used) const { return {k, k, k < used}; }
};
struct ListedInstances {
    static constexpr bool kListed = true;
    InstanceList l;
    // (the same address in every lane: one scalar load per wave, once per kernel)
    __device__ __forceinline__ uint32_t used(uint32_t cells) const { return l.count ? min(*l.count, cells) : cells; }
    __device__ __forceinline__ Lane lane(uint32_t k, uint32_t used) const {
        const bool in = k < used;
        const uint32_t id = in ? l.ids[k] : 0u;
        return {k, id, in && id < l.n_rows};
    }
};

// The lane of a kernel with one thread per (cell, item) -- `per` bones or morphs to a cell, THREADS to a workgroup, an x-grid over
// `cells` of them: its instance, its item and `at` = row * per + item, where the item sits in a [rows][per] array of the caller.
// false: the lane has nothing to do -- it is behind the end or behind the count, or its id is no row.  Workgroups wholly behind a
// list's count leave first (one scalar compare, before any lane reads an id).
struct LaneItem {
    Lane ln;
    uint32_t item;
    size_t at;
};
template <uint32_t THREADS, class Instances>
__device__ __forceinline__ bool lane_item(const Instances &sel, uint32_t cells, uint32_t per, LaneItem &it) {
    const uint32_t used = sel.used(cells);
    const size_t n = size_t(used) * per;
    if (Instances::kListed && size_t(blockIdx.x) * THREADS >= n) return false;
    const size_t idx = size_t(blockIdx.x) * THREADS + threadIdx.x;
    if (idx >= n) return false;
    const uint32_t k = uint32_t(idx / per), item = uint32_t(idx - size_t(k) * per);
    const Lane ln = sel.lane(k, used);
    it = {ln, item, Instances::kListed ? size_t(ln.row) * per + item : idx};
    return !Instances::kListed || ln.live;          // (every instance: k < used follows from idx < n)
}

// the launch lane_item expects: ceil(cells * per / THREADS) workgroups, none for an empty call
template <uint32_t THREADS, class Kernel, class... Args>
hipError_t launch_lane_items(Kernel kernel, uint32_t cells, uint32_t per, hipStream_t stream, const Args &...args) {
    const size_t n = size_t(cells) * per;
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(kernel, dim3(uint32_t((n + THREADS - 1) / THREADS)), dim3(THREADS), 0, stream, args...);
    return hipGetLastError();
}

}  // namespace mmdx

// instance_list.hpp -- the device form of an mmdx_instance_select and which instance a lane of a select kernel works on: shared by
// the select kernels of rig_kernels.hip (mmdx_skeleton_solve_select, the bone side of the *_blend_*_time_select calls) and of
// kernels.hip (the morph side), so every select call reads a list the same way.
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
// cells: the instance count of a plain call, the list's capacity of a select call.  The plain kernels derive cell = row = instance
// themselves, as they always did; the select forms go through ListedInstances.
struct Lane {
    uint32_t cell, row;
    bool live;
};
struct ListedInstances {
    InstanceList l;
    // (the same address in every lane: one scalar load per wave, once per kernel)
    __device__ __forceinline__ uint32_t used(uint32_t cells) const { return l.count ? min(*l.count, cells) : cells; }
    __device__ __forceinline__ Lane lane(uint32_t k, uint32_t used) const {
        const bool in = k < used;
        const uint32_t id = in ? l.ids[k] : 0u;
        return {k, id, in && id < l.n_rows};
    }
};

}  // namespace mmdx

// socket_kernels.hpp -- launch interface between socket_api.cpp (mmdx_palette_sockets) and the gfx950 kernel of socket_kernels.hip
// (the row of a socket set's device table is socket_table.hpp's).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "instance_list.hpp"
#include "socket_table.hpp"

namespace mmdx {

constexpr uint32_t kSocketThreads = 256;            // lanes per workgroup when the call has that many rows; else its rows, rounded up to a wave
constexpr uint32_t kSocketMaxCells = 1u << 23;      // instances or list positions: cells * 4 rows stays far below 2^32 work-items

struct SocketLaunch {
    const float *palettes;       // device [ni][nb][16], 16-byte aligned
    const SocketEntry *table;    // device [ns]; every bone < nb
    float *out;                  // device [ns][ni][16], 16-byte aligned, disjoint from palettes
    uint32_t ni, nb, ns;
    bool any_offset;             // some entry has has_offset != 0
};

// Lanes per workgroup and workgroups per socket for `cells` instances or list positions (pure: also what the tests state shapes by)
inline uint32_t socket_threads(uint32_t cells) {
    const uint64_t rows = uint64_t(cells) * 4;
    return rows >= kSocketThreads ? kSocketThreads : uint32_t((rows + 63) / 64 * 64);
}
inline uint32_t socket_chunks(uint32_t cells) {
    const uint32_t t = socket_threads(cells);
    return uint32_t((uint64_t(cells) * 4 + t - 1) / t);
}

// One launch on `stream`.  ni, nb and ns are non-zero, ns <= kSocketMaxSockets.  list == nullptr: every instance, ni <= kSocketMaxCells;
// else `cells` list positions (0 < cells <= kSocketMaxCells), list->n_rows == ni.
hipError_t launch_palette_sockets(const SocketLaunch &p, const InstanceList *list, uint32_t cells, hipStream_t stream);

}  // namespace mmdx

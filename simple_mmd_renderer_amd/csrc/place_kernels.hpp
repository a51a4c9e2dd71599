// place_kernels.hpp -- launch interface between place_api.cpp (mmdx_palette_place) and the gfx950 kernel of place_kernels.hip.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace mmdx {

constexpr uint32_t kPlaceThreads = 256;          // lanes per workgroup when an instance has that many rows; else its rows, rounded up to a wave
constexpr uint32_t kPlaceMaxInstances = 1u << 23;   // grid x = instances: instances * kPlaceThreads stays below 2^32 work-items

struct PlaceLaunch {
    const float *palettes;     // device [ni][nb][16], 16-byte aligned
    const float *placements;   // device [ni][8] (pose form) or [ni][16] (matrix form)
    float *out;                // device [ni][nb][16], 16-byte aligned; == palettes or disjoint from it
    uint32_t ni, nb;
    bool matrix;
};

// Lanes per workgroup and workgroups per instance for a model of nb bones (pure: also what the tests state the shapes by)
inline uint32_t place_threads(uint32_t nb) {
    const uint64_t rows = uint64_t(nb) * 4;
    return rows >= kPlaceThreads ? kPlaceThreads : uint32_t((rows + 63) / 64 * 64);
}
inline uint32_t place_chunks(uint32_t nb) {
    const uint32_t t = place_threads(nb);
    return uint32_t((uint64_t(nb) * 4 + t - 1) / t);
}

// One launch on `stream`; ni and nb are non-zero, ni <= kPlaceMaxInstances, place_chunks(nb) <= 65535.
hipError_t launch_palette_place(const PlaceLaunch &p, hipStream_t stream);

}  // namespace mmdx

// pbounds_kernels.hpp -- launch interface between pbounds_api.cpp (mmdx_palette_bounds) and the gfx950 kernel of pbounds_kernels.hip.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace mmdx {

constexpr uint32_t kPBoundsThreads = 256;              // lanes per workgroup, both forms
constexpr uint32_t kPBoundsWaveRows = 64;              // tables of at most this many rows: one wave per instance, four instances per workgroup
constexpr uint32_t kPBoundsMaxInstances = 1u << 23;    // instances * kPBoundsThreads stays below 2^32 work-items
constexpr uint32_t kPBoundsRowFloats = 12;             // device table row: {lo xyz, bone as bits}, {hi xyz, 0}, {reach xyz, 0}: three 16-byte loads

struct PBoundsLaunch {
    const float *palettes;     // device [ni][nb][16], 16-byte aligned
    const float *table;        // device [n_boxes][kPBoundsRowFloats], 16-byte aligned; every bone < nb
    float *out;                // device [ni][6], 4-byte aligned
    uint32_t ni, nb, n_boxes;
    float eps, morph_scale, pos_scale;
};

// Waves per instance (1 or 4) and workgroups of a launch (pure: also what the tests state the shapes by)
inline uint32_t pbounds_waves_per_instance(uint32_t n_boxes) { return n_boxes <= kPBoundsWaveRows ? 1u : 4u; }
inline uint32_t pbounds_workgroups(uint32_t ni, uint32_t n_boxes) { return pbounds_waves_per_instance(n_boxes) == 1 ? (ni + 3) / 4 : ni; }

// One launch on `stream`; ni is non-zero and <= kPBoundsMaxInstances.  n_boxes == 0 writes NaN rows.
hipError_t launch_palette_bounds(const PBoundsLaunch &p, hipStream_t stream);

}  // namespace mmdx

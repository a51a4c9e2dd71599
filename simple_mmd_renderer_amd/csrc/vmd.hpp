// vmd.hpp -- glue between the VMD host code (vmd.cpp, no HIP) and the HIP side (api.cpp, kernels.hip).
#pragma once

#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/mmdx.h"

namespace mmdx {

struct MorphMotionHost {          // keyframes of every model morph, model-morph order
    uint32_t nm;
    const uint32_t *key_off;      // [nm+1]
    const uint32_t *frames;       // [nkeys] ascending inside a morph
    const float *weights;         // [nkeys]
    uint32_t nkeys;
};

struct MorphMotionDevice;         // the tables and scratch in device memory: defined, created on first use and deleted by api.cpp

const MorphMotionHost morph_motion_host(const mmdx_morph_motion_s *m);
MorphMotionDevice *&morph_motion_device(mmdx_morph_motion_s *m);
void morph_motion_release_device(MorphMotionDevice &d);   // api.cpp: frees the buffers and the object itself

struct VmdBoneTracks {            // views into a parsed motion, valid until mmdx_vmd_destroy
    const std::vector<std::string> *names;    // UTF-8, track order
    const std::vector<uint32_t> *off;         // [tracks+1] into keys
    const mmdx_vmd_bone_key *keys;            // sorted by frame inside a track
};
VmdBoneTracks vmd_bone_tracks(const mmdx_vmd_s *v);

// The argument checks the *_time entry points share beyond NULL / n_instances: flag bits outside `allowed`, and NaN in
// host-resident times (size_t(NaN) is undefined behaviour in the reference; device times that are NaN take the first key).
mmdx_status check_time_args(const double *times, uint32_t n_instances, uint32_t flags, uint32_t allowed);

struct MorphTrackParams {
    const uint32_t *key_off, *key_frames;
    const float *key_weights;
    const uint32_t *frames;       // [ni] frame number of every instance
    float *out;                   // [ni][nm]
    uint32_t nm, ni;
    const double *times;          // [ni] seconds instead of frames (MotionPlayer::SeekTime), or nullptr
};

}  // namespace mmdx

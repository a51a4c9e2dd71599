// api_internal.hpp -- what api.cpp (the drop-in boundary, include/mmdx.h), bench_api.cpp (the measurement / A-B entry points,
// include/mmdx_bench.h) and the other files of calls on a model share: the model handle and the launch-shape overrides.  The host
// plumbing (error mapping, device buffer, call steps) is host_runtime.hpp.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdlib>
#include <string>
#include <thread>
#include <vector>

#include "../../include/mmdx.h"
#include "../../include/mmdx_bench.h"
#include "error.hpp"
#include "graph_pin.hpp"
#include "host_runtime.hpp"
#include "kernels.hpp"
#include "launch_shape.hpp"
#include "plan.hpp"
#include "rig.hpp"

namespace mmdx {

// The launch-shape overrides (launch_shape.hpp), as the environment sets them
LaunchOverrides read_launch_overrides();
LaunchOverrides &launch_overrides();
void reload_cull_overrides();       // MMDX_CULL_FORM / MMDX_CULL_CHUNK (cull_api.cpp), re-read with the launch-shape overrides
int env_int(const char *name, int dflt);
std::vector<float> bone_box_device_table(const Plan &p);   // pbounds_api.cpp: the plan's bone boxes in the kernel's row layout
// average ms of `iters` store-pattern launches on the default stream (after one warm-up launch); bench_api.cpp
hipError_t time_store_pattern(void *a, void *b, uint32_t nv, uint32_t ni, uint32_t bpva, uint32_t bpvb, int iters, float *avg_ms,
                              uint32_t pitch = 0);   // pitch: vertices from one instance to the next (0 = nv)
// rig_api.cpp, the owner of the motion-set handle, for mmdx_animator_root_motion (anim_api.cpp): what a set says about its bone
// side without the device ...
struct SetBoneSide {
    bool has_bones;
    uint32_t n_clips, nb;
    int device;                                 // where its tables are, -1 = nowhere yet
};
SetBoneSide motion_set_bone_side(const mmdx_motion_set_s *set);
// ... and its bone tables on `device` as a parameter block (clock and output fields empty), the set noted in `model`'s recording
mmdx_status motion_set_bone_tables(mmdx_motion_set_s *set, mmdx_model_t model, int device, BoneTrackParams *p);
// rig_api.cpp, the owner of the skeleton handle, for mmdx_spring_set_create (spring_api.cpp): what a spring set copies of a
// skeleton at creation, without the device
struct SkeletonRest {
    uint32_t nb;
    const int32_t *parent;                      // [nb] as mmdx_skeleton_desc.parent gave it; the skeleton's own
    const float *neg_rest;                      // [nb][4] -rest position
};
SkeletonRest skeleton_rest(const mmdx_skeleton_s *s);
// socket_api.cpp, the owner of the socket-set handle, for mmdx_model_destroy: the sets created on `m` refuse every call from here on
void socket_sets_forget_model(mmdx_model_s *m);

}  // namespace mmdx

struct mmdx_model_s {
    mmdx::Plan plan;
    int device = -1;  // -1: host-only
    hipStream_t own_stream = nullptr, stream = nullptr;
    hipEvent_t ev_t0 = nullptr, ev_t1 = nullptr;
    hipEvent_t ev_switch = nullptr;   // mmdx_model_set_stream: orders the new stream behind the old one (no timing)
    // per-call kernel timing (mmdx_profile_*): event quadruples {skin0, skin1, morph0, morph1},
    // recorded on the launch stream without any host sync; read back by mmdx_profile_collect
    std::vector<hipEvent_t> prof_events;
    std::vector<uint8_t> prof_has_morph;
    size_t prof_calls = 0;
    bool profile = false;
    uint32_t profile_stride = 1, prof_seen = 0;     // time every profile_stride-th call
    uint64_t device_bytes = 0;
    // static streams
    mmdx::DevBuf tiles, spos, snrm, suv, perm, skin1, skin2_ids, skin2_w, skin4_ids, skin4_w, bone_list,
        ell, entries, slot_top, chain_off, chain_rate;
    // per-call scratch (grown on demand, reused)
    mmdx::DevBuf pal, rates, wslot, morphed, out_a, out_b;
    mmdx::DevBuf seen;              // RatesSeen record (kernels.hpp): the rates `morphed` was last computed from, device side
    mmdx::DevBuf bnd;               // mmdx_deform_batched_bounds: partial bounds, then (host bounds) the [NI][6] result
    mmdx::DevBuf sel;               // mmdx_deform_batched_select with a host list: {live count, ids[n_ids]}
    std::vector<uint32_t> sel_host; // ... and its image on the host, the source of the upload
    mmdx::DevBuf cull;              // mmdx_cull_bounds in two launches: per-chunk, per-level counts
    mmdx::DevBuf place_in, place_w, place_out;   // mmdx_palette_place with host operands: palettes, placements, result
    mmdx::DevBuf bone_boxes;                     // static: the bone-box table of mmdx_palette_bounds (pbounds_kernels.hpp row layout)
    mmdx::DevBuf pbounds_in, pbounds_out;        // mmdx_palette_bounds with host operands: palettes, result
    mmdx::DevBuf blend_a, blend_b, blend_p, blend_out;   // mmdx_pose_blend / mmdx_rate_blend / mmdx_pose_add / mmdx_rate_add with host
                                                         // operands: A, B, {weights, mask ids, masks, ref ids, refs}, result
    mmdx::DevBuf blend_sel;                      // ... with a host list: {live count, ids[live]}
    std::vector<uint32_t> blend_sel_host;        // ... its source, alive until the copy has left it
    bool morphed_valid = false;     // `morphed` holds the result of a shared morph pass (MMDX_MORPH_UNCHANGED)
    std::vector<float> host_rates;  // ... and the host's copy of those rates when they came from host memory
    bool host_rates_valid = false;
    uint32_t host_skips = 0;        // crowd calls whose morph pass the host-side comparison skipped (mmdx_debug_morph_pass_stats)
    bool capturing = false;         // between mmdx_graph_begin and mmdx_graph_end: the stream records
    std::thread::id capture_thread; // ... begun on this thread (thread-local capture mode: it must end there too)
    mmdx::GraphPin pin;                   // graphs that hold addresses of this model's scratch buffers
    std::vector<mmdx::GraphPin *> rec_pins;   // handles that took part in the recording in progress (incl. this model)
    bool rec_poisoned = false;          // one of them was destroyed before mmdx_graph_end: the recording cannot become a graph
    bool last_write_through = false;          // store flavour of the last crowd launch (mmdx_debug_last_store_policy)
    mmdx_debug_launch_shape last_shape{};     // ... and the rest of its shape (mmdx_debug_last_launch_shape); struct_size unused
    mmdx_model_s() {
        for (mmdx::DevBuf *b : {&pal, &rates, &wslot, &morphed, &out_a, &out_b, &bnd, &sel, &cull, &place_in, &place_w, &place_out, &pbounds_in,
                                 &pbounds_out, &blend_a, &blend_b, &blend_p, &blend_out, &blend_sel}) b->pin = &pin;
    }
    // page-locked bounce buffer for small outputs bound for pageable host memory (see mmdx_deform_batched)
    void *bounce = nullptr, *bounce_dev = nullptr;  // host address, device-side address
    size_t bounce_bytes = 0;
    void *bounce_in = nullptr;                     // the same for small pageable inputs (palette, rates)
};

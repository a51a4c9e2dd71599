// launch_shape.hpp -- the shape of one deform launch (threads, store flavour, group size, LDS layout, which kernel), decided from
// values alone: no handle, no HIP call, no environment.  Pure C++17 like plan.cpp, so every heuristic in it can be swept on a machine
// without a GPU (tests/test_launch_shape.py).
#pragma once

#include <cstddef>
#include <cstdint>
#include <string>

#include "lds_layout.hpp"
#include "plan.hpp"

namespace mmdx {

// Launch-shape overrides for A/B runs (tools/): read ONCE, at the first deform call of the process -- the
// per-frame call has a budget of a few microseconds and getenv walks the whole environment.
struct LaunchOverrides {
    int interleave, threads, lds_target, group, placement_log, placement_park;
    int frame_kernel;   // MMDX_FRAME_KERNEL: 0 = a single frame always runs the tile kernel, 1 = models of fewer than 256 tiles run the
                        // frame kernel (default), 2 = always (A/B); MMDX_FRAME_THREADS: 128 / 256 lanes per workgroup
    int frame_threads;
    int shared_fused;   // MMDX_SHARED_FUSED: crowds with a shared facial state gather the morphs inside the deform kernel: 0 never,
                        // 1 up to 8 instances (default), 2 always (A/B, tests)
    int store_wt;       // MMDX_STORE_WT: 0 / 1 force cached / write-through stores where the caller gave no hint (A/B); -1 default
    int morph_autoskip; // MMDX_MORPH_AUTOSKIP: 0 turns the automatic "shared rates unchanged" detection off (A/B); 1 default
    int fused_pack;     // MMDX_FUSED_PACK: 0 = per-instance morph weights run deform_kernel<512, ., kMorphFused4> (default),
                        // 1 = pack_kernel (round 4's higher-occupancy shape: measured slower, kept for the A/B)
    int stagger;        // MMDX_STAGGER: start offset between the workgroups of a CU, in units of 64 cycles per residency slot (A/B)
    int select_interleave;   // MMDX_SELECT_INTERLEAVE: 1 = select launches deal list positions interleaved over the workgroups like the
                             // plain crowd call (default, measured faster); 0 = blocked (A/B)
};

// What of one mmdx_deform_batched* call the launch shape depends on
struct DeformCall {
    uint32_t layout, ni;
    uint32_t nwork;             // instances the launch is sized for: the list's capacity of a select call, else ni
    uint32_t flags;             // mmdx_deform_args.flags (the MMDX_OUT_STORES_* hints are read)
    int morph;                  // kMorph*
    bool bounds, select;
    bool out_dev;               // outputs in device memory
    bool out_host_mapped;       // ... or written by the kernel into page-locked host memory (the caller's, or the handle's bounce buffer)
    size_t out_bytes;           // both output arrays
};

struct LaunchShape {
    enum Kernel { kNone, kDeform, kPack, kFrame };      // kNone: a select call with an empty list launches no deform kernel
    Kernel kernel;
    int threads;                // as passed to launch_deform (kDeform)
    uint32_t group;             // instances per workgroup
    size_t lds;                 // dynamic LDS of the chosen kernel
    uint32_t stage_off, w_off, mp_off, bounds_off;      // byte offsets inside it (DeformParams)
    uint32_t bounds_units;      // partial bounds per instance (deform_bounds_units); 0 without bounds
    uint32_t stagger, slots_per_cu;
    bool write_through;
};

// MMDX_OK and `shape`, or MMDX_ERR_UNSUPPORTED and `err` when a workgroup would need more LDS than a CU has.
mmdx_status plan_deform_launch(const Plan &p, const DeformCall &c, const LaunchOverrides &ov, LaunchShape &shape, std::string &err);

}  // namespace mmdx

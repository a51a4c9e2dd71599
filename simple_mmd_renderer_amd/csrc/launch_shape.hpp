// launch_shape.hpp -- the shape of one deform launch (threads, store flavour, group size, LDS layout, which kernel), decided from
// values alone: no handle, no HIP call, no environment.  Pure C++17 like plan.cpp, so every heuristic in it can be swept on a machine
// without a GPU (tests/test_launch_shape.py).  Below it, the morph step of the same call (plan_morph_pass, tests/test_morph_plan.py).
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

// ---- the morph step of the same call: which morph mode (DeformCall::morph), which launches in front of the deform kernel, and what
// the handle knows afterwards about the positions it keeps.  A handle keeps ONE buffer of morphed positions (`morphed`), and two
// records of the rates it was computed from: the host's (MorphRecord) and the device's (RatesSeen, kernels.hpp).  The rules
// (tests/test_morph_plan.py sweeps them and proves the records sound over every short sequence of calls):
//   * morph == kMorphNone iff the model has no slot; per-instance rates are kMorphFused4 and never touch `morphed` or a record;
//   * a single frame (ni == 1) is kMorphFused1, gathers in its kernel and is never handed `morphed` (withhold_morphed);
//   * a crowd with one set of rates either gathers in the deform kernel (kMorphFused1, pass kGather) or reads `morphed`
//     (kMorphShared); kMorphShared with pass kNoPass reads what an earlier call left there, which takes the caller's word
//     (MMDX_MORPH_UNCHANGED, refused unless morphed_valid) or the host's comparison (host_skip);
//   * what a pass leaves behind:   pass           `morphed`        device record                host record      morphed_valid
//                                  kNoPass        kept             untouched                    kept             kept
//                                  kFlatten       kept             untouched                    kept             kept
//                                  kGather, ni=1  kept             untouched                    kept             kept
//                                  kGather, crowd the call's       cleared by the deform kernel void             true
//                                  kFusedApply    the call's       compared, then = the call's  stored* or void  true
//                                                                  (untouched without autoskip)
//                                  kFlattenApply  the call's       cleared by a memset          stored* or void  true
//     (* stored: the rates came from host memory and the crowd is past the small-crowd size; the copy is what later host-rates
//     calls are compared with);
//   * the host record is only ever trusted together with morphed_valid, with autoskip on, and by a call that would store it.
struct MorphRecord {
    bool morphed_valid;         // `morphed` holds the result of a crowd's morph pass or gather
    bool host_rates_valid;      // ... and host_rates are the rates it was computed from
    const float *host_rates;
    size_t n_host_rates;
};

struct MorphCall {
    uint32_t ns, nm;            // the model's slots and morphs
    uint32_t ni, flags;         // mmdx_deform_args (MMDX_WEIGHTS_SHARED, MMDX_MORPH_UNCHANGED and MMDX_WEIGHTS_ON_DEVICE are read)
    bool select;                // a select call ...
    uint32_t n_ids;             // ... and its list's capacity
    int shared_fused, morph_autoskip;   // LaunchOverrides
    const float *rates;         // mmdx_deform_args.morph_weights; read (nm floats) only without MMDX_WEIGHTS_ON_DEVICE
};

struct MorphPlan {
    enum Pass {
        kNoPass,                // nothing in front of the deform kernel
        kFusedApply,            // morph_apply_kernel with the flatten fused in: one launch
        kFlattenApply,          // flatten, morph_apply_kernel, and a memset of the device record's valid word
        kFlatten,               // flatten alone: the slot weights of per-instance rates
        kGather                 // none either: the deform kernel flattens and gathers (DeformParams::fused_rates)
    };
    enum Seen { kSeenUntouched, kSeenCompared, kSeenClearedByDeform, kSeenClearedByMemset };
    enum HostRates { kRatesKept, kRatesStored, kRatesVoid };
    int morph;                  // kMorph*
    Pass pass;
    bool upload;                // the call's rates go to the handle's scratch first (niw rows of nm)
    uint32_t niw;               // rows of rates: 1 shared; per-instance the instances, or the list positions of a select call
    uint32_t wslot_rows;        // rows of ns + 1 slot weights the scratch must hold (niw, in whole quads for kMorphFused4)
    bool quad;                  // flatten writes instance quads (kMorphFused4)
    bool select_rows;           // flatten takes row j from rates[sel_ids[j]]
    Seen seen;                  // the device record
    bool withhold_morphed;      // dp.morphed = nullptr
    bool host_skip;             // kNoPass because the host found the rates equal to the recorded ones (counted in host_skips)
    bool morphed_valid;         // the handle's record after the call ...
    HostRates host_rates;       // ... and its copy of the rates: as before, = the call's, or void
};

// MMDX_OK and `plan`, or MMDX_ERR_INVALID_ARGUMENT and `err`: MMDX_MORPH_UNCHANGED on a crowd whose handle holds no positions.
mmdx_status plan_morph_pass(const MorphCall &c, const MorphRecord &rec, MorphPlan &plan, std::string &err);

}  // namespace mmdx

// kernels.hpp -- launch interface between the C-ABI host code (api.cpp) and the gfx950 kernels.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "instance_list.hpp"
#include "lds_layout.hpp"
#include "plan.hpp"
#include "vmd.hpp"

namespace mmdx {

struct DeformParams {
    // static streams (HBM, uploaded once by mmdx_model_create)
    const TileHdr *tiles;
    const void *spos;            // f32 [NV][3]  |  f16 mode: u16 [NV][4]
    const float *snrm;           // [NV][3]
    const float *suv;            // [NV][2]
    const uint16_t *perm;        // [NV]
    const uint16_t *skin1;
    const uint32_t *skin2_ids;
    const float *skin2_w;
    const uint2 *skin4_ids;
    const float4 *skin4_w;
    const uint32_t *bone_list;
    const uint2 *ell;            // [ntiles*8] {first entry, padded row length} per 64-slot slice
    const void *entries;         // float4 [NE]  |  f16 mode: uint2 [NE]
    // per call
    const float *palettes;       // [NI][NB][16] device
    const float *wslot;          // rows of NS+1 weights (column NS = table padding, always 0):
                                 // kMorphFused1: f32 [NI][NS+1]
                                 // kMorphFused4: float4 [ceil(NI/4)][NS+1] (instance quads)
                                 // morph_apply : f32 [NS+1]
    float *morphed;              // f32 [NV][3] sorted order (kMorphShared)
    // kMorphFused1 with fused_rates != nullptr: slot weights are evaluated inside the kernel from the
    // raw morph rates [NI][NM] (saves the flatten launch of a single-model frame)
    const float *fused_rates;
    const uint32_t *slot_top, *chain_off;
    const float *chain_rate;
    uint32_t nm;
    void *out_a;
    void *out_b;
    // pitch: output vertices from one instance to the next (MMDX_OUT_PITCHED; = nv for dense outputs).  It sits where nv sat
    // before it existed, and nv (read by the morph pass only) at the end: the kernels that write outputs see the same
    // kernel-argument layout as the dense-only build and compile to the same registers
    uint32_t pitch, nb, ns, ni;
    uint32_t group;              // instances per workgroup (multiple of 4 for kMorphFused4)
    uint32_t ntiles, ngroups, rem_per_xcd;  // filled by launch_deform (XCD-aware work mapping)
    uint32_t pal_stride;         // float4 per instance in LDS (= max_tile_bones * 3)
    uint32_t stage_off;          // byte offsets inside dynamic LDS
    uint32_t w_off;
    uint32_t mp_off;             // pack_kernel: the coordinate / position-image regions
    float pos_scale;
    uint32_t out_aligned;        // out_a and out_b are 16-byte aligned
    uint32_t finite_offsets;     // every vertex-morph offset is finite (branch-free morph skip is exact)
    uint32_t interleave;         // crowd modes: instance = g*ngroups + grp instead of grp*group + g
    uint32_t tile_order;         // MMDX_CREATE_TILE_ORDER: outputs in the engine's vertex order (tile-local class sort), stored straight
                                 // from registers -- no LDS image, no per-instance barrier
    uint32_t write_through;      // launch the write-through flavour of the copy-out (launch_shape.cpp sets it only where deform_has_write_through())
    uint32_t stagger;            // per-instance-morph kernels: first-round workgroups of residency slot k start k * stagger * 64 cycles late,
                                 // so that the workgroups sharing a CU are not all in their walk (or all in their stores) at once
    uint32_t slots_per_cu;       // ... with this many workgroups resident per CU
    unsigned long long *stamps;  // diagnostic builds of pack_kernel only (PK_STAMPS): per-wave cycle counters; nullptr in the product
    uint32_t *morph_seen;        // kMorphFused1 crowds: the handle's RatesSeen record; a launch that overwrites `morphed` clears its
                                 // valid word (the record no longer describes what `morphed` holds)
    uint32_t nv;                 // vertices of the model
    // mmdx_deform_batched_bounds (behind every field the other kernels read, so their argument layout does not move):
    uint32_t bounds_off;         // byte offset in dynamic LDS of the combine words (kBoundsLdsBytes; image path only)
    float *bounds;               // partial bounds, 6 floats per deform_bounds_units(); nullptr = the plain deform_kernel
    // mmdx_deform_batched_select (again behind everything the other kernels read): the SELECT flavour of deform_kernel takes its
    // instances from a list in device memory.  `ni` stays the extent of the call's arrays (ids >= ni are skipped); the grid is
    // sized from sel_n; partial bounds are indexed by list position.
    const uint32_t *sel_ids;     // [sel_n] instance indices; nullptr = not a select launch
    const uint32_t *sel_count;   // live prefix of sel_ids (clamped to sel_n); nullptr = all of them
    uint32_t sel_n;
    uint32_t sel_interleave;     // list position = g*ngroups + grp (default) instead of grp*group + g; never with kMorphFused4
};

// out[i][6] = bounds of instance i from the partials ([ni][units][6]), on `stream` behind the bounds launch
hipError_t launch_bounds_reduce(const float *partials, uint32_t units, uint32_t ni, float *out, hipStream_t stream);
// select launches: partials are [sel_n][units][6] by list position; block j writes out[ids[j]] when j is live and ids[j] < ni
hipError_t launch_bounds_reduce_select(const float *partials, uint32_t units, uint32_t ni, float *out, const uint32_t *ids,
                                       const uint32_t *count, uint32_t n_ids, hipStream_t stream);

// Device-side record of the morph rates the `morphed` buffer of a handle was last computed from (shared morph pass of a crowd):
// morph_apply_kernel compares the call's rates with it, bit for bit, and skips its walk when they are equal -- the automatic form of
// MMDX_MORPH_UNCHANGED for rates that live in device memory, where the host cannot look.  u32 words:
enum : uint32_t { kSeenValid = 0, kSeenTicket = 1, kSeenWalks = 2, kSeenSkips = 3, kSeenRates = 4 };   // then NM rate bit patterns

struct FlattenParams {
    const float *rates;          // [NIw][NM] device
    const uint32_t *slot_top, *chain_off;
    const float *chain_rate;
    float *out;
    uint32_t nm, ns, niw;
    uint32_t quad;               // 1: write float4 [ceil(NIw/4)][NS] instance quads (pad lanes = 0)
    uint32_t *seen;              // morph_apply with the flatten fused in: the handle's RatesSeen record (nullptr: always walk)
    // select launches (behind everything the other kernels read; ids == nullptr: not one): row j of the output comes from
    // rates[list.ids[j]]; rows behind the live count and rows whose id is no row of the rates are written as zeros.  niw = sel_n then.
    InstanceList list;
};

// One variant of deform_kernel: what pick() (kernels.hip) chooses an instantiation by.
struct DeformVariant {
    int threads, layout, morph;  // threads 256 / 512; morph: kMorphNone .. kMorphFused4
    bool f16;
    bool tile;                   // outputs in the engine's vertex order (MMDX_CREATE_TILE_ORDER): the direct-store variants
    bool wt;                     // write-through stores; exists where deform_has_write_through(), every other shape keeps its nt stores
    bool bounds, select;         // the BOUNDS / SELECT flavours (mmdx_deform_batched_bounds / _select): every shape, nt stores only
};

// The launch functions of one build of the kernels: kernels.hip as it stands (bit-exact), or compiled a second time with multiply-add
// contraction allowed (kernels_fast.hip, MMDX_CREATE_FAST_MATH models).
struct KernelSet {
    // LDS offsets of p and lds_bytes: from the launch's LaunchShape (launch_shape.hpp)
    hipError_t (*launch_deform)(const DeformVariant &v, const DeformParams &p, uint32_t ntiles, size_t lds_bytes, hipStream_t stream);
    // One frame of one model (ni == 1, kMorphNone / kMorphFused1): latency-ordered kernel, a workgroup = `threads` (128 / 256) sorted
    // slots of a tile, direct stores.
    hipError_t (*launch_frame)(int threads, int layout, int morph, bool f16, const DeformParams &p, uint32_t ntiles, size_t lds_bytes,
                               hipStream_t stream);
    // Per-instance morph weights, packs of 4 instances, 512 threads (kernels.hip pack_kernel): SoA f32 and f16-position layouts, original
    // vertex order.  p.group a multiple of 4.
    hipError_t (*launch_pack)(int layout, bool f16, const DeformParams &p, uint32_t ntiles, size_t lds_bytes, hipStream_t stream);
    // `fused` != nullptr: evaluate the slot weights inside the kernel (ns <= kMaxFusedSlots), no flatten launch
    hipError_t (*launch_morph_apply)(bool f16, const DeformParams &p, const FlattenParams *fused, hipStream_t stream);
    hipError_t (*prepare)();     // raise the dynamic-LDS limit of every deform variant (once per device)
};
const KernelSet &kernels();         // kernels.hip
const KernelSet &kernels_fast();    // kernels_fast.hip
inline const KernelSet &kernel_set(bool fast) { return fast ? kernels_fast() : kernels(); }
// pitch: vertices from one instance's piece to the next (0 = nv)
hipError_t launch_pattern_fill(void *a, void *b, uint32_t nv, uint32_t ni, uint32_t bpva, uint32_t bpvb,
                               hipStream_t stream, uint32_t pitch = 0);
hipError_t launch_flatten(const FlattenParams &p, hipStream_t stream);
hipError_t launch_morph_track_eval(const MorphTrackParams &t, hipStream_t stream);
// a motion set's morph side: t holds the concatenated tables, clips[ni] (device) the clip of every instance; ids >= n_clips give rate 0
hipError_t launch_morph_track_eval_set(const MorphTrackParams &t, const uint32_t *clips, uint32_t n_clips, hipStream_t stream);
struct BlendOperands;
// the cross-fade between two clips of a set (motion_blend.hpp), morph side: rates of clip a at time a and clip b at time b, blended
hipError_t launch_morph_track_blend_set(const MorphTrackParams &t, const BlendOperands &o, hipStream_t stream);
// mmdx_motion_set_blend_morphs_time_select: the same for the listed instances (instance_list.hpp); t.ni = the list's capacity,
// operand rows and rate rows addressed by id
hipError_t launch_morph_track_blend_set_select(const MorphTrackParams &t, const BlendOperands &o, const InstanceList &list,
                                               hipStream_t stream);
hipError_t launch_copy(void *dst, const void *src, size_t bytes, hipStream_t stream);
hipError_t launch_fill(void *dst, size_t bytes, hipStream_t stream);

}  // namespace mmdx

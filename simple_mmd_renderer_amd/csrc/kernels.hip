// kernels.hip -- gfx950 (MI355X / CDNA4) kernels of the deformation path.  Hand-written HIP; built
// with -ffp-contract=off so that every f32 operation is the reference's operation, in the
// reference's order (no FMA contraction): results are bit-identical to libmmd's CPU path.
//
// Replaces (reference file:line, L/ = 3rd_party/libmmd/include/mmd/):
//   morph accumulate   L/motion/poser_impl.inl:328-346, :362-365, :384-386  -> sliced-ELL walks (kernels_morph_walk.inl)
//   Poser::Deform      L/motion/poser_impl.inl:396-437                      -> deform_kernel / frame_kernel / pack_kernel
//   Lerp / M*s / M+M   L/util/math_impl.inl:924-963, :1004-1023, :1241-1259  -> blend2 / mul_add / add_mul
//   transform / rotate L/util/math_impl.inl:1032-1045                        -> xform_pos / xform_nrm
//   32-byte repack     main.cpp:50-54, :838-859                              -> MMDX_OUT_VERTEX32
//
// This file is the translation unit: the preamble, the kernel families it includes (one file each, in the order the code object
// has always had them), the dispatch from a call's variant to an instantiation, and the launch functions.
//
// What the deform kernels share: a workgroup is one 512-vertex TILE x a GROUP of instances.  The tile's vertices are pre-sorted by
// deform class (plan.cpp), so wavefronts are class-uniform and skip the other classes' code.
//   * the group's bone palettes are staged in LDS, only the bones the tile uses, transposed to
//     3 x float4 columns per bone (the 4th matrix column is never read by the path);
//   * static per-vertex data (position, normal, class data) is loaded ONCE into registers and reused
//     for every instance of the group -- static streams cost HBM/L2 traffic once per group;
//   * each instance's results are scattered to an LDS image of the tile's output range (undoing the
//     class sort), then written out cooperatively as 16-byte coalesced stores.
//   HBM-bound: ~24-32 B written per vertex-instance against ~100 VALU ops; no MFMA (gather of small
//   mat x vec, <= 3 flop/B).
// The forms of that shape:
//   deform_kernel   the crowd kernel: 512 threads (one sorted slot per lane, 8 wave64) or 256 (two slots per lane); morph mode
//                   none / shared (positions morphed by morph_apply_kernel) / one set of rates walked in the kernel / per-instance
//                   rates; tile-order outputs (direct stores: no image, no barrier); write-through stores (SoA f32 crowd only);
//                   with per-instance bounds; with the instances taken from a device list (select)
//   pack_kernel     per-instance rates in packs of 4, walk and skinning in separate phases (opt-in, MMDX_FUSED_PACK=1)
//   frame_kernel    one frame of one model: a workgroup is a part of a tile, 128 or 256 threads, direct stores
// and beside them the shared morph pass and flatten, the VMD morph-track kernels, the bounds reduction and bench.py's copy / fill /
// store-pattern kernels.
#include "clip_source.hpp"
#include "instance_list.hpp"
#include "kernels.hpp"

#include <type_traits>
#ifdef PK_STAMPS
#include <algorithm>
#include <cstdio>
#include <vector>
#endif

// MMDX_FAST_MATH (kernels_fast.hip includes this file with it defined): the SAME kernels with multiply-add contraction allowed
// (v_fma_f32 / v_pk_fma_f32) for models created with MMDX_CREATE_FAST_MATH -- results within a stated tolerance of the
// reference's instead of bit-identical (include/mmdx.h).  Only the deform / frame / pack / shared-morph kernels exist in that
// build, under *_fast launch names; everything else in this file is compiled once, uncontracted.
#ifdef MMDX_FAST_MATH
#pragma clang fp contract(fast)
#define MMDX_K(name) name##_fast
#else
#define MMDX_K(name) name
#endif

// Timing-diagnostic build knobs (PK_SKIP_WALK, PK_SKIP_SKIN, FUSED4_SKIP_WALK: a kernel without one of its halves -- WRONG results by
// design; PK_STAMPS: in-kernel cycle stamps): only together with MMDX_DIAGNOSTIC_BUILD, and never the product -- the build's flags
// are part of the source stamp (build.py source_sha), so bench.py / smoke() refuse such a library unless it is loaded explicitly
// through MMDX_LIB by a tool.
#if (defined(PK_SKIP_WALK) || defined(PK_SKIP_SKIN) || defined(FUSED4_SKIP_WALK) || defined(PK_STAMPS)) && !defined(MMDX_DIAGNOSTIC_BUILD)
#error "PK_SKIP_* / FUSED4_SKIP_WALK / PK_STAMPS are timing diagnostics (wrong results): add MMDX_DIAGNOSTIC_BUILD to MMDX_BUILD_DEFS"
#endif

namespace mmdx {
namespace {

constexpr int kThreads = 256;                     // workgroup of the one-thread-per-item kernels (morph pass, flatten, tracks, bench)
using KernelFn = void (*)(const DeformParams);

#include "kernels_store.inl"            // store16 / store3 / store_elem, copy_out2, copy_out_fast
#include "kernels_skin_math.inl"        // h2f / f2h, M12 and its blends, xform_*, Slot, skin_matrix
#include "kernels_morph_walk.inl"       // row_prefetch / row_consume / for_row, walk_rolling, fused4_walk, slot_weight
#include "kernels_setup.inl"            // map_workgroup and xcd_grid, load_slot, stage_palettes, setup_fused1, stagger_start
#include "kernels_bounds.inl"           // bound_op ... wave_bounds6, BoundsOut
#include "kernels_deform.inl"           // skin_instance, deform_kernel
#include "kernels_pack.inl"             // pack_kernel, launch_pack
#include "kernels_frame.inl"            // frame_kernel
#include "kernels_morph_pass.inl"       // morph_apply_kernel; flatten_kernel, flatten_select_kernel (bit-exact build only)
#ifndef MMDX_FAST_MATH
#include "kernels_morph_track.inl"      // morph_track_*_kernel
#include "kernels_bench.inl"            // copy_kernel, fill_kernel, pattern_fill_kernel
#include "kernels_bounds_reduce.inl"    // bounds_reduce_kernel, bounds_reduce_select_kernel
#endif

// ---- from a call's variant to an instantiation ------------------------------------------------------------------------------------
template <int THREADS, int LAYOUT, bool F16, bool TILE, bool BOUNDS, bool SELECT>
KernelFn pick_morph(int morph) {
    constexpr int kSel = SELECT ? int(kMorphSelect) : 0;
    switch (morph) {
    case kMorphNone: return deform_kernel<THREADS, LAYOUT, kMorphNone | kSel, F16, TILE, false, BOUNDS>;
    case kMorphShared: return deform_kernel<THREADS, LAYOUT, kMorphShared | kSel, F16, TILE, false, BOUNDS>;
    case kMorphFused1: return deform_kernel<THREADS, LAYOUT, kMorphFused1 | kSel, F16, TILE, false, BOUNDS>;
    default: return deform_kernel<THREADS, LAYOUT, kMorphFused4 | kSel, F16, TILE, false, BOUNDS>;
    }
}

template <int THREADS, bool TILE, bool BOUNDS, bool SELECT>
KernelFn pick_t(const DeformVariant &v) {
    if (v.f16) return v.layout == MMDX_OUT_SOA_POS16 ? pick_morph<THREADS, MMDX_OUT_SOA_POS16, true, TILE, BOUNDS, SELECT>(v.morph) : nullptr;
    if (v.layout == MMDX_OUT_SOA) return pick_morph<THREADS, MMDX_OUT_SOA, false, TILE, BOUNDS, SELECT>(v.morph);
    if (v.layout == MMDX_OUT_VERTEX32) return pick_morph<THREADS, MMDX_OUT_VERTEX32, false, TILE, BOUNDS, SELECT>(v.morph);
    return nullptr;
}

template <bool BOUNDS, bool SELECT>
KernelFn pick_b(const DeformVariant &v) {
#if MMDX_TILE >= 512
    if (v.threads != 256) return v.tile ? pick_t<512, true, BOUNDS, SELECT>(v) : pick_t<512, false, BOUNDS, SELECT>(v);
#endif
    return v.tile ? pick_t<256, true, BOUNDS, SELECT>(v) : pick_t<256, false, BOUNDS, SELECT>(v);
}

// The instantiation of deform_kernel for a variant (DeformVariant, kernels.hpp); nullptr: no such layout.  The write-through
// flavour is instantiated where it was measured to pay -- the SoA f32 crowd kernels (deform_has_write_through()); the bounds and
// select flavours have nt stores only.
KernelFn pick(const DeformVariant &v) {
    if (v.select) return v.bounds ? pick_b<true, true>(v) : pick_b<false, true>(v);
    if (v.bounds) return pick_b<true, false>(v);
    if (v.wt && deform_has_write_through(v.threads, v.layout, v.morph, v.f16, v.tile))
        return v.morph == kMorphNone ? deform_kernel<256, MMDX_OUT_SOA, kMorphNone, false, false, true>
                                     : deform_kernel<256, MMDX_OUT_SOA, kMorphShared, false, false, true>;
    return pick_b<false, false>(v);
}

constexpr int kLayouts[][2] = {{MMDX_OUT_SOA, 0}, {MMDX_OUT_VERTEX32, 0}, {MMDX_OUT_SOA_POS16, 1}};      // {layout, f16}

// fn(variant) for exactly the variants pick() has a kernel for, the two write-through ones included; stops at the first error
template <typename Fn>
hipError_t for_each_deform_variant(Fn fn) {
    for (int threads : {256, 512})
        for (const auto &l : kLayouts)
            for (int morph = kMorphNone; morph <= kMorphFused4; ++morph) {
                const bool f16 = l[1] != 0;
                for (int tile = 0; tile < 2; ++tile)
                    for (int bounds = 0; bounds < 2; ++bounds)
                        for (int select = 0; select < 2; ++select)
                            if (hipError_t e = fn(DeformVariant{threads, l[0], morph, f16, tile != 0, false, bounds != 0, select != 0});
                                e != hipSuccess)
                                return e;
                if (deform_has_write_through(threads, l[0], morph, f16, false))
                    if (hipError_t e = fn(DeformVariant{threads, l[0], morph, f16, false, true, false, false}); e != hipSuccess) return e;
            }
    return hipSuccess;
}

template <int THREADS, int LAYOUT, bool F16>
KernelFn pick_frame_morph(int morph) {
    return morph == kMorphNone ? frame_kernel<THREADS, LAYOUT, kMorphNone, F16> : frame_kernel<THREADS, LAYOUT, kMorphFused1, F16>;
}
KernelFn pick_frame(int threads, int layout, int morph, bool f16) {
    if (morph != kMorphNone && morph != kMorphFused1) return nullptr;
    if (f16) {
        if (layout != MMDX_OUT_SOA_POS16) return nullptr;
        return threads == 128 ? pick_frame_morph<128, MMDX_OUT_SOA_POS16, true>(morph) : pick_frame_morph<256, MMDX_OUT_SOA_POS16, true>(morph);
    }
    if (layout == MMDX_OUT_SOA)
        return threads == 128 ? pick_frame_morph<128, MMDX_OUT_SOA, false>(morph) : pick_frame_morph<256, MMDX_OUT_SOA, false>(morph);
    if (layout == MMDX_OUT_VERTEX32)
        return threads == 128 ? pick_frame_morph<128, MMDX_OUT_VERTEX32, false>(morph) : pick_frame_morph<256, MMDX_OUT_VERTEX32, false>(morph);
    return nullptr;
}

// fn(threads, layout, morph, f16) for exactly the variants pick_frame() has a kernel for; stops at the first error
template <typename Fn>
hipError_t for_each_frame_variant(Fn fn) {
    for (int threads : {128, 256})
        for (const auto &l : kLayouts)
            for (int morph : {int(kMorphNone), int(kMorphFused1)})
                if (hipError_t e = fn(threads, l[0], morph, l[1] != 0); e != hipSuccess) return e;
    return hipSuccess;
}

KernelFn pick_pack(int layout, bool f16, bool finite) {
    if (f16) {
        if (layout != MMDX_OUT_SOA_POS16) return nullptr;
        return finite ? pack_kernel<MMDX_OUT_SOA_POS16, true, true> : pack_kernel<MMDX_OUT_SOA_POS16, true, false>;
    }
    if (layout != MMDX_OUT_SOA) return nullptr;
    return finite ? pack_kernel<MMDX_OUT_SOA, false, true> : pack_kernel<MMDX_OUT_SOA, false, false>;
}

// ---- the launch functions ---------------------------------------------------------------------------------------------------------
hipError_t raise_lds_limit(KernelFn fn) {
    return hipFuncSetAttribute(reinterpret_cast<const void *>(fn), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
}

hipError_t prepare_kernels() {
    for (int f16 = 0; f16 < 2; ++f16)
        for (int fin = 0; fin < 2; ++fin)
            if (hipError_t e = raise_lds_limit(pick_pack(f16 ? MMDX_OUT_SOA_POS16 : MMDX_OUT_SOA, f16 != 0, fin != 0)); e != hipSuccess) return e;
    if (hipError_t e = for_each_deform_variant([](const DeformVariant &v) { return raise_lds_limit(pick(v)); }); e != hipSuccess) return e;
    return for_each_frame_variant([](int threads, int layout, int morph, bool f16) { return raise_lds_limit(pick_frame(threads, layout, morph, f16)); });
}

hipError_t launch_deform(const DeformVariant &v, const DeformParams &p, uint32_t ntiles, size_t lds_bytes, hipStream_t stream) {
    if (v.select && p.sel_n == 0) return hipSuccess;       // an empty list: nothing to launch
    KernelFn fn = pick(v);
    if (!fn) return hipErrorInvalidValue;
    DeformParams q = p;
    const dim3 grid = xcd_grid(q, ntiles, v.select ? p.sel_n : p.ni);      // select: the grid covers the list's capacity
    hipLaunchKernelGGL(fn, grid, dim3((v.threads == 256 || kTileVerts < 512) ? 256 : 512), lds_bytes, stream, q);
    return hipGetLastError();
}

hipError_t launch_frame(int threads, int layout, int morph, bool f16, const DeformParams &p, uint32_t ntiles, size_t lds_bytes,
                        hipStream_t stream) {
    threads = threads == 128 ? 128 : 256;
    KernelFn fn = pick_frame(threads, layout, morph, f16);
    if (!fn) return hipErrorInvalidValue;
    hipLaunchKernelGGL(fn, dim3(ntiles * (kTileVerts / uint32_t(threads))), dim3(threads), lds_bytes, stream, p);
    return hipGetLastError();
}

hipError_t launch_morph_apply(bool f16, const DeformParams &p, const FlattenParams *fused, hipStream_t stream) {
    const dim3 grid((p.nv + kThreads - 1) / kThreads);
    if (fused) {
        const size_t lds = size_t(fused->ns + 1) * 4;
        if (f16) hipLaunchKernelGGL((morph_apply_kernel<true, true>), grid, dim3(kThreads), lds, stream, p, *fused);
        else hipLaunchKernelGGL((morph_apply_kernel<false, true>), grid, dim3(kThreads), lds, stream, p, *fused);
    } else {
        FlattenParams none{};
        if (f16) hipLaunchKernelGGL((morph_apply_kernel<true, false>), grid, dim3(kThreads), 0, stream, p, none);
        else hipLaunchKernelGGL((morph_apply_kernel<false, false>), grid, dim3(kThreads), 0, stream, p, none);
    }
    return hipGetLastError();
}

}  // namespace

const KernelSet &MMDX_K(kernels)() {
    static const KernelSet set = {launch_deform, launch_frame, launch_pack, launch_morph_apply, prepare_kernels};
    return set;
}

#ifndef MMDX_FAST_MATH
hipError_t launch_pattern_fill(void *a, void *b, uint32_t nv, uint32_t ni, uint32_t bpva, uint32_t bpvb,
                               hipStream_t stream, uint32_t pitch) {
    const uint32_t ntiles = (nv + kTileVerts - 1) / kTileVerts;
    hipLaunchKernelGGL(pattern_fill_kernel, dim3(ntiles * ((ni + 15) / 16)), dim3(kThreads), 0, stream,
                       reinterpret_cast<float4 *>(a), reinterpret_cast<float4 *>(b), nv, ni, ntiles, bpva, bpvb,
                       pitch ? pitch : nv);
    return hipGetLastError();
}

hipError_t launch_bounds_reduce(const float *partials, uint32_t units, uint32_t ni, float *out, hipStream_t stream) {
    hipLaunchKernelGGL(bounds_reduce_kernel, dim3(ni), dim3(64), 0, stream, partials, out, units);
    return hipGetLastError();
}

hipError_t launch_bounds_reduce_select(const float *partials, uint32_t units, uint32_t ni, float *out, const uint32_t *ids,
                                       const uint32_t *count, uint32_t n_ids, hipStream_t stream) {
    if (n_ids == 0) return hipSuccess;
    hipLaunchKernelGGL(bounds_reduce_select_kernel, dim3(n_ids), dim3(64), 0, stream, partials, out, units, ni, ids, count, n_ids);
    return hipGetLastError();
}

hipError_t launch_flatten(const FlattenParams &f, hipStream_t stream) {
    const uint32_t rows = f.quad ? ((f.niw + 3) / 4) * 4 : f.niw;
    return launch_lane_items<kThreads>(f.list.ids ? flatten_select_kernel : flatten_kernel, rows, f.ns + 1, stream, f);
}

// The per-(instance, morph) kernels: launch_lane_items (instance_list.hpp); the select form is sized from t.ni = the list's capacity.
hipError_t launch_morph_track_eval(const MorphTrackParams &t, hipStream_t stream) {
    return launch_lane_items<kThreads>(MMDX_BY_CLOCK(morph_track_eval_kernel, t.times), t.ni, t.nm, stream, t);
}

hipError_t launch_morph_track_eval_set(const MorphTrackParams &t, const uint32_t *clips, uint32_t n_clips, hipStream_t stream) {
    return launch_lane_items<kThreads>(MMDX_BY_CLOCK(morph_track_eval_set_kernel, t.times), t.ni, t.nm, stream, t, clips, n_clips);
}

hipError_t launch_morph_track_blend_set(const MorphTrackParams &t, const BlendOperands &o, hipStream_t stream) {
    return launch_lane_items<kThreads>(morph_track_blend_set_kernel<TimeClock>, t.ni, t.nm, stream, t, o);
}

hipError_t launch_morph_track_blend_set_select(const MorphTrackParams &t, const BlendOperands &o, const InstanceList &list,
                                               hipStream_t stream) {
    return launch_lane_items<kThreads>(morph_track_blend_set_select_kernel<TimeClock>, t.ni, t.nm, stream, t, o, list);
}

hipError_t launch_copy(void *dst, const void *src, size_t bytes, hipStream_t stream) {
    hipLaunchKernelGGL(copy_kernel, dim3(uint32_t((bytes / 16 + kThreads - 1) / kThreads)),
                       dim3(kThreads), 0, stream, reinterpret_cast<float4 *>(dst),
                       reinterpret_cast<const float4 *>(src), bytes / 16);
    return hipGetLastError();
}

hipError_t launch_fill(void *dst, size_t bytes, hipStream_t stream) {
    hipLaunchKernelGGL(fill_kernel, dim3(uint32_t((bytes / 16 + kThreads - 1) / kThreads)),
                       dim3(kThreads), 0, stream, reinterpret_cast<float4 *>(dst), bytes / 16);
    return hipGetLastError();
}

#endif  // !MMDX_FAST_MATH

}  // namespace mmdx

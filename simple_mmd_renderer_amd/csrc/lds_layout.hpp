// lds_layout.hpp -- the dynamic-LDS layout of the deform kernels, in one place for the kernels (kernels.hip) and for the host code
// that sizes a launch (launch_shape.cpp).  No HIP runtime dependency: a plain C++17 compiler reads it as it stands.
#pragma once

#include <cstddef>
#include <cstdint>

#include "plan.hpp"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MMDX_HD __host__ __device__
#else
#define MMDX_HD
#endif

namespace mmdx {

// Morph handling of one deform launch
enum : int {
    kMorphNone = 0,     // model has no vertex-morph slot
    kMorphShared = 1,   // positions come from the `morphed` buffer written by morph_apply (crowd
                        // with one shared facial state: the morph pass runs once per call)
    kMorphFused1 = 2,   // ONE set of morph rates for the launch, gathered inside the deform kernel: a single-model frame,
                        // or a crowd with a shared facial state (every workgroup repeats its tile's walk)
    kMorphFused4 = 3,   // per-instance weights, 4 instances share one pass over a CSR row
    kMorphSelect = 16   // kernels.hip only: ORed into deform_kernel's morph-mode template argument for the flavour of
                        // mmdx_deform_batched_select (modes 16..19 in kernel listings)
};
// Most slots whose weights a kernel evaluates itself, into LDS (morph_apply_kernel with the flatten fused in, the kMorphFused1
// gather of a crowd); models past it take the separate flatten launch (launch_shape.cpp, plan_morph_pass)
constexpr uint32_t kMaxFusedSlots = 8192;

// LDS staging images of one tile's output range (bytes; all multiples of 16)
constexpr uint32_t kSoaImgBytes = (kTileVerts * 3 + 4) * 4;        // f32 xyz + alignment slack
constexpr uint32_t kV32ImgBytes = kTileVerts * 32;
constexpr uint32_t kP16ImgBytes = (kTileVerts * 3 + 8) * 2;        // f16 xyz + alignment slack
static_assert(kSoaImgBytes % 16 == 0 && kP16ImgBytes % 16 == 0, "image alignment");

MMDX_HD constexpr uint32_t stage_bytes(int layout) {
    return layout == MMDX_OUT_SOA ? 2 * kSoaImgBytes
                                  : (layout == MMDX_OUT_VERTEX32 ? kV32ImgBytes
                                                                 : kP16ImgBytes + kSoaImgBytes);
}

constexpr uint32_t kPkPack = 4;
constexpr uint32_t kPkRegion = kSoaImgBytes;          // one `mp` region: 512 x 3 f32 coordinates, or a position image (f32: 6160 B, f16: 3088 B)
static_assert(kPkRegion >= kTileVerts * 12 && kPkRegion >= kP16ImgBytes && kPkRegion % 16 == 0, "mp region");

constexpr uint32_t kBoundsLdsBytes = 2 * 8 * 6 * 4;     // combine words: 2 instance parities x up to 8 waves x 6 floats

// Bytes of dynamic LDS the deform kernel needs for (layout, morph mode, group).
inline size_t deform_lds_bytes(int threads, int layout, int morph, uint32_t group, uint32_t max_tile_bones, uint32_t ns,
                               uint32_t *stage_off, uint32_t *w_off, bool tile_order = false) {
    size_t off = size_t(group) * max_tile_bones * 48;
    *stage_off = uint32_t(off);
    if (!tile_order) off += 2 * size_t(stage_bytes(layout));     // tile-order outputs need no LDS image
    *w_off = uint32_t(off);
    if (morph == kMorphFused1) off += (size_t(ns + 1) * 4 + 15) / 16 * 16;
    else if (morph == kMorphFused4) off += (threads == 512 ? 2 : 1) * size_t(ns + 1) * 16;   // one or two instance quads
    return off;
}

// pack_kernel: [palettes of the group][slot weights of one pack][kPkPack coordinate / position-image regions][2 normal images]
inline size_t pack_lds_bytes(uint32_t group, uint32_t max_tile_bones, uint32_t ns, uint32_t *stage_off, uint32_t *w_off, uint32_t *mp_off) {
    size_t off = size_t(group) * max_tile_bones * 48;
    *w_off = uint32_t(off);
    off += size_t(ns + 1) * 16;
    *mp_off = uint32_t(off);
    off += size_t(kPkPack) * kPkRegion;
    *stage_off = uint32_t(off);
    off += 2 * size_t(kSoaImgBytes);
    return off;
}

// frame_kernel: the tile's palette, then the slot weights at *w_off.
inline size_t frame_lds_bytes(int morph, uint32_t max_tile_bones, uint32_t ns, uint32_t *w_off) {
    size_t off = (size_t(max_tile_bones) * 48 + 15) / 16 * 16;
    *w_off = uint32_t(off);
    if (morph == kMorphFused1) off += (size_t(ns + 1) * 4 + 15) / 16 * 16;
    return off;
}

// Partial bounds (6 floats) per instance of a bounds launch: one per tile, or one per wave of a tile for tile-order outputs (no
// per-instance barrier there to combine the waves' partials).  `threads` as passed to launch_deform.
inline uint32_t deform_bounds_units(int threads, uint32_t ntiles, bool tile_order) {
    return tile_order ? ntiles * ((threads == 256 || kTileVerts < 512) ? 256u : 512u) / 64u : ntiles;
}

// Does this launch shape exist in the write-through store flavour?  (Measured to pay on the SoA f32 crowd kernels only: 256 threads,
// no morphs or shared morphs, original vertex order.)  The planner asks before it sets LaunchShape::write_through, pick() asserts it.
constexpr bool deform_has_write_through(int threads, int layout, int morph, bool f16, bool tile_order) {
    return threads == 256 && layout == 0 /* MMDX_OUT_SOA */ && !f16 && !tile_order && (morph == kMorphNone || morph == kMorphShared);
}

}  // namespace mmdx

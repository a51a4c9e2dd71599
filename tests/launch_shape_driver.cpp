// CPU driver of the launch planner (simple_mmd_renderer_amd/csrc/launch_shape.cpp), built by tests/test_launch_shape.py with g++ under
// ASan + UBSan from this file and launch_shape.cpp alone.
//   launch_shape_driver sweep     the planner over a cross product of calls, models and overrides; every shape is checked against
//                                 what follows from the code's own rules (no measured number); prints the row count
//   launch_shape_driver eval      one call per line on stdin (the fields of Case in order), its shape per line on stdout
// LAUNCH_SHAPE_DRIVER_NO_MAIN: a scratch program may include this file for for_each_case() / plan_case() and compare the planner,
// over the same sweep, with another build of the heuristics.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../simple_mmd_renderer_amd/csrc/launch_shape.hpp"

using namespace mmdx;

namespace {

struct Case {
    // the model
    uint32_t f16, tile_order, ntiles, max_tile_bones, ns;
    // the call
    uint32_t layout, ni, nwork, flags;
    int morph;
    uint32_t bounds, select, out_dev, out_host_mapped;
    uint64_t out_bytes;
    // the overrides that shape a launch (0 / 0 / 0 / 0 / -1 / 1 / 0 by default)
    int ov_threads, ov_group, ov_lds_target, ov_fused_pack, ov_store_wt, ov_frame_kernel, ov_stagger;
};

struct Result {
    mmdx_status status;
    LaunchShape shape;
    std::string err;
};

Result plan_case(const Case &c) {
    Plan p;
    p.f16 = c.f16 != 0;
    p.flags = c.tile_order ? uint32_t(MMDX_CREATE_TILE_ORDER) : 0u;
    p.ntiles = c.ntiles; p.max_tile_bones = c.max_tile_bones; p.ns = c.ns;
    DeformCall call{c.layout, c.ni, c.nwork, c.flags, c.morph, c.bounds != 0, c.select != 0, c.out_dev != 0, c.out_host_mapped != 0,
                    size_t(c.out_bytes)};
    // the defaults of read_launch_overrides() (api.cpp)
    LaunchOverrides ov{1, c.ov_threads, c.ov_lds_target, c.ov_group, 0, 0, c.ov_frame_kernel, 256, 1, c.ov_store_wt, 1, c.ov_fused_pack,
                       c.ov_stagger, 1};
    Result r;
    r.status = plan_deform_launch(p, call, ov, r.shape, r.err);
    return r;
}

uint64_t out_bytes_of(uint32_t layout, uint32_t ni, uint32_t nv) {
    const uint64_t nvi = uint64_t(ni) * nv;
    return layout == MMDX_OUT_SOA ? nvi * 24 : (layout == MMDX_OUT_VERTEX32 ? nvi * 32 : nvi * 18);
}

template <typename Fn>
void for_each_case(Fn fn) {
    struct Ov { int threads, group, fused_pack, store_wt, frame_kernel; };
    const Ov ovs[] = {{0, 0, 0, -1, 1}, {256, 0, 0, -1, 1}, {512, 0, 0, -1, 1}, {0, 16, 0, -1, 1}, {0, 0, 1, -1, 1},
                      {0, 0, 0, 0, 1},  {0, 0, 0, 1, 1},    {0, 0, 0, -1, 0},   {0, 0, 0, -1, 2}};
    const uint32_t layouts[][2] = {{MMDX_OUT_SOA, 0}, {MMDX_OUT_VERTEX32, 0}, {MMDX_OUT_SOA_POS16, 1}};      // {layout, f16}
    const uint32_t nis[] = {1, 2, 8, 9, 64, 1000, 1024, 16384}, ntiles_s[] = {1, 7, 98, 255, 256, 500};
    const uint32_t bones[] = {1, 48, 300, 900}, slots[] = {0, 1, 200, 8192, 8193, 40000};
    const uint32_t hints[] = {0, MMDX_OUT_STORES_WRITE_THROUGH, MMDX_OUT_STORES_CACHED};
    const uint32_t places[][2] = {{1, 0}, {0, 1}, {0, 0}};      // {out_dev, out_host_mapped}: device, page-locked host, staging
    Case c{};
    c.ov_lds_target = 0; c.ov_stagger = 0;
    for (const auto &l : layouts)
    for (int morph = kMorphNone; morph <= kMorphFused4; ++morph)
    for (uint32_t tile = 0; tile < 2; ++tile)
    for (uint32_t bounds = 0; bounds < 2; ++bounds)
    for (uint32_t ni : nis)
    for (int selk = -1; selk < 4; ++selk)                       // -1: no list; else its capacity 0, 1, 64, ni
    for (uint32_t ntiles : ntiles_s)
    for (uint32_t mtb : bones)
    for (uint32_t ns : slots)
    for (uint32_t hint : hints)
    for (const auto &pl : places)
    for (const Ov &o : ovs) {
        c.layout = l[0]; c.f16 = l[1]; c.morph = morph; c.tile_order = tile; c.bounds = bounds; c.ni = ni;
        c.select = selk >= 0;
        c.nwork = selk < 0 ? ni : (selk == 0 ? 0u : (selk == 1 ? 1u : (selk == 2 ? 64u : ni)));
        c.ntiles = ntiles; c.max_tile_bones = mtb; c.ns = ns; c.flags = hint;
        c.out_dev = pl[0]; c.out_host_mapped = pl[1];
        c.out_bytes = out_bytes_of(c.layout, ni, ntiles * kTileVerts);
        c.ov_threads = o.threads; c.ov_group = o.group; c.ov_fused_pack = o.fused_pack; c.ov_store_wt = o.store_wt;
        c.ov_frame_kernel = o.frame_kernel;
        fn(c);
    }
}

#ifndef LAUNCH_SHAPE_DRIVER_NO_MAIN

void print_case(FILE *f, const Case &c) {
    std::fprintf(f, "f16=%u tile_order=%u ntiles=%u max_tile_bones=%u ns=%u layout=%u ni=%u nwork=%u flags=%u morph=%d bounds=%u select=%u "
                    "out_dev=%u out_host_mapped=%u out_bytes=%" PRIu64 " threads=%d group=%d lds_target=%d fused_pack=%d store_wt=%d "
                    "frame_kernel=%d stagger=%d\n",
                 c.f16, c.tile_order, c.ntiles, c.max_tile_bones, c.ns, c.layout, c.ni, c.nwork, c.flags, c.morph, c.bounds, c.select, c.out_dev,
                 c.out_host_mapped, c.out_bytes, c.ov_threads, c.ov_group, c.ov_lds_target, c.ov_fused_pack, c.ov_store_wt, c.ov_frame_kernel,
                 c.ov_stagger);
}

uint64_t g_failures = 0;
#define CHECK(cond)                                                                        \
    do {                                                                                   \
        if (!(cond)) {                                                                     \
            if (g_failures++ < 20) { std::fprintf(stderr, "FAILED %s\n  ", #cond); print_case(stderr, c); } \
            return;                                                                        \
        }                                                                                  \
    } while (0)

constexpr size_t kLds = 160 * 1024;

size_t weight_bytes(const Case &c, int threads) {
    if (c.morph == kMorphFused1) return (size_t(c.ns) + 1) * 4;
    if (c.morph == kMorphFused4) return (threads == 512 ? 2 : 1) * (size_t(c.ns) + 1) * 16;
    return 0;
}

void check_case(const Case &c, uint64_t &rejected) {
    const Result r = plan_case(c);
    const LaunchShape &s = r.shape;
    if (r.status != MMDX_OK) {
        // the only refusal: more LDS than a CU has
        CHECK(r.status == MMDX_ERR_UNSUPPORTED && s.lds > kLds && !r.err.empty());
        ++rejected;
        return;
    }
    CHECK(s.lds <= kLds);
    CHECK(s.threads == 256 || s.threads == 512);
    CHECK(s.group >= 1);
    if (c.morph == kMorphFused4) CHECK(s.group % (s.kernel == LaunchShape::kPack || s.threads == 256 ? 4u : 8u) == 0);
    const bool plain = !c.bounds && !c.select;
    CHECK(!s.write_through ||
          (deform_has_write_through(s.threads, int(c.layout), c.morph, c.f16 != 0, c.tile_order != 0) && c.out_dev && plain));
    CHECK(s.kernel != LaunchShape::kFrame || (c.ni == 1 && !c.out_host_mapped && plain));
    CHECK(s.kernel != LaunchShape::kPack || (c.ov_fused_pack != 0 && plain && c.morph == kMorphFused4));
    CHECK((s.kernel == LaunchShape::kNone) == (c.select && c.nwork == 0));
    CHECK(s.bounds_units == (c.bounds ? deform_bounds_units(s.threads, c.ntiles, c.tile_order != 0) : 0u));
    CHECK((s.stage_off | s.w_off | s.mp_off | s.bounds_off) % 16 == 0);
    const size_t pal = size_t(s.group) * c.max_tile_bones * 48;
    if (s.kernel == LaunchShape::kFrame) {
        // [the tile's palette][slot weights]
        CHECK(s.w_off >= size_t(c.max_tile_bones) * 48 && s.w_off + weight_bytes(c, 256) <= s.lds);
    } else if (s.kernel == LaunchShape::kPack) {
        // [palettes][slot weights of one pack][kPkPack regions][2 normal images]
        CHECK(pal <= s.w_off && s.w_off + (size_t(c.ns) + 1) * 16 <= s.mp_off);
        CHECK(s.mp_off + size_t(kPkPack) * kPkRegion <= s.stage_off && s.stage_off + 2 * size_t(kSoaImgBytes) <= s.lds);
    } else {
        // [palettes][2 staging images, none in tile order][slot weights][bounds combine words, image path only]
        const size_t images = c.tile_order ? 0 : 2 * size_t(stage_bytes(int(c.layout)));
        const bool combine = c.bounds && !c.tile_order;
        const size_t end = combine ? s.bounds_off : s.lds;
        CHECK(pal <= s.stage_off && s.stage_off + images <= s.w_off && s.w_off + weight_bytes(c, s.threads) <= end);
        CHECK(s.stage_off <= s.w_off && s.w_off <= end);
        if (combine) CHECK(s.bounds_off < s.lds && s.bounds_off + kBoundsLdsBytes <= s.lds);
        else CHECK(s.bounds_off == 0);
    }
}

void print_result(const Result &r) {
    const LaunchShape &s = r.shape;
    if (r.status != MMDX_OK) { std::printf("status=%d err=%s\n", int(r.status), r.err.c_str()); return; }
    std::printf("status=0 kernel=%d threads=%d group=%u lds=%zu stage_off=%u w_off=%u mp_off=%u bounds_off=%u bounds_units=%u stagger=%u "
                "slots_per_cu=%u write_through=%d\n",
                int(s.kernel), s.threads, s.group, s.lds, s.stage_off, s.w_off, s.mp_off, s.bounds_off, s.bounds_units, s.stagger,
                s.slots_per_cu, int(s.write_through));
}

}  // namespace

int main(int argc, char **argv) {
    if (argc == 2 && !std::strcmp(argv[1], "sweep")) {
        uint64_t rows = 0, rejected = 0;
        for_each_case([&](const Case &c) { ++rows; check_case(c, rejected); });
        std::printf("rows=%" PRIu64 " rejected=%" PRIu64 " failures=%" PRIu64 "\n", rows, rejected, g_failures);
        return g_failures ? 1 : 0;
    }
    if (argc == 2 && !std::strcmp(argv[1], "eval")) {
        Case c{};
        while (std::scanf("%u %u %u %u %u %u %u %u %u %d %u %u %u %u %" SCNu64 " %d %d %d %d %d %d %d", &c.f16, &c.tile_order, &c.ntiles,
                          &c.max_tile_bones, &c.ns, &c.layout, &c.ni, &c.nwork, &c.flags, &c.morph, &c.bounds, &c.select, &c.out_dev,
                          &c.out_host_mapped, &c.out_bytes, &c.ov_threads, &c.ov_group, &c.ov_lds_target, &c.ov_fused_pack, &c.ov_store_wt,
                          &c.ov_frame_kernel, &c.ov_stagger) == 22)
            print_result(plan_case(c));
        return 0;
    }
    std::fprintf(stderr, "usage: %s sweep | eval\n", argv[0]);
    return 2;
}

#else
}  // namespace
#endif

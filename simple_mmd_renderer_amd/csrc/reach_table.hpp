// reach_table.hpp -- a reach set's table and its host builder: what mmdx_reach_set_create (reach_api.cpp) validates and uploads, and
// what the kernel (reach_kernels.hip) reads per reach and subtree row; and the planner of the kernel's launch.  No HIP here:
// tests/reach_math_driver.cpp compiles these lines with g++ (and under ASan + UBSan).  Everything is decided from the desc and the
// skeleton's parents and rest positions; no device is touched.  The hierarchy is the parent array alone, walked as bone_mask.hpp
// walks it: a value outside [0, nb) ends a chain, and a chain is followed for at most nb steps.
#pragma once

#include <cstdint>
#include <string>
#include <vector>

#include "../../include/mmdx.h"
#include "error.hpp"
#include "reach_math.hpp"

namespace mmdx {

// ---- the block of instances of one workgroup -------------------------------------------------------------------------------------
// One workgroup of the kernel owns (reach, 16 consecutive instances or list positions) and keeps their three matrices in LDS,
// instance fastest: [3][12][16] floats, then one word per instance, "applied".  The aim's A/B found no crowd size at
// which a larger block wins, so there is one block size and no knob.
constexpr uint32_t kReachThreads = 256, kReachBlock = 16;
constexpr uint32_t kReachMaxCells = 1u << 23;      // instances or list positions in one call
constexpr uint32_t kReachMaxBones = 1u << 20;      // of the skeleton: a workgroup's 16 x n_rows x 4 items stay far below 2^32

struct ReachShape {
    uint32_t block;           // instances per workgroup: 16
    uint32_t threads;         // lanes per workgroup
    uint32_t nblocks;         // ceil(cells / block): the x extent of the grid (y: the reaches)
    uint32_t lds;             // bytes of dynamic LDS
};

// cells: instances, or list positions of a select call (> 0)
inline ReachShape plan_reach_launch(uint32_t cells) {
    ReachShape s{};
    s.block = kReachBlock;
    s.threads = kReachThreads;
    s.nblocks = (cells + s.block - 1) / s.block;
    s.lds = s.block * (kReachDepths * kReachMatrixFloats + 1) * 4;
    return s;
}

// ---- the table -------------------------------------------------------------------------------------------------------------------
struct ReachTable {
    std::vector<ReachReach> reaches;
    std::vector<ReachRow> rows;
    uint32_t nb = 0;
};

// `b` is `a` or below it
inline bool reach_is_under(const int32_t *parent, uint32_t nb, uint32_t a, uint32_t b) {
    uint32_t c = b;
    for (uint32_t step = 0; step <= nb; ++step) {        // b itself, then at most nb parents
        if (c == a) return true;
        const int32_t p = parent[c];
        if (p < 0 || uint32_t(p) >= nb || step == nb) break;
        c = uint32_t(p);
    }
    return false;
}

// The table `d` describes on a skeleton of nb bones (parent[nb], -1 = none; rest[nb][3]), validated.
inline mmdx_status reach_table_build(const mmdx_reach_set_desc *d, uint32_t nb, const int32_t *parent, const float *rest, ReachTable *out) {
    const auto bad = [](const std::string &m) { return fail(MMDX_ERR_INVALID_ARGUMENT, "mmdx_reach_set_desc: " + m); };
    const auto nan = [](float x) { return x != x; };
    if (!d) return fail(MMDX_ERR_INVALID_ARGUMENT, "desc is NULL");
    if (d->struct_size != sizeof(mmdx_reach_set_desc)) return bad("struct_size mismatch");
    if (d->reserved0 != 0) return bad("reserved0 must be 0");
    if (nb > kReachMaxBones) return fail(MMDX_ERR_UNSUPPORTED, "mmdx_reach_set_create: a skeleton of more than 2^20 bones");
    if (!d->n_reaches || d->n_reaches > kReachMaxReaches)
        return bad("n_reaches = " + std::to_string(d->n_reaches) + ": 1 to MMDX_REACH_MAX_REACHES (16)");
    if (!d->bones || !d->tip_point || !d->pole || !d->max_extension || !d->flags)
        return bad("bones / tip_point / pole / max_extension / flags is NULL");
    for (uint32_t i = 0; i < d->n_reaches * 3; ++i)
        if (d->bones[i] >= nb)
            return fail(MMDX_ERR_BAD_INDEX, "mmdx_reach_set_desc.bones[" + std::to_string(i / 3) + "][" + std::to_string(i % 3) + "] = " +
                                            std::to_string(d->bones[i]) + ": the skeleton has " + std::to_string(nb) + " bones");
    ReachTable t;
    t.nb = nb;
    t.reaches.assign(d->n_reaches, ReachReach{});
    std::vector<int32_t> owner(nb, -1);                  // the reach whose subtree holds the bone
    for (uint32_t r = 0; r < d->n_reaches; ++r) {
        const uint32_t a = d->bones[r * 3], b = d->bones[r * 3 + 1], c = d->bones[r * 3 + 2];
        const std::string name = "reach " + std::to_string(r);
        if (b == a || !reach_is_under(parent, nb, a, b))
            return bad("b = " + std::to_string(b) + " of " + name + " is not a strict descendant of a = " + std::to_string(a));
        if (c == b || !reach_is_under(parent, nb, b, c))
            return bad("c = " + std::to_string(c) + " of " + name + " is not a strict descendant of b = " + std::to_string(b));
        const float *e = d->tip_point + size_t(r) * 3, *pole = d->pole + size_t(r) * 3, ext = d->max_extension[r];
        for (int j = 0; j < 3; ++j)
            if (nan(e[j]) || nan(pole[j])) return bad("tip_point / pole of " + name + " holds a NaN");
        if (nan(ext)) return bad("max_extension of " + name + " is a NaN");
        if (!(ext > 0.0f && ext <= 1.0f)) return bad("max_extension of " + name + " is outside (0, 1]");
        if (!reach_finite(pole[0]) || !reach_finite(pole[1]) || !reach_finite(pole[2]) || (pole[0] == 0.0f && pole[1] == 0.0f && pole[2] == 0.0f))
            return bad("pole of " + name + " is zero or not finite");
        if (d->flags[r] & ~uint32_t(MMDX_REACH_KEEP_END_ROTATION))
            return bad("unknown flag bits in flags of " + name);
        ReachReach &m = t.reaches[r];
        m.a = a; m.b = b; m.c = c;
        m.flags = d->flags[r];
        m.max_extension = ext;
        for (int j = 0; j < 3; ++j) {
            m.ha[j] = rest[size_t(a) * 3 + j];
            m.hb[j] = rest[size_t(b) * 3 + j];
            m.hc[j] = rest[size_t(c) * 3 + j];
            m.e[j] = e[j];
            m.pole[j] = pole[j];
        }
        m.first_row = uint32_t(t.rows.size());
        for (uint32_t s = 0; s < nb; ++s) {              // ascending bone order
            if (!reach_is_under(parent, nb, a, s)) continue;
            if (owner[s] >= 0)
                return bad("the subtrees of reach " + std::to_string(owner[s]) + " and " + name + " intersect at bone " + std::to_string(s));
            owner[s] = int32_t(r);
            const uint32_t depth = reach_is_under(parent, nb, c, s) ? 2u : reach_is_under(parent, nb, b, s) ? 1u : 0u;
            t.rows.push_back(ReachRow{s, depth});
        }
        m.n_rows = uint32_t(t.rows.size()) - m.first_row;
    }
    *out = std::move(t);
    return MMDX_OK;
}

// One instance, every reach: what a workgroup of the kernel does for one of its instances, on the host.  pal: this instance's
// [nb][16] rows, rewritten in place (a reach reads rows of its own subtree only, and the subtrees of a set are disjoint); tgt: its
// four target floats.
inline void reach_instance(const ReachTable &t, float *pal, const float *tgt) {
    const float w = reach_weight(tgt);
    if (!(w > 0.0f)) return;
    for (const ReachReach &m : t.reaches) {
        float c[kReachDepths][16];
        if (!reach_solve(pal + size_t(m.a) * 16, pal + size_t(m.b) * 16, pal + size_t(m.c) * 16, m, tgt, w, c[0], c[1], c[2])) continue;
        for (uint32_t r = m.first_row; r < m.first_row + m.n_rows; ++r) {
            const ReachRow &s = t.rows[r];
            float *row = pal + size_t(s.bone) * 16, o[16];
            reach_mul(row, c[s.depth], o);
            for (int i = 0; i < 16; ++i) row[i] = o[i];
        }
    }
}

}  // namespace mmdx

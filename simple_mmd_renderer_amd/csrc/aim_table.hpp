// aim_table.hpp -- an aim set's table and its host builder: what mmdx_aim_set_create (aim_api.cpp) validates and uploads, and what
// the kernel (aim_kernels.hip) reads per aim, link and subtree row; and the planner of the kernel's block of instances.  No HIP here:
// tests/aim_math_driver.cpp compiles these lines with g++ (and under ASan + UBSan).  Everything is decided from the desc and the
// skeleton's parents and rest positions; no device is touched.  The hierarchy is the parent array alone, walked as bone_mask.hpp
// walks it: a value outside [0, nb) ends a chain, and a chain is followed for at most nb steps.
#pragma once

#include <cstdint>
#include <string>
#include <vector>

#include "../../include/mmdx.h"
#include "aim_math.hpp"
#include "error.hpp"

namespace mmdx {

// ---- the block of instances of one workgroup -------------------------------------------------------------------------------------
// One workgroup of the kernel owns (aim, `block` consecutive instances or list positions) and keeps their cumulative matrices in
// LDS, instance fastest: [max_links][12][block] floats, then one word per instance, the first applied link.
// Measured (tools/aim_ab.py): 16 instances to a workgroup take 0.36 and 0.47 of the time of 64 at 1 024 and 16 384
// instances x 300 bones, 1.01 and 0.95 at 65 536 and 131 072 -- no crowd size was found at which 64 is clearly faster, so the crowd
// size does not enter the choice: 16 unless MMDX_AIM_BLOCK asks for 64.
constexpr uint32_t kAimThreads = 256, kAimSmallBlock = 16, kAimLargeBlock = 64;
constexpr uint32_t kAimMaxCells = 1u << 23;      // instances or list positions in one call
constexpr uint32_t kAimMaxBones = 1u << 20;      // of the skeleton: a workgroup's 64 x n_rows x 4 items stay far below 2^32

struct AimShape {
    uint32_t block;           // instances per workgroup: 16 or 64
    uint32_t threads;         // lanes per workgroup
    uint32_t nblocks;         // ceil(cells / block): the x extent of the grid (y: the aims)
    uint32_t lds;             // bytes of dynamic LDS
};

// cells: instances, or list positions of a select call (> 0); max_links: the longest aim of the set; env: MMDX_AIM_BLOCK as read
// for this call (64 forces the large block, anything else: the small one).
inline AimShape plan_aim_launch(uint32_t cells, uint32_t max_links, int env) {
    AimShape s{};
    s.block = env == int(kAimLargeBlock) ? kAimLargeBlock : kAimSmallBlock;
    s.threads = kAimThreads;
    s.nblocks = (cells + s.block - 1) / s.block;
    s.lds = s.block * (max_links * kAimMatrixFloats + 1) * 4;
    return s;
}

// ---- the table -------------------------------------------------------------------------------------------------------------------
struct AimTable {
    std::vector<AimAim> aims;
    std::vector<AimLink> links;
    std::vector<AimRow> rows;
    uint32_t nb = 0, max_links = 0;
};

// `b` is `a` or below it
inline bool aim_is_under(const int32_t *parent, uint32_t nb, uint32_t a, uint32_t b) {
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
inline mmdx_status aim_table_build(const mmdx_aim_set_desc *d, uint32_t nb, const int32_t *parent, const float *rest, AimTable *out) {
    const auto bad = [](const std::string &m) { return fail(MMDX_ERR_INVALID_ARGUMENT, "mmdx_aim_set_desc: " + m); };
    const auto nan = [](float x) { return x != x; };
    if (!d) return fail(MMDX_ERR_INVALID_ARGUMENT, "desc is NULL");
    if (d->struct_size != sizeof(mmdx_aim_set_desc)) return bad("struct_size mismatch");
    if (d->reserved0 != 0) return bad("reserved0 must be 0");
    if (nb > kAimMaxBones) return fail(MMDX_ERR_UNSUPPORTED, "mmdx_aim_set_create: a skeleton of more than 2^20 bones");
    if (!d->n_aims || d->n_aims > kAimMaxAims) return bad("n_aims = " + std::to_string(d->n_aims) + ": 1 to MMDX_AIM_MAX_AIMS (16)");
    if (!d->link_offset || !d->link_bone || !d->link_params || !d->eye_bone || !d->eye_point || !d->forward)
        return bad("link_offset / link_bone / link_params / eye_bone / eye_point / forward is NULL");
    if (d->link_offset[0] != 0) return bad("link_offset[0] must be 0");
    for (uint32_t a = 0; a < d->n_aims; ++a) {
        const uint32_t lo = d->link_offset[a], hi = d->link_offset[a + 1];
        if (hi <= lo || hi - lo > kAimMaxLinks)
            return bad("aim " + std::to_string(a) + " has " + std::to_string(hi <= lo ? 0u : hi - lo) + " links: 1 to MMDX_AIM_MAX_LINKS (4)");
    }
    const uint32_t nl = d->link_offset[d->n_aims];
    for (uint32_t l = 0; l < nl; ++l)
        if (d->link_bone[l] >= nb)
            return fail(MMDX_ERR_BAD_INDEX, "mmdx_aim_set_desc.link_bone[" + std::to_string(l) + "] = " + std::to_string(d->link_bone[l]) +
                                            ": the skeleton has " + std::to_string(nb) + " bones");
    for (uint32_t a = 0; a < d->n_aims; ++a)
        if (d->eye_bone[a] >= nb)
            return fail(MMDX_ERR_BAD_INDEX, "mmdx_aim_set_desc.eye_bone[" + std::to_string(a) + "] = " + std::to_string(d->eye_bone[a]) +
                                            ": the skeleton has " + std::to_string(nb) + " bones");
    AimTable t;
    t.nb = nb;
    t.aims.assign(d->n_aims, AimAim{});
    t.links.assign(nl, AimLink{});
    std::vector<int32_t> owner(nb, -1);                  // the aim whose subtree holds the bone
    for (uint32_t a = 0; a < d->n_aims; ++a) {
        const uint32_t lo = d->link_offset[a], hi = d->link_offset[a + 1];
        const std::string name = "aim " + std::to_string(a);
        for (uint32_t l = lo; l < hi; ++l) {
            const uint32_t b = d->link_bone[l];
            if (l > lo && (b == d->link_bone[l - 1] || !aim_is_under(parent, nb, d->link_bone[l - 1], b)))
                return bad("link_bone[" + std::to_string(l) + "] = " + std::to_string(b) + " is not a strict descendant of the link before it");
            const float share = d->link_params[size_t(l) * 2], cos_limit = d->link_params[size_t(l) * 2 + 1];
            if (nan(share) || nan(cos_limit)) return bad("link_params[" + std::to_string(l) + "] holds a NaN");
            if (!(share >= 0.0f && share <= 1.0f)) return bad("link_params[" + std::to_string(l) + "]: share is outside [0, 1]");
            if (!(cos_limit >= -1.0f && cos_limit <= 1.0f)) return bad("link_params[" + std::to_string(l) + "]: cos_limit is outside [-1, 1]");
            AimLink &k = t.links[l];
            k.bone = b;
            for (int j = 0; j < 3; ++j) k.h[j] = rest[size_t(b) * 3 + j];
            k.share = share;
            k.cos_limit = cos_limit;
            k.sin_limit = float(sqrt(double(1.0f - cos_limit * cos_limit)));
        }
        if (!aim_is_under(parent, nb, d->link_bone[hi - 1], d->eye_bone[a]))
            return bad("eye_bone[" + std::to_string(a) + "] = " + std::to_string(d->eye_bone[a]) + " is outside the subtree of the last link of " + name);
        const float *e = d->eye_point + size_t(a) * 3, *f = d->forward + size_t(a) * 3;
        for (int j = 0; j < 3; ++j)
            if (nan(e[j]) || nan(f[j])) return bad("eye_point / forward of " + name + " holds a NaN");
        if (!aim_finite(f[0]) || !aim_finite(f[1]) || !aim_finite(f[2]) || (f[0] == 0.0f && f[1] == 0.0f && f[2] == 0.0f))
            return bad("forward of " + name + " is zero or not finite");
        AimAim &m = t.aims[a];
        m.first_link = lo;
        m.n_links = hi - lo;
        m.eye_bone = d->eye_bone[a];
        m.first_row = uint32_t(t.rows.size());
        for (int j = 0; j < 3; ++j) {
            m.e[j] = e[j];
            m.f[j] = f[j];
        }
        for (uint32_t b = 0; b < nb; ++b) {              // ascending bone order
            if (!aim_is_under(parent, nb, d->link_bone[lo], b)) continue;
            if (owner[b] >= 0)
                return bad("the subtrees of aim " + std::to_string(owner[b]) + " and " + name + " intersect at bone " + std::to_string(b));
            owner[b] = int32_t(a);
            uint32_t depth = 0;
            for (uint32_t l = lo + 1; l < hi; ++l)
                if (aim_is_under(parent, nb, d->link_bone[l], b)) depth = l - lo;
            t.rows.push_back(AimRow{b, depth});
        }
        m.n_rows = uint32_t(t.rows.size()) - m.first_row;
        t.max_links = m.n_links > t.max_links ? m.n_links : t.max_links;
    }
    *out = std::move(t);
    return MMDX_OK;
}

// One instance, every aim: what a workgroup of the kernel does for one of its instances, on the host.  pal: this instance's
// [nb][16] rows, rewritten in place; tgt: its four target floats.
inline void aim_instance(const AimTable &t, float *pal, const float *tgt) {
    const float w = aim_weight(tgt);
    if (!(w > 0.0f)) return;
    for (const AimAim &m : t.aims) {
        float c[kAimMaxLinks][16];
        uint32_t first = m.n_links;
        float cur[16];
        for (uint32_t l = 0; l < m.n_links; ++l) {
            const AimLink &k = t.links[m.first_link + l];
            if (aim_link(pal + size_t(k.bone) * 16, pal + size_t(m.eye_bone) * 16, k, m.e, m.f, tgt, w, cur, first < m.n_links) &&
                first == m.n_links)
                first = l;
            for (int i = 0; i < 16; ++i) c[l][i] = first < m.n_links ? cur[i] : 0.0f;
        }
        for (uint32_t r = m.first_row; r < m.first_row + m.n_rows; ++r) {
            const AimRow &s = t.rows[r];
            if (s.depth < first) continue;
            float *row = pal + size_t(s.bone) * 16, o[16];
            aim_mul(row, c[s.depth], o);
            for (int i = 0; i < 16; ++i) row[i] = o[i];
        }
    }
}

}  // namespace mmdx

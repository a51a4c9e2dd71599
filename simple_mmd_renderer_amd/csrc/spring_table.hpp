// spring_table.hpp -- a spring set's table and its host builder: what mmdx_spring_set_create (spring_api.cpp) validates and uploads,
// and what the kernel (spring_kernels.hip) reads per chain, joint and collider.  No HIP here: tests/spring_math_driver.cpp compiles
// these lines with g++ (and under ASan + UBSan).  Everything is decided from the desc and the skeleton's parents and rest positions;
// no device is touched.
#pragma once

#include <cstdint>
#include <string>
#include <vector>

#include "../../include/mmdx.h"
#include "error.hpp"
#include "spring_math.hpp"

namespace mmdx {

struct SpringTable {
    std::vector<SpringChain> chains;
    std::vector<SpringJoint> joints;
    std::vector<SpringCollider> colliders;
    float gravity[3] = {0.0f, 0.0f, 0.0f};
    uint32_t max_instances = 0, nb = 0;
};

// The table `d` describes on a skeleton of nb bones (parent[nb], -1 = none; rest[nb][3]), validated.
inline mmdx_status spring_table_build(const mmdx_spring_set_desc *d, uint32_t nb, const int32_t *parent, const float *rest,
                                      SpringTable *out) {
    const auto bad = [](const std::string &m) { return fail(MMDX_ERR_INVALID_ARGUMENT, "mmdx_spring_set_desc: " + m); };
    const auto nan = [](float x) { return x != x; };
    if (!d) return fail(MMDX_ERR_INVALID_ARGUMENT, "desc is NULL");
    if (d->struct_size != sizeof(mmdx_spring_set_desc)) return bad("struct_size mismatch");
    if (d->reserved0 != 0) return bad("reserved0 must be 0");
    if (!d->n_chains) return bad("n_chains == 0");
    if (d->n_chains > 65535u) return bad("n_chains is above 65535");
    if (!d->max_instances) return bad("max_instances == 0");
    if (d->n_colliders > kSpringMaxColliders)
        return bad("n_colliders = " + std::to_string(d->n_colliders) + ": at most MMDX_SPRING_MAX_COLLIDERS (16)");
    if (!d->chain_offset || !d->joint_bone || !d->chain_params) return bad("chain_offset / joint_bone / chain_params is NULL");
    if (d->n_colliders && (!d->collider_bone || !d->collider_sphere)) return bad("collider_bone / collider_sphere is NULL");
    if (d->chain_offset[0] != 0) return bad("chain_offset[0] must be 0");
    for (uint32_t c = 0; c < d->n_chains; ++c) {
        const uint32_t lo = d->chain_offset[c], hi = d->chain_offset[c + 1];
        if (hi <= lo || hi - lo > kSpringMaxJoints)
            return bad("chain " + std::to_string(c) + " has " + std::to_string(hi <= lo ? 0u : hi - lo) +
                       " joints: 1 to MMDX_SPRING_MAX_JOINTS (32)");
    }
    const uint32_t nj = d->chain_offset[d->n_chains];
    for (int k = 0; k < 3; ++k)
        if (nan(d->gravity[k])) return bad("gravity is NaN");
    std::vector<uint8_t> is_joint(nb, 0);
    for (uint32_t j = 0; j < nj; ++j) {
        const uint32_t b = d->joint_bone[j];
        if (b >= nb)
            return fail(MMDX_ERR_BAD_INDEX, "mmdx_spring_set_desc.joint_bone[" + std::to_string(j) + "] = " + std::to_string(b) +
                                            ": the skeleton has " + std::to_string(nb) + " bones");
        if (is_joint[b]) return bad("bone " + std::to_string(b) + " is listed twice");
        is_joint[b] = 1;
    }
    for (uint32_t j = 0; j < d->n_colliders; ++j)
        if (d->collider_bone[j] >= nb)
            return fail(MMDX_ERR_BAD_INDEX, "mmdx_spring_set_desc.collider_bone[" + std::to_string(j) + "] = " +
                                            std::to_string(d->collider_bone[j]) + ": the skeleton has " + std::to_string(nb) + " bones");
    SpringTable t;
    t.max_instances = d->max_instances;
    t.nb = nb;
    for (int k = 0; k < 3; ++k) t.gravity[k] = d->gravity[k];
    t.chains.assign(d->n_chains, SpringChain{});
    t.joints.assign(nj, SpringJoint{});
    t.colliders.assign(d->n_colliders, SpringCollider{});
    for (uint32_t c = 0; c < d->n_chains; ++c) {
        const uint32_t lo = d->chain_offset[c], hi = d->chain_offset[c + 1];
        const float *prm = d->chain_params + size_t(c) * 4;
        for (int k = 0; k < 4; ++k)
            if (nan(prm[k])) return bad("chain_params[" + std::to_string(c) + "] holds a NaN");
        if (!(prm[1] >= 0.0f && prm[1] <= 1.0f)) return bad("chain_params[" + std::to_string(c) + "]: drag is outside [0, 1]");
        const int32_t anchor = parent[d->joint_bone[lo]];
        if (anchor < 0 || uint32_t(anchor) >= nb) return bad("the first joint of chain " + std::to_string(c) + " has no parent");
        if (is_joint[anchor]) return bad("the anchor of chain " + std::to_string(c) + ", bone " + std::to_string(anchor) +
                                         ", is a joint of a chain");
        t.chains[c] = SpringChain{lo, hi - lo, uint32_t(anchor), 0u, prm[0], prm[1], prm[2], prm[3]};
        for (uint32_t j = lo; j < hi; ++j) {
            const uint32_t b = d->joint_bone[j];
            if (j > lo && (parent[b] < 0 || uint32_t(parent[b]) != d->joint_bone[j - 1]))
                return bad("the skeleton parent of joint_bone[" + std::to_string(j) + "] is not the joint before it");
            SpringJoint &e = t.joints[j];
            e.bone = b;
            const float *h = rest + size_t(b) * 3, *hp = rest + size_t(parent[b]) * 3;
            for (int k = 0; k < 3; ++k) {
                e.h[k] = h[k];
                if (d->joint_tail) e.t[k] = d->joint_tail[size_t(j) * 3 + k];
                else if (j + 1 < hi) e.t[k] = rest[size_t(d->joint_bone[j + 1]) * 3 + k];
                else e.t[k] = h[k] + (h[k] - hp[k]);
                if (nan(e.t[k])) return bad("joint_tail[" + std::to_string(j) + "] holds a NaN");
            }
        }
    }
    for (uint32_t j = 0; j < d->n_colliders; ++j) {
        const uint32_t b = d->collider_bone[j];
        if (is_joint[b]) return bad("collider_bone[" + std::to_string(j) + "] = " + std::to_string(b) + " is a joint of a chain");
        SpringCollider &e = t.colliders[j];
        e.bone = b;
        for (int k = 0; k < 3; ++k) e.centre[k] = d->collider_sphere[size_t(j) * 4 + k];
        e.r = d->collider_sphere[size_t(j) * 4 + 3];
        for (int k = 0; k < 4; ++k)
            if (nan(d->collider_sphere[size_t(j) * 4 + k])) return bad("collider_sphere[" + std::to_string(j) + "] holds a NaN");
    }
    *out = std::move(t);
    return MMDX_OK;
}

// One instance, every chain: the loop of the kernel's lanes, on the host.  pal: this instance's [nb][16] rows, rewritten in place;
// state: this instance's [n_joints][6].
inline void spring_step_instance(const SpringTable &t, float *pal, float *state, float dt, bool reset) {
    float centres[kSpringMaxColliders][4];
    const uint32_t nc = uint32_t(t.colliders.size());
    for (uint32_t j = 0; j < nc; ++j) {
        spring_pt(t.colliders[j].centre, pal + size_t(t.colliders[j].bone) * 16, centres[j]);
        centres[j][3] = t.colliders[j].r;
    }
    for (const SpringChain &ch : t.chains) {
        float row[16];
        for (int k = 0; k < 16; ++k) row[k] = pal[size_t(ch.anchor) * 16 + k];
        for (uint32_t j = ch.first; j < ch.first + ch.count; ++j) {
            const SpringJoint &e = t.joints[j];
            float *s = state + size_t(j) * kSpringStateFloats;
            spring_joint(row, e.h, e.t, s, s + 3, ch.stiffness, ch.drag, ch.gravity_scale, ch.radius, t.gravity, dt, reset, centres, nc);
            for (int k = 0; k < 16; ++k) pal[size_t(e.bone) * 16 + k] = row[k];
        }
    }
}

}  // namespace mmdx

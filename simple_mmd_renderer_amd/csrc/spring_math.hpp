// spring_math.hpp -- the arithmetic of mmdx_spring_step (include/mmdx.h states it, steps 1-7), once: the gfx950 kernel
// (spring_kernels.hip) and a CPU driver (tests/spring_math_driver.cpp) compile these same lines, and tests/spring_ref.py restates
// them in numpy.  Every operation is binary32 in the order written, the square root is float(sqrt(double(s))) as in
// motion_blend.hpp, there is no trigonometry; both builds pass -ffp-contract=off, so nothing is fused.
#pragma once

#include <cmath>
#include <cstdint>

#include "place_math.hpp"

#if defined(__HIPCC__)
#define MMDX_SPRING_FN __host__ __device__ __forceinline__
#define MMDX_SPRING_UNROLL _Pragma("unroll")
#else
#define MMDX_SPRING_FN inline
#define MMDX_SPRING_UNROLL
#endif

namespace mmdx {

// the values of MMDX_SPRING_MAX_JOINTS / _COLLIDERS of include/mmdx.h (spring_api.cpp asserts they agree)
constexpr uint32_t kSpringMaxJoints = 32, kSpringMaxColliders = 16;
constexpr uint32_t kSpringStateFloats = 6;      // c xyz, p xyz

// The set's device table, three arrays of 32-byte rows; every row is wave-uniform in the kernel (scalar loads).
struct alignas(16) SpringChain {
    uint32_t first, count, anchor, pad0;        // joints [first, first + count); anchor = the first joint's skeleton parent
    float stiffness, drag, gravity_scale, radius;
};
struct alignas(16) SpringJoint {
    uint32_t bone;
    float h[3], t[3];                           // rest position, tail rest point
    uint32_t pad0;
};
struct alignas(16) SpringCollider {
    uint32_t bone;
    float centre[3], r;
    uint32_t pad0, pad1, pad2;
};
static_assert(sizeof(SpringChain) == 32 && sizeof(SpringJoint) == 32 && sizeof(SpringCollider) == 32, "32-byte table rows");

MMDX_SPRING_FN bool spring_finite(float x) { return x - x == 0.0f; }

// pt(x, S): the first three columns of place_row(x0, x1, x2, 1, S)
MMDX_SPRING_FN void spring_pt(const float *x, const float *s, float *o) {
    float r[4];
    place_row(x[0], x[1], x[2], 1.0f, s, r);
    o[0] = r[0]; o[1] = r[1]; o[2] = r[2];
}

MMDX_SPRING_FN float spring_len(float d0, float d1, float d2) {
    const float s = (d0 * d0 + d1 * d1) + d2 * d2;
    return float(sqrt(double(s)));
}

// Step 4: n back onto the sphere of radius la around H; T0 when n sits on H or is not finite.  A tail that IS T0 stays T0, every
// bit: T0 is at la from H by la's own definition, and (a / la) * la need not round back to a.
MMDX_SPRING_FN void spring_constrain(float *n, const float *hh, const float *t0, float la) {
    if (n[0] == t0[0] && n[1] == t0[1] && n[2] == t0[2]) return;
    const float d0 = n[0] - hh[0], d1 = n[1] - hh[1], d2 = n[2] - hh[2];
    const float l = spring_len(d0, d1, d2);
    if (!(l > 0.0f) || !spring_finite(l)) {
        n[0] = t0[0]; n[1] = t0[1]; n[2] = t0[2];
        return;
    }
    n[0] = hh[0] + (d0 / l) * la;
    n[1] = hh[1] + (d1 / l) * la;
    n[2] = hh[2] + (d2 / l) * la;
}

// One joint, steps 1-7.  row: the parent's current row on entry (P), this joint's row on return.  c, p: the joint's state, in and
// out.  centres: [nc][4] = {C xyz (step 5's pt(centre, S[collider bone]) of this instance), r}.
MMDX_SPRING_FN void spring_joint(float *row, const float *h, const float *t, float *c, float *p, float stiffness, float drag,
                                 float gravity_scale, float radius, const float *g, float dt, bool reset,
                                 const float (*centres)[4], uint32_t nc) {
    float hh[3], t0[3];
    spring_pt(h, row, hh);
    spring_pt(t, row, t0);
    const float a0 = t0[0] - hh[0], a1 = t0[1] - hh[1], a2 = t0[2] - hh[2];
    const float la = spring_len(a0, a1, a2);
    if (!(la > 0.0f) || !spring_finite(la)) {                                                      // step 1: a degenerate segment
        for (int k = 0; k < 3; ++k) c[k] = p[k] = t0[k];
        return;
    }
    bool heal = reset;                                                                              // step 2
    for (int k = 0; k < 3; ++k) heal = heal || !spring_finite(c[k]) || !spring_finite(p[k]);
    if (heal)
        for (int k = 0; k < 3; ++k) c[k] = p[k] = t0[k];
    float n[3] = {c[0], c[1], c[2]};
    if (dt > 0.0f) {                                                                                // step 3
        const float keep = 1.0f - drag, sd = stiffness * dt, gd = gravity_scale * dt;
        for (int k = 0; k < 3; ++k) {
            n[k] = c[k] + (c[k] - p[k]) * keep;
            n[k] = n[k] + (t0[k] - c[k]) * sd;
            n[k] = n[k] + g[k] * gd;
        }
    }
    spring_constrain(n, hh, t0, la);                                                                // step 4
    MMDX_SPRING_UNROLL
    for (uint32_t j = 0; j < kSpringMaxColliders; ++j) {                                            // step 5
        if (j >= nc) continue;                                                                      // (no break: the loop unrolls whole)
        const float rr = centres[j][3] + radius;
        const float d0 = n[0] - centres[j][0], d1 = n[1] - centres[j][1], d2 = n[2] - centres[j][2];
        const float l = spring_len(d0, d1, d2);
        if (l > 0.0f && l < rr) {
            n[0] = centres[j][0] + (d0 / l) * rr;
            n[1] = centres[j][1] + (d1 / l) * rr;
            n[2] = centres[j][2] + (d2 / l) * rr;
            spring_constrain(n, hh, t0, la);
        }
    }
    for (int k = 0; k < 3; ++k) {                                                                   // step 6
        p[k] = c[k];
        c[k] = n[k];
    }
    if (n[0] == t0[0] && n[1] == t0[1] && n[2] == t0[2]) return;                                    // step 7: rigid, row = P
    const float u0 = a0 / la, u1 = a1 / la, u2 = a2 / la;
    const float v0 = (n[0] - hh[0]) / la, v1 = (n[1] - hh[1]) / la, v2 = (n[2] - hh[2]) / la;
    const float k0 = u1 * v2 - u2 * v1, k1 = u2 * v0 - u0 * v2, k2 = u0 * v1 - u1 * v0;
    const float cs = (u0 * v0 + u1 * v1) + u2 * v2;
    const float m = 1.0f + cs;
    if (!(m > 1e-6f)) {                                                                             // antiparallel
        for (int k = 0; k < 3; ++k) c[k] = p[k] = t0[k];
        return;
    }
    const float q00 = (k0 * k0) / m, q01 = (k0 * k1) / m, q02 = (k0 * k2) / m, q11 = (k1 * k1) / m, q12 = (k1 * k2) / m,
                q22 = (k2 * k2) / m;
    const float r[3][3] = {{cs + q00, q01 + k2, q02 - k1}, {q01 - k2, cs + q11, q12 + k0}, {q02 + k1, q12 - k0, cs + q22}};
    float o[16];
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) o[4 * i + j] = (row[4 * i] * r[0][j] + row[4 * i + 1] * r[1][j]) + row[4 * i + 2] * r[2][j];
        o[4 * i + 3] = 0.0f;
    }
    for (int j = 0; j < 3; ++j) o[12 + j] = hh[j] - ((h[0] * o[j] + h[1] * o[4 + j]) + h[2] * o[8 + j]);
    o[15] = 1.0f;
    for (int k = 0; k < 16; ++k) row[k] = o[k];
}

}  // namespace mmdx

// reach_math.hpp -- the arithmetic of mmdx_palette_reach (include/mmdx.h states it, steps 0-5), once: the gfx950 kernel
// (reach_kernels.hip) and a CPU driver (tests/reach_math_driver.cpp) compile these same lines, and tests/reach_ref.py restates them
// in numpy.  Every operation is binary32 in the order written, the square root is float(sqrt(double(s))) as in spring_math.hpp,
// there is no trigonometry; both builds pass -ffp-contract=off, so nothing is fused.  pt, dir, len, mul, finite and the rotation are
// those of the aim section, restated here: aim_math.hpp and spring_math.hpp stay as they are and no file that holds another kernel
// includes this header.
#pragma once

#include <cmath>
#include <cstdint>

#include "place_math.hpp"

#if defined(__HIPCC__)
#define MMDX_REACH_FN __host__ __device__ __forceinline__
#else
#define MMDX_REACH_FN inline
#endif

namespace mmdx {

// the values of MMDX_REACH_MAX_REACHES / MMDX_REACH_KEEP_END_ROTATION of include/mmdx.h (reach_api.cpp asserts they agree)
constexpr uint32_t kReachMaxReaches = 16, kReachKeepEndRotation = 1;
constexpr uint32_t kReachDepths = 3;              // C_0, C_1, C_2: the matrices of the subtrees of a, b and c
constexpr uint32_t kReachMatrixFloats = 12;       // what is kept of a matrix: its fourth column is {0, 0, 0, 1}

// The set's device table: reaches (96-byte rows, uniform over a workgroup of the kernel: scalar loads), subtree rows (8 bytes).
struct alignas(16) ReachReach {
    uint32_t a, b, c, flags;                      // upper bone, middle bone, end bone; MMDX_REACH_KEEP_END_ROTATION
    float ha[3];                                  // rest positions of a, b and c: the pivots
    uint32_t first_row;                           // subtree rows [first_row, + n_rows)
    float hb[3];
    uint32_t n_rows;
    float hc[3];
    float max_extension;
    float e[3];                                   // rest-space tip point, carried by c
    uint32_t pad0;
    float pole[3];                                // rest-space pole vector, carried by a
    uint32_t pad1;
};
struct ReachRow {
    uint32_t bone, depth;                         // a bone of the subtree of a, and the deepest of a, b, c that is it or above it: 0, 1, 2
};
static_assert(sizeof(ReachReach) == 96 && sizeof(ReachRow) == 8, "the table rows");

MMDX_REACH_FN bool reach_finite(float x) { return x - x == 0.0f; }

MMDX_REACH_FN float reach_sqrt(float s) { return float(sqrt(double(s))); }

MMDX_REACH_FN float reach_len(const float *d) { return reach_sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]); }

MMDX_REACH_FN float reach_dot(const float *a, const float *b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

// pt(x, S): the first three columns of place_row(x0, x1, x2, 1, S)
MMDX_REACH_FN void reach_pt(const float *x, const float *s, float *o) {
    float r[4];
    place_row(x[0], x[1], x[2], 1.0f, s, r);
    o[0] = r[0]; o[1] = r[1]; o[2] = r[2];
}

// dir(x, S)[c] = (x0*S[c] + x1*S[4+c]) + x2*S[8+c]
MMDX_REACH_FN void reach_dir(const float *x, const float *s, float *o) {
    for (int j = 0; j < 3; ++j) o[j] = (x[0] * s[j] + x[1] * s[4 + j]) + x[2] * s[8 + j];
}

// o = mul(a, b), every row by place_row; o is neither a nor b
MMDX_REACH_FN void reach_mul(const float *a, const float *b, float *o) {
    for (int r = 0; r < 4; ++r) place_row(a[4 * r], a[4 * r + 1], a[4 * r + 2], a[4 * r + 3], b, o + 4 * r);
}

// Step 0: the weight of a target, 0 when nothing of the instance is written
MMDX_REACH_FN float reach_weight(const float *tgt) {
    const float w = tgt[3];
    if (!(w > 0.0f) || !reach_finite(tgt[0]) || !reach_finite(tgt[1]) || !reach_finite(tgt[2]) || !reach_finite(w)) return 0.0f;
    return w < 1.0f ? w : 1.0f;
}

// rot(u, v, H): the shortest rotation from the unit vector u to the unit vector v about the pivot H, 16 floats; false: antiparallel
MMDX_REACH_FN bool reach_rot(const float *u, const float *v, const float *hh, float *ml) {
    const bool same = u[0] == v[0] && u[1] == v[1] && u[2] == v[2];                                  // the identity, exactly
    const float cs = reach_dot(u, v);
    const float k0 = u[1] * v[2] - u[2] * v[1], k1 = u[2] * v[0] - u[0] * v[2], k2 = u[0] * v[1] - u[1] * v[0];
    const float m = 1.0f + cs;
    if (!same && !(m > 1e-6f)) return false;
    const float q00 = (k0 * k0) / m, q01 = (k0 * k1) / m, q02 = (k0 * k2) / m, q11 = (k1 * k1) / m, q12 = (k1 * k2) / m,
                q22 = (k2 * k2) / m;
    const float r[3][3] = {{cs + q00, q01 + k2, q02 - k1}, {q01 - k2, cs + q11, q12 + k0}, {q02 + k1, q12 - k0, cs + q22}};
    for (int i = 0; i < 3; ++i) {                                                                    // (selects, element by element: a
        for (int j = 0; j < 3; ++j) ml[4 * i + j] = same ? (i == j ? 1.0f : 0.0f) : r[i][j];         //  branch around whole-array writes
        ml[4 * i + 3] = 0.0f;                                                                        //  has cost the kernel scratch)
    }
    for (int j = 0; j < 3; ++j) ml[12 + j] = same ? 0.0f : hh[j] - ((hh[0] * r[0][j] + hh[1] * r[1][j]) + hh[2] * r[2][j]);
    ml[15] = 1.0f;
    return true;
}

// Steps 1-5 for one reach of one instance.  ra, rb, rc: the rows of a, b and c as read from the palette; g, w: the target and its
// weight after step 0 (w > 0); c0, c1, c2: 16 floats each.  true: the three matrices are set; false: nothing is written for this
// (instance, reach).
MMDX_REACH_FN bool reach_solve(const float *ra, const float *rb, const float *rc, const ReachReach &k, const float *g, float w, float *c0,
                               float *c1, float *c2) {
    const bool keep = (k.flags & kReachKeepEndRotation) != 0;
    float A[3], B[3], K[3], T[3], G[3], Gw[3];                                                       // ---- 1. points
    reach_pt(k.ha, ra, A);
    reach_pt(k.hb, rb, B);
    reach_pt(k.hc, rc, K);
    reach_pt(k.e, rc, T);
    for (int j = 0; j < 3; ++j) {
        if (keep) {
            G[j] = g[j] - (T[j] - K[j]);
            T[j] = K[j];
        } else {
            G[j] = g[j];
        }
    }
    for (int j = 0; j < 3; ++j) Gw[j] = w >= 1.0f ? G[j] : T[j] + (G[j] - T[j]) * w;
    float ba[3], tb[3], dv[3];
    for (int j = 0; j < 3; ++j) {
        ba[j] = B[j] - A[j];
        tb[j] = T[j] - B[j];
        dv[j] = Gw[j] - A[j];
    }
    const float l1 = reach_len(ba), l2 = reach_len(tb), d = reach_len(dv);
    if (!(l1 > 0.0f) || !(l2 > 0.0f) || !(d > 0.0f) || !reach_finite(l1) || !reach_finite(l2) || !reach_finite(d)) return false;
    const float s = l1 + l2, lmax = s * k.max_extension, lmin = fabsf(l1 - l2) + (s - lmax);          // ---- 2. clamp
    if (!(lmin <= lmax)) return false;
    float dc = d < lmin ? lmin : d;
    dc = dc > lmax ? lmax : dc;
    float dh[3], Gc[3];
    for (int j = 0; j < 3; ++j) {
        dh[j] = dv[j] / d;
        Gc[j] = A[j] + dh[j] * dc;
    }
    const float x = ((l1 * l1 - l2 * l2) + dc * dc) / (2.0f * dc);                                   // ---- 3. elbow
    const float y2 = l1 * l1 - x * x;
    const float y = y2 > 0.0f ? reach_sqrt(y2) : 0.0f;
    float p[3];
    float bd = reach_dot(ba, dh);
    for (int j = 0; j < 3; ++j) p[j] = ba[j] - dh[j] * bd;
    float lp = reach_len(p);
    if (!(lp > 1e-4f * l1)) {                                                                        // straight: the pole
        float b[3];
        reach_dir(k.pole, ra, b);
        bd = reach_dot(b, dh);
        for (int j = 0; j < 3; ++j) p[j] = b[j] - dh[j] * bd;
        lp = reach_len(p);
        if (!(lp > 0.0f)) return false;
    }
    float nb[3], u1[3], v1[3];
    for (int j = 0; j < 3; ++j) nb[j] = dh[j] * x + (p[j] / lp) * y;
    const float ln = reach_len(nb);
    for (int j = 0; j < 3; ++j) {
        v1[j] = nb[j] / ln;
        u1[j] = ba[j] / l1;
    }
    if (!reach_rot(u1, v1, A, c0)) return false;
    float pb[16], pc[16], B1[3], T1[3], t1[3], g1[3], u2[3], v2[3], mb[16];                           // ---- 4. forearm
    reach_mul(rb, c0, pb);
    reach_mul(rc, c0, pc);
    reach_pt(k.hb, pb, B1);
    reach_pt(keep ? k.hc : k.e, pc, T1);
    for (int j = 0; j < 3; ++j) {
        t1[j] = T1[j] - B1[j];
        g1[j] = Gc[j] - B1[j];
    }
    const float lt = reach_len(t1), lg = reach_len(g1);
    if (!(lt > 0.0f) || !(lg > 0.0f) || !reach_finite(lt) || !reach_finite(lg)) return false;
    for (int j = 0; j < 3; ++j) {
        u2[j] = t1[j] / lt;
        v2[j] = g1[j] / lg;
    }
    if (!reach_rot(u2, v2, B1, mb)) return false;
    reach_mul(c0, mb, c1);
    c1[3] = c1[7] = c1[11] = 0.0f;                                                                   // (what the product gives for finite c0, mb)
    c1[15] = 1.0f;
    float K1[3] = {0.0f, 0.0f, 0.0f};                                                                // ---- 5. end bone
    if (keep) {
        reach_mul(rc, c1, pc);
        reach_pt(k.hc, pc, K1);
    }
    for (int r = 0; r < 3; ++r) {                                                                    // (selects, element by element: a
        for (int j = 0; j < 3; ++j) c2[4 * r + j] = keep ? (r == j ? 1.0f : 0.0f) : c1[4 * r + j];   //  branch around whole-array writes
        c2[4 * r + 3] = 0.0f;                                                                        //  has cost the kernel scratch)
        c2[12 + r] = keep ? K1[r] - K[r] : c1[12 + r];
    }
    c2[15] = 1.0f;
    return true;
}

}  // namespace mmdx

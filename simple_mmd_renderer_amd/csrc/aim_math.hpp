// aim_math.hpp -- the arithmetic of mmdx_palette_aim (include/mmdx.h states it, steps 0-2), once: the gfx950 kernel
// (aim_kernels.hip) and a CPU driver (tests/aim_math_driver.cpp) compile these same lines, and tests/aim_ref.py restates them in
// numpy.  Every operation is binary32 in the order written, the square root is float(sqrt(double(s))) as in spring_math.hpp, there
// is no trigonometry; both builds pass -ffp-contract=off, so nothing is fused.  The rotation is the formula of spring step 7,
// restated here: spring_math.hpp stays as it is and no file that holds another kernel includes this header.
#pragma once

#include <cmath>
#include <cstdint>

#include "place_math.hpp"

#if defined(__HIPCC__)
#define MMDX_AIM_FN __host__ __device__ __forceinline__
#else
#define MMDX_AIM_FN inline
#endif

namespace mmdx {

// the values of MMDX_AIM_MAX_AIMS / _LINKS of include/mmdx.h (aim_api.cpp asserts they agree)
constexpr uint32_t kAimMaxAims = 16, kAimMaxLinks = 4;
constexpr uint32_t kAimMatrixFloats = 12;       // what is kept of a cumulative matrix: its fourth column is {0, 0, 0, 1}

// The set's device table: aims (48-byte rows), links (32-byte rows), subtree rows (8 bytes).  Aims and links are uniform over a
// workgroup of the kernel (scalar loads).
struct alignas(16) AimAim {
    uint32_t first_link, n_links, eye_bone, first_row, n_rows;      // links [first_link, + n_links), subtree rows [first_row, + n_rows)
    float e[3], f[3];                                                // rest-space eye point and forward vector, carried by eye_bone
    uint32_t pad0;
};
struct alignas(16) AimLink {
    uint32_t bone;
    float h[3];                                 // rest position of the bone: the pivot
    float share, cos_limit, sin_limit;          // sin_limit = float(sqrt(double(1.0f - cos_limit*cos_limit)))
    uint32_t pad0;
};
struct AimRow {
    uint32_t bone, depth;                       // a bone of the subtree of the aim's first link, and the deepest link that is it or above it
};
static_assert(sizeof(AimAim) == 48 && sizeof(AimLink) == 32 && sizeof(AimRow) == 8, "the table rows");

MMDX_AIM_FN bool aim_finite(float x) { return x - x == 0.0f; }

MMDX_AIM_FN float aim_len(float d0, float d1, float d2) {
    const float s = (d0 * d0 + d1 * d1) + d2 * d2;
    return float(sqrt(double(s)));
}

// pt(x, S): the first three columns of place_row(x0, x1, x2, 1, S)
MMDX_AIM_FN void aim_pt(const float *x, const float *s, float *o) {
    float r[4];
    place_row(x[0], x[1], x[2], 1.0f, s, r);
    o[0] = r[0]; o[1] = r[1]; o[2] = r[2];
}

// o = mul(a, b), every row by place_row; o is neither a nor b
MMDX_AIM_FN void aim_mul(const float *a, const float *b, float *o) {
    for (int r = 0; r < 4; ++r) place_row(a[4 * r], a[4 * r + 1], a[4 * r + 2], a[4 * r + 3], b, o + 4 * r);
}

// Step 0: the weight of a target, 0 when nothing of the instance is written
MMDX_AIM_FN float aim_weight(const float *tgt) {
    const float w = tgt[3];
    if (!(w > 0.0f) || !aim_finite(tgt[0]) || !aim_finite(tgt[1]) || !aim_finite(tgt[2]) || !aim_finite(w)) return 0.0f;
    return w < 1.0f ? w : 1.0f;
}

// Step 1 for one link.  p_in, q_in: the rows of the link bone and of the eye bone as read from the palette; g, w: the target and
// its weight after step 0; c: the cumulative matrix, 16 floats, meaningful when `set`.  true: the link was applied and c is the new
// cumulative matrix; false: the link was skipped and c is as it was.
MMDX_AIM_FN bool aim_link(const float *p_in, const float *q_in, const AimLink &k, const float *e, const float *f, const float *g,
                          float w, float *c, bool set) {
    float p[16], q[16];
    if (set) {
        aim_mul(p_in, c, p);
        aim_mul(q_in, c, q);
    } else {
        for (int i = 0; i < 16; ++i) {
            p[i] = p_in[i];
            q[i] = q_in[i];
        }
    }
    float hh[3], ee[3], a[3], d[3];
    aim_pt(k.h, p, hh);
    aim_pt(e, q, ee);
    for (int j = 0; j < 3; ++j) {
        a[j] = (f[0] * q[j] + f[1] * q[4 + j]) + f[2] * q[8 + j];
        d[j] = g[j] - ee[j];
    }
    const float la = aim_len(a[0], a[1], a[2]), ld = aim_len(d[0], d[1], d[2]);
    if (!(la > 0.0f) || !(ld > 0.0f) || !aim_finite(la) || !aim_finite(ld)) return false;
    const float u[3] = {a[0] / la, a[1] / la, a[2] / la}, v[3] = {d[0] / ld, d[1] / ld, d[2] / ld};
    if (u[0] == v[0] && u[1] == v[1] && u[2] == v[2]) return false;
    float v2[3];
    const float t = k.share * w;
    if (t >= 1.0f) {
        for (int j = 0; j < 3; ++j) v2[j] = v[j];
    } else {
        float n[3];
        for (int j = 0; j < 3; ++j) n[j] = u[j] + (v[j] - u[j]) * t;
        const float ln = aim_len(n[0], n[1], n[2]);
        if (!(ln > 0.0f)) return false;
        for (int j = 0; j < 3; ++j) v2[j] = n[j] / ln;
    }
    float cs = (u[0] * v2[0] + u[1] * v2[1]) + u[2] * v2[2];
    if (cs < k.cos_limit) {                                                                         // the limit
        float s[3];
        for (int j = 0; j < 3; ++j) s[j] = v2[j] - u[j] * cs;
        const float lp = aim_len(s[0], s[1], s[2]);
        if (!(lp > 0.0f)) return false;
        for (int j = 0; j < 3; ++j) v2[j] = u[j] * k.cos_limit + (s[j] / lp) * k.sin_limit;
        cs = (u[0] * v2[0] + u[1] * v2[1]) + u[2] * v2[2];
    }
    const float k0 = u[1] * v2[2] - u[2] * v2[1], k1 = u[2] * v2[0] - u[0] * v2[2], k2 = u[0] * v2[1] - u[1] * v2[0];
    const float m = 1.0f + cs;
    if (!(m > 1e-6f)) return false;                                                                 // antiparallel
    const float q00 = (k0 * k0) / m, q01 = (k0 * k1) / m, q02 = (k0 * k2) / m, q11 = (k1 * k1) / m, q12 = (k1 * k2) / m,
                q22 = (k2 * k2) / m;
    const float r[3][3] = {{cs + q00, q01 + k2, q02 - k1}, {q01 - k2, cs + q11, q12 + k0}, {q02 + k1, q12 - k0, cs + q22}};
    float ml[16];
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) ml[4 * i + j] = r[i][j];
        ml[4 * i + 3] = 0.0f;
    }
    for (int j = 0; j < 3; ++j) ml[12 + j] = hh[j] - ((hh[0] * r[0][j] + hh[1] * r[1][j]) + hh[2] * r[2][j]);
    ml[15] = 1.0f;
    if (set) {
        float o[16];
        aim_mul(c, ml, o);
        for (int i = 0; i < 16; ++i) c[i] = o[i];
        c[3] = c[7] = c[11] = 0.0f;                                                                 // (what the product gives for finite c)
        c[15] = 1.0f;
    } else {
        for (int i = 0; i < 16; ++i) c[i] = ml[i];
    }
    return true;
}

}  // namespace mmdx

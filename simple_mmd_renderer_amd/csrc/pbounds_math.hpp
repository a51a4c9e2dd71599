// pbounds_math.hpp -- the arithmetic of mmdx_palette_bounds (include/mmdx.h), once: the gfx950 kernel (pbounds_kernels.hip) and a
// CPU driver (tests/pbounds_math_driver.cpp) compile these same lines.  Every operation is binary32 in the order written; both
// builds pass -ffp-contract=off, so nothing is fused.  kernels.hip keeps its own f2key / key2f: moving them has changed existing
// kernels' code before.
#pragma once

#include <climits>

#if defined(__HIPCC__)
#define MMDX_PB_FN __host__ __device__ __forceinline__
#else
#define MMDX_PB_FN inline
#endif

namespace mmdx {

// min / max of the contract: the first operand unless the second is strictly smaller / larger (so a NaN in the second operand is
// ignored, a NaN in the first is returned; both products of one matrix element are NaN together unless 0 * inf is involved)
MMDX_PB_FN float pb_min(float a, float b) { return b < a ? b : a; }
MMDX_PB_FN float pb_max(float a, float b) { return a < b ? b : a; }
MMDX_PB_FN float pb_abs(float a) { return __builtin_fabsf(a); }

// One table row against one skinning matrix: lo, hi, reach [3]; m [16] row-vector layout (elements 3, 7, 11 and 15 are not read);
// ms = morph_scale -> blo, bhi [3], the padded box of the row's vertices in the matrix's target space.
MMDX_PB_FN void pbounds_row(const float *lo, const float *hi, const float *reach, float ms, const float *m, float eps, float *blo,
                            float *bhi) {
    float L[3], H[3];
    for (int k = 0; k < 3; ++k) {
        const float g = reach[k] * ms;
        L[k] = lo[k] - g;
        H[k] = hi[k] + g;
    }
    for (int j = 0; j < 3; ++j) {
        const float p0l = L[0] * m[j], p0h = H[0] * m[j];
        const float p1l = L[1] * m[4 + j], p1h = H[1] * m[4 + j];
        const float p2l = L[2] * m[8 + j], p2h = H[2] * m[8 + j];
        const float t = m[12 + j];
        const float mn = ((pb_min(p0l, p0h) + pb_min(p1l, p1h)) + pb_min(p2l, p2h)) + t;
        const float mx = ((pb_max(p0l, p0h) + pb_max(p1l, p1h)) + pb_max(p2l, p2h)) + t;
        const float a = ((pb_max(pb_abs(p0l), pb_abs(p0h)) + pb_max(pb_abs(p1l), pb_abs(p1h))) + pb_max(pb_abs(p2l), pb_abs(p2h))) +
                        pb_abs(t);
        const float pad = a * eps;
        blo[j] = mn - pad;
        bhi[j] = mx + pad;
    }
}

// Ordered integer keys: signed order of the keys = numeric order of the floats, -0 just below +0; pb_unkey(pb_key(x)) == x bit for
// bit.  The fold over the rows is an integer min / max of keys, so it does not depend on the reduction tree.
MMDX_PB_FN int pb_key(float x) {
    const int b = __builtin_bit_cast(int, x);
    return b ^ ((b >> 31) & 0x7fffffff);
}
MMDX_PB_FN float pb_unkey(int k) { return __builtin_bit_cast(float, k ^ ((k >> 31) & 0x7fffffff)); }

struct PBoundsAcc {
    int kmin[3], kmax[3];      // the identities are INT_MAX / INT_MIN: no float's key
    bool nan;                  // some blo / bhi was NaN: the whole row becomes NaN
};
MMDX_PB_FN void pbounds_init(PBoundsAcc &a) {
    for (int c = 0; c < 3; ++c) { a.kmin[c] = INT_MAX; a.kmax[c] = INT_MIN; }
    a.nan = false;
}
MMDX_PB_FN void pbounds_fold(PBoundsAcc &a, const float *blo, const float *bhi) {
    for (int c = 0; c < 3; ++c) {
        a.nan = a.nan || blo[c] != blo[c] || bhi[c] != bhi[c];
        const int kl = pb_key(blo[c]), kh = pb_key(bhi[c]);
        a.kmin[c] = kl < a.kmin[c] ? kl : a.kmin[c];
        a.kmax[c] = kh > a.kmax[c] ? kh : a.kmax[c];
    }
}
// The row as stored: {min xyz, max xyz} * pos_scale, or six quiet NaNs for a NaN anywhere and for an empty table
MMDX_PB_FN void pbounds_finish(const int *kmin, const int *kmax, bool nan_or_empty, float pos_scale, float *out) {
    const float qnan = __builtin_bit_cast(float, 0x7fc00000);
    for (int c = 0; c < 3; ++c) {
        out[c] = nan_or_empty ? qnan : pb_unkey(kmin[c]) * pos_scale;
        out[3 + c] = nan_or_empty ? qnan : pb_unkey(kmax[c]) * pos_scale;
    }
}

}  // namespace mmdx

// ground_math.hpp -- the arithmetic of mmdx_ground_place and mmdx_ground_targets (include/mmdx.h states it), once: the gfx950
// kernels (ground_kernels.hip) and a CPU driver (tests/ground_math_driver.cpp) compile these same lines, and tests/ground_ref.py
// restates them in numpy.  Every operation is binary32 in the order written; both builds pass -ffp-contract=off, so nothing is
// fused.  There is no square root and no trigonometry.  No file that holds another kernel includes this header.
#pragma once

#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define MMDX_GROUND_FN __host__ __device__ __forceinline__
#else
#define MMDX_GROUND_FN inline
#endif

namespace mmdx {

// the values of MMDX_GROUND_MAX_FEET / MMDX_GROUND_MIN_SAMPLES / _MAX_SAMPLES of include/mmdx.h (ground_api.cpp asserts they agree)
constexpr uint32_t kGroundMaxFeet = 8, kGroundMinSamples = 2, kGroundMaxSamples = 8192;
constexpr uint32_t kGroundPoseFloats = 8;         // MMDX_POSE_FLOATS: a placement

// The field without its heights: 24 bytes, a kernel argument (uniform: scalar registers).  heights are [nz][nx] floats.
struct GroundField {
    uint32_t nx, nz;                              // 2 .. 8192 each: nz * nx <= 2^26 samples, a 32-bit index
    float origin_x, origin_z, cell_x, cell_z;     // finite; cells > 0
};

MMDX_GROUND_FN bool ground_finite(float x) { return x - x == 0.0f; }

// "Cell and fraction" along one axis: x -> the cell i in [0, n-2] and the fraction f in [0, 1] (or -0).  false: the sample FAILS.
MMDX_GROUND_FN bool ground_axis(float x, float origin, float cell, uint32_t n, uint32_t &i, float &f) {
    float u = (x - origin) / cell;
    if (!ground_finite(u)) return false;
    const float top = float(n - 1);
    u = u < 0.0f ? 0.0f : u;
    u = u > top ? top : u;
    i = uint32_t(u);
    if (i > n - 2) i = n - 2;
    f = u - float(i);
    return true;
}

// h(x, z): four gathers and the barycentric form of the cell's triangle.  false: the sample FAILS and h is untouched.
MMDX_GROUND_FN bool ground_height(const GroundField &g, const float *H, float x, float z, float &h) {
    uint32_t iu, iv;
    float fu, fv;
    if (!ground_axis(x, g.origin_x, g.cell_x, g.nx, iu, fu)) return false;
    if (!ground_axis(z, g.origin_z, g.cell_z, g.nz, iv, fv)) return false;
    const float *row = H + size_t(iv) * g.nx + iu;
    const float h00 = row[0], h10 = row[1], h01 = row[g.nx], h11 = row[g.nx + 1];
    if (fu + fv <= 1.0f)
        h = (h00 * ((1.0f - fu) - fv) + h10 * fu) + h01 * fv;
    else
        h = (h11 * ((fu + fv) - 1.0f) + h10 * (1.0f - fv)) + h01 * (1.0f - fu);
    return true;
}

// mmdx_ground_place, one instance: p its placement (only p[1] is ever written), drop its drop or nullptr.
MMDX_GROUND_FN void ground_place_instance(const GroundField &g, const float *H, float *p, const float *drop, float y_offset) {
    float h0;
    if (!ground_height(g, H, p[0], p[2], h0)) return;
    if (drop) {
        const float d = *drop;
        if (!ground_finite(d)) return;
        p[1] = (h0 + y_offset) + d;
    } else {
        p[1] = h0 + y_offset;
    }
}

MMDX_GROUND_FN void ground_store4(float *dst, float a, float b, float c, float d) {
#if defined(__HIP_DEVICE_COMPILE__)
    *reinterpret_cast<float4 *>(dst) = make_float4(a, b, c, d);          // (out_targets is 16-byte aligned: one store)
#else
    dst[0] = a; dst[1] = b; dst[2] = c; dst[3] = d;
#endif
}

// mmdx_ground_targets, one instance: p its placement (read only), points its foot 0 (foot f: + f*slab_stride), out its target of
// foot 0 (foot f: + f*out_slab), out_drop its drop or nullptr.
MMDX_GROUND_FN void ground_targets_instance(const GroundField &g, const float *H, const float *p, const float *points, size_t slab_stride,
                                            uint32_t n_feet, float max_step, float max_drop, float *out, size_t out_slab, float *out_drop) {
    const float ty = p[1];
    float h0 = 0.0f;
    const bool want_drop = out_drop != nullptr;
    const bool h0_ok = want_drop && ground_height(g, H, p[0], p[2], h0);
    float m = 0.0f;
    for (uint32_t f = 0; f < n_feet; ++f) {
        const float *P = points + f * slab_stride;
        const float px = P[0], py = P[1], pz = P[2];
        float hf = 0.0f;
        const bool sampled = ground_height(g, H, px, pz, hf);
        float *t = out + f * out_slab;
        if (sampled && ground_finite(px) && ground_finite(py) && ground_finite(pz) && ground_finite(ty)) {
            float dy = hf - ty;
            dy = dy < -max_step ? -max_step : dy;
            dy = dy > max_step ? max_step : dy;
            ground_store4(t, px, py + dy, pz, 1.0f);
        } else {
            ground_store4(t, 0.0f, 0.0f, 0.0f, 0.0f);
        }
        if (sampled && h0_ok) {
            const float d = hf - h0;
            m = d < m ? d : m;
        }
    }
    if (want_drop) {
        float r = m < 0.0f ? m : 0.0f;
        r = r < -max_drop ? -max_drop : r;
        *out_drop = r;
    }
}

}  // namespace mmdx

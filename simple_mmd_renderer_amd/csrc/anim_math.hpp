// anim_math.hpp -- the arithmetic of mmdx_animator_advance (include/mmdx.h states it), once: the gfx950 kernel (anim_kernels.hip)
// and a CPU driver (tests/anim_math_driver.cpp) compile these same lines, and tests/animator_ref.py restates them in numpy.
// IEEE operations only -- add, multiply, divide, compare, conversions between double, float and integer -- and no libm, so host
// and device agree bit for bit; both builds pass -ffp-contract=off, so nothing is fused.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define MMDX_ANIM_FN __host__ __device__ __forceinline__
#else
#define MMDX_ANIM_FN inline
#endif

namespace mmdx {

// the values of MMDX_CLIP_NONE, MMDX_ANIM_NO_REQUEST and MMDX_ANIM_* of include/mmdx.h (anim_api.cpp asserts they agree)
constexpr uint32_t kAnimClipNone = 0xFFFFFFFFu, kAnimNoRequest = 0xFFFFFFFEu;
enum : uint32_t { kAnimLoop = 0, kAnimHold = 1, kAnimThen = 2 };

// the per-clip table, [n_clips] each
struct AnimClips {
    const double *length;                       // seconds, resolved (never NaN or negative)
    const uint32_t *mode, *next;
    const float *fade;
    uint32_t n_clips;
};

// one instance's row of the eleven state arrays
struct AnimLane {
    uint32_t clip_a, clip_b;
    double time_a, time_b;
    float weight, speed, fade_rate;
    uint32_t req_clip;
    float req_fade;
    double req_time;
    uint32_t loops;
};

// floor(x) from a truncating conversion: every double of magnitude >= 2^52 is an integer already (NaN and the infinities pass)
MMDX_ANIM_FN double anim_floor(double x) {
    if (!(x > -4503599627370496.0 && x < 4503599627370496.0)) return x;
    const double t = double(static_cast<long long>(x));
    return t > x ? t - 1.0 : t;
}

// t into [0, L]; a NaN becomes 0
MMDX_ANIM_FN double anim_clamp(double t, double L) { return t > L ? L : (t >= 0.0 ? t : 0.0); }

// the clock of clip c after a step; *wrapped = 1 when a looping clock left [0, L) and was folded back
MMDX_ANIM_FN double anim_wrap(const AnimClips &k, uint32_t c, double t, uint32_t *wrapped) {
    *wrapped = 0;
    if (c >= k.n_clips) return t;               // the rest pose has no length
    const double L = k.length[c];
    if (k.mode[c] != kAnimLoop) return anim_clamp(t, L);
    if (!(L > 0.0)) return 0.0;
    if (t < 0.0 || t >= L) {
        t = t - anim_floor(t / L) * L;
        t = anim_clamp(t, L);
        *wrapped = 1;
    }
    return t;
}

// one step of one instance; dt is not NaN (the callers return before)
MMDX_ANIM_FN void anim_advance(const AnimClips &k, AnimLane &s, double dt) {
    const double step = double(s.speed) * dt;
    uint32_t wrapped, unused;
    s.time_a = anim_wrap(k, s.clip_a, s.time_a + step, &wrapped);
    s.loops += wrapped;
    if (s.fade_rate > 0.0f) {
        s.time_b = anim_wrap(k, s.clip_b, s.time_b + step, &unused);
        const float grown = float(dt) * s.fade_rate;
        s.weight = s.weight + grown;
        if (!(s.weight >= 0.0f)) s.weight = 0.0f;
        if (s.weight > 1.0f - 1e-7f) {          // the blend's "row is B" threshold (motion_blend.hpp): b becomes a
            s.clip_a = s.clip_b;
            s.time_a = s.time_b;
            s.clip_b = kAnimClipNone;
            s.time_b = 0.0;
            s.weight = 0.0f;
            s.fade_rate = 0.0f;
        }
    }
    if (s.fade_rate == 0.0f) {
        bool go = false;
        uint32_t c = 0;
        float fade = 0.0f;
        double t0 = 0.0;
        if (s.req_clip != kAnimNoRequest) {
            go = true; c = s.req_clip; fade = s.req_fade; t0 = s.req_time;
        } else if (s.clip_a < k.n_clips && k.mode[s.clip_a] == kAnimThen &&
                   s.time_a >= k.length[s.clip_a] - double(k.fade[s.clip_a])) {
            go = true; c = k.next[s.clip_a]; fade = k.fade[s.clip_a];
        }
        if (go) {
            if (!(fade > 0.0f)) {
                s.clip_a = c;
                s.time_a = t0;
            } else {
                s.clip_b = c;
                s.time_b = t0;
                s.weight = 0.0f;
                s.fade_rate = 1.0f / fade;
            }
            s.req_clip = kAnimNoRequest;
        }
    }
}

}  // namespace mmdx

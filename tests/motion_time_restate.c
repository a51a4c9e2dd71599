/* tests/motion_time_restate.c -- TEST INFRASTRUCTURE ONLY: a from-scratch restatement of libmmd's time-based track
 * evaluation, Motion::GetBonePose(name, double time) and GetMorphPose(name, double time)
 * (L/motion/motion_impl.inl:321-380, :426-465), for the randomized GPU tests (the real libmmd is not there).
 * Compiled at test time by tests/motion_time_ref.py with plain gcc -O2 -ffp-contract=off (scalar IEEE double and
 * float, as the reference's own build).  The curve set-up and lookup are the oracle's (oracle/mmdx_oracle.c,
 * #included); what is new here is the time path:
 *   dframe = time * 30.0 (double); first key if !(first < dframe) (NaN too: undefined in the reference, the device
 *   takes the first key), last key if last <= dframe; bracket = upper_bound((uint32_t)dframe);
 *   bary = (float)((dframe - left) / (right - left)) in double; no exact-hit shortcut. */
#include "../oracle/mmdx_oracle.c"

/* keys l < r bracket the instant: the left key's curves, translation lerp and NLerp (L/util/math_impl.inl:1260-1282) */
static void blend_pose(const float *tr, const float *rot, const int8_t *interp, uint32_t l, uint32_t r, float bary,
                       float *t, float *q) {
    const float *lt = tr + 3 * (size_t)l, *rt = tr + 3 * (size_t)r;
    const float *lq = rot + 4 * (size_t)l, *rq = rot + 4 * (size_t)r;
    curve_t cv;
    float lambda;
    for (int c = 0; c < 3; ++c) {
        curve_setup(interp + 64 * (size_t)l + 16 * c, &cv);
        lambda = curve_eval(&cv, bary);
        t[c] = lt[c] * (1 - lambda) + rt[c] * lambda;
    }
    curve_setup(interp + 64 * (size_t)l + 48, &cv);
    lambda = curve_eval(&cv, bary);
    if (lambda < (float)MMDX_EPS_D) {
        memcpy(q, lq, 16);
    } else if (lambda > (1.0f - (float)MMDX_EPS_D)) {
        memcpy(q, rq, 16);
    } else {
        const float dot = lq[0] * rq[0] + lq[1] * rq[1] + lq[2] * rq[2] + lq[3] * rq[3];
        const float a = 1.0f - lambda;
        float v[4];
        for (int c = 0; c < 4; ++c) {
            const float x = a * lq[c], y = lambda * rq[c];
            v[c] = dot < 0.0f ? x - y : x + y;
        }
        const float norm = (float)sqrt((double)(v[0] * v[0] + v[1] * v[1] + v[2] * v[2] + v[3] * v[3]));
        const float inv = 1.0f / norm;
        for (int c = 0; c < 4; ++c) q[c] = v[c] * inv;
    }
}

/* the key to copy (0 / n-1), or n with *l, *r the bracketing keys and *bary the position between them */
static uint32_t locate(uint32_t n, const uint32_t *frames, double time, uint32_t *l, uint32_t *r, float *bary) {
    const double dframe = time * 30.0;
    if (!((double)frames[0] < dframe)) return 0;
    if ((double)frames[n - 1] <= dframe) return n - 1;
    const uint32_t s = (uint32_t)dframe;              /* size_t(dframe): inside [first, last) here */
    uint32_t k = 0;
    while (frames[k] <= s) ++k;                         /* upper_bound */
    *r = k;
    *l = k - 1;
    *bary = (float)((dframe - (double)frames[*l]) / (double)(frames[*r] - frames[*l]));
    return n;
}

/* One bone track (as mmdx_oracle_bone_pose) at `time` seconds; out = t.xyz, 0, q.xyzw. */
void mt_bone_pose_time(uint32_t n, const uint32_t *frames, const float *tr, const float *rot, const int8_t *interp,
                       double time, float *out) {
    float t[3] = {0.0f, 0.0f, 0.0f}, q[4] = {0.0f, 0.0f, 0.0f, 1.0f};
    if (n) {
        uint32_t l = 0, r = 0;
        float bary = 0.0f;
        const uint32_t k = locate(n, frames, time, &l, &r, &bary);
        if (k < n) {
            memcpy(t, tr + 3 * (size_t)k, 12);
            memcpy(q, rot + 4 * (size_t)k, 16);
        } else {
            blend_pose(tr, rot, interp, l, r, bary, t, q);
        }
    }
    out[0] = t[0]; out[1] = t[1]; out[2] = t[2]; out[3] = 0.0f;
    memcpy(out + 4, q, 16);
}

/* Every model morph (as mmdx_oracle_morph_tracks) at times[i] seconds -> out[ni][nm]; no track: 0. */
void mt_morph_tracks_time(uint32_t nm, const uint32_t *key_off, const uint32_t *frames, const float *weights, uint32_t ni,
                          const double *times, float *out) {
    for (uint32_t i = 0; i < ni; ++i) {
        for (uint32_t m = 0; m < nm; ++m) {
            const uint32_t b = key_off[m], e = key_off[m + 1];
            float w = 0.0f;
            if (e > b) {
                uint32_t l = 0, r = 0;
                float bary = 0.0f;
                const uint32_t k = locate(e - b, frames + b, times[i], &l, &r, &bary);
                if (k < e - b) {
                    w = weights[b + k];
                } else {
                    const float x = weights[b + l] * (1 - bary);   /* the weight curve is linear: lambda = bary */
                    const float y = weights[b + r] * bary;
                    w = x + y;
                }
            }
            out[(size_t)i * nm + m] = w;
        }
    }
}

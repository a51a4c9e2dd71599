// tests/motion_blend_driver.cpp -- TEST INFRASTRUCTURE ONLY: the cross-fade between two clips (include/mmdx.h,
// mmdx_motion_blend_args) computed by the real libmmd.  The two rows are Motion::GetBonePose / GetMorphPose(name, double time)
// (L/motion/motion_impl.inl:321-380, :426-465) of two mmd::Motions; the blend is what the reference does between two keys,
// applied between the two rows: the translation by the lerp of motion_impl.inl:364-372 (restated here, the same float
// arithmetic), the rotation by mmd::NLerp(qa, qb)[w] (L/util/math_impl.inl:1260-1282), the morph weight by the lerp of
// motion_impl.inl:462 (restated).  NLerp's short circuits are applied to the whole row first (!(w >= eps): the row is A; w > 1 - eps: the row is B), so NLerp is only entered on its middle
// branch.  libmmd is #included by path at build time (tests/motion_blend_ref.py compiles this file with g++ -O2
// -ffp-contract=off); nothing built from it is committed.  (L/ = 3rd_party/libmmd/include/mmd/)

// The include order of oracle/ref_harness.cpp and of the viewer: <math.h> / <stdlib.h> before mmd.hxx, so
// Bezier::interpolate's unqualified `abs` binds to the float overload (otherwise every curve collapses).
#include <math.h>
#include <stdlib.h>

#include <mmd/mmd.hxx>

#include <cstdint>
#include <exception>
#include <string>

namespace {

const uint32_t kClipNone = 0xFFFFFFFFu;

struct Pose {
    mmd::Vector3f t;
    mmd::Vector4f q;
};

// what MotionPlayer::SeekTime leaves in a poser for this bone: the track at `time`, or ResetPosing's pose without a track / a clip
Pose pose_of(void *const *motions, uint32_t n_motions, uint32_t clip, const std::wstring &key, double time) {
    Pose p;
    p.t.p.x = p.t.p.y = p.t.p.z = 0.f;
    p.q.v[0] = p.q.v[1] = p.q.v[2] = 0.f;
    p.q.v[3] = 1.f;
    if (clip == kClipNone || clip >= n_motions) return p;
    mmd::Motion *m = static_cast<mmd::Motion *>(motions[clip]);
    if (!m->IsBoneRegistered(key)) return p;
    const mmd::Motion::BonePose bp = m->GetBonePose(key, time);
    p.t = bp.GetTranslation();
    p.q = bp.GetRotation();
    return p;
}

float rate_of(void *const *motions, uint32_t n_motions, uint32_t clip, const std::wstring &key, double time) {
    if (clip == kClipNone || clip >= n_motions) return 0.f;
    mmd::Motion *m = static_cast<mmd::Motion *>(motions[clip]);
    if (!m->IsMorphRegistered(key)) return 0.f;
    return m->GetMorphPose(key, time).GetWeight();
}

}  // namespace

extern "C" {

// VmdReader + Motion of a .vmd file; nullptr on a read error
void *mbd_load(const char *path) {
    mmd::Motion *m = new mmd::Motion;
    try {
        std::string p(path);
        mmd::FileReader file(std::wstring(p.begin(), p.end()));
        mmd::VmdReader(file).ReadMotion(*m);
    } catch (const std::exception &) {
        delete m;
        return nullptr;
    }
    return m;
}

void mbd_destroy(void *h) { delete static_cast<mmd::Motion *>(h); }

// Row i of the bone stored under the Shift-JIS name: clip clips_a[i] at times_a[i] blended with clip clips_b[i] at times_b[i]
// by w[i] -> out[i][8] = t.xyz, 0, q.xyzw.  motions[n_motions] are mbd_load handles; MMDX_CLIP_NONE plays nothing.
void mbd_blend_bone(void *const *motions, uint32_t n_motions, const char *sjis_name, uint32_t n, const uint32_t *clips_a,
                    const double *times_a, const uint32_t *clips_b, const double *times_b, const float *w, float *out) {
    const std::wstring key = mmd::ShiftJISToUTF16String(std::string(sjis_name));
    for (uint32_t i = 0; i < n; ++i) {
        Pose r;
        if (!(w[i] >= 1e-7f)) {
            r = pose_of(motions, n_motions, clips_a[i], key, times_a[i]);
        } else if (w[i] > 1.0f - 1e-7f) {
            r = pose_of(motions, n_motions, clips_b[i], key, times_b[i]);
        } else {
            const Pose a = pose_of(motions, n_motions, clips_a[i], key, times_a[i]);
            const Pose b = pose_of(motions, n_motions, clips_b[i], key, times_b[i]);
            // the lerp the reference applies between two keys of a track (motion_impl.inl:364-372), between the two rows:
            // float, this order, -ffp-contract=off keeps it unfused
            const float wb = w[i], wa = 1.0f - wb;
            r.t.p.x = a.t.p.x * wa + b.t.p.x * wb;
            r.t.p.y = a.t.p.y * wa + b.t.p.y * wb;
            r.t.p.z = a.t.p.z * wa + b.t.p.z * wb;
            r.q = mmd::NLerp(a.q, b.q)[wb];                                        // as motion_impl.inl:375
        }
        float *o = out + size_t(i) * 8;
        for (int k = 0; k < 3; ++k) o[k] = r.t.v[k];
        o[3] = 0.f;
        for (int k = 0; k < 4; ++k) o[4 + k] = r.q.v[k];
    }
}

// The same for the morph stored under the Shift-JIS name -> out[i].
void mbd_blend_morph(void *const *motions, uint32_t n_motions, const char *sjis_name, uint32_t n, const uint32_t *clips_a,
                     const double *times_a, const uint32_t *clips_b, const double *times_b, const float *w, float *out) {
    const std::wstring key = mmd::ShiftJISToUTF16String(std::string(sjis_name));
    for (uint32_t i = 0; i < n; ++i) {
        if (!(w[i] >= 1e-7f)) {
            out[i] = rate_of(motions, n_motions, clips_a[i], key, times_a[i]);
        } else if (w[i] > 1.0f - 1e-7f) {
            out[i] = rate_of(motions, n_motions, clips_b[i], key, times_b[i]);
        } else {
            const float ra = rate_of(motions, n_motions, clips_a[i], key, times_a[i]);
            const float rb = rate_of(motions, n_motions, clips_b[i], key, times_b[i]);
            out[i] = ra * (1.0f - w[i]) + rb * w[i];          // the reference's lerp of two morph keys (motion_impl.inl:462)
        }
    }
}

}  // extern "C"

// tests/motion_time_driver.cpp -- TEST INFRASTRUCTURE ONLY: the real libmmd's time-based track evaluation,
// Motion::GetBonePose(name, double time) and GetMorphPose(name, double time) (L/motion/motion_impl.inl:321-380,
// :426-465), behind a small C interface for tests/motion_time_ref.py.  libmmd is #included by path at build time
// (tests/motion_time_ref.py compiles this file with g++ -O2 -ffp-contract=off); nothing built from it is committed.
// (L/ = 3rd_party/libmmd/include/mmd/)

// The include order of oracle/ref_harness.cpp and of the viewer: <math.h> / <stdlib.h> before mmd.hxx, so
// Bezier::interpolate's unqualified `abs` binds to the float overload (otherwise every curve collapses).
#include <math.h>
#include <stdlib.h>

#include <mmd/mmd.hxx>

#include <cstdint>
#include <exception>
#include <string>

extern "C" {

// VmdReader + Motion of a .vmd file; nullptr on a read error
void *mtd_load(const char *path) {
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

void mtd_destroy(void *h) { delete static_cast<mmd::Motion *>(h); }

// GetBonePose(name, times[i]) for the track stored under the Shift-JIS name -> out[i][8] = t.xyz, 0, q.xyzw.
// Returns 0 (out untouched) when the motion has no such track.  NaN times are undefined behaviour in libmmd: not passed.
int mtd_bone_poses_time(void *h, const char *sjis_name, uint32_t n, const double *times, float *out) {
    mmd::Motion *m = static_cast<mmd::Motion *>(h);
    const std::wstring key = mmd::ShiftJISToUTF16String(std::string(sjis_name));
    if (!m->IsBoneRegistered(key)) return 0;
    for (uint32_t i = 0; i < n; ++i) {
        const mmd::Motion::BonePose pose = m->GetBonePose(key, times[i]);
        float *o = out + size_t(i) * 8;
        for (int k = 0; k < 3; ++k) o[k] = pose.GetTranslation().v[k];
        o[3] = 0.f;
        for (int k = 0; k < 4; ++k) o[4 + k] = pose.GetRotation().v[k];
    }
    return 1;
}

// GetMorphPose(name, times[i]) -> out[i]; returns 0 (out untouched) when the motion has no such track.
int mtd_morph_weights_time(void *h, const char *sjis_name, uint32_t n, const double *times, float *out) {
    mmd::Motion *m = static_cast<mmd::Motion *>(h);
    const std::wstring key = mmd::ShiftJISToUTF16String(std::string(sjis_name));
    if (!m->IsMorphRegistered(key)) return 0;
    for (uint32_t i = 0; i < n; ++i) out[i] = m->GetMorphPose(key, times[i]).GetWeight();
    return 1;
}

}  // extern "C"

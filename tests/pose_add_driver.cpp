// tests/pose_add_driver.cpp -- TEST INFRASTRUCTURE ONLY: additive layers (include/mmdx.h, mmdx_pose_add / mmdx_rate_add) computed by
// the real libmmd.  A stand-alone program over libmmd's own Quaternionf / Vector3f operators, Inverse() and
// SLerp(Quaternionf::Identity(), .)[.], in the order the header states: the difference the way the CCD loop extracts one
// (L/motion/poser_impl.inl:290), applied the way Poser::UpdateMorphTransform (:347-353) and UpdateBoneTransform (:144-145) apply a
// bone morph to a bone whose morph_* were just reset; rates in the form of a vertex morph (:344).  libmmd is #included by path at
// build time (tests/pose_add_ref.py compiles this file with g++ -O2 -ffp-contract=off); nothing built from it is committed.
// (L/ = 3rd_party/libmmd/include/mmd/)
//
//   pose_add_driver IN OUT
// IN:  u32 n_poses, u32 n_rates; n_poses x { f32 a[8], f32 b[8], f32 r[8], f32 e, u32 has_ref }; n_rates x { f32 a, b, r, e; u32
//      has_ref }, items as t.xyz, 0, q.xyzw.  OUT: n_poses x f32[8], n_rates x f32.
#include <math.h>
#include <stdlib.h>

#include <mmd/mmd.hxx>

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

namespace {

struct PoseIn {
    float a[8], b[8], r[8], e;
    uint32_t has_ref;
};
struct RateIn {
    float a, b, r, e;
    uint32_t has_ref;
};

mmd::Vector3f vec_of(const float *p) {
    mmd::Vector3f v;
    v.p.x = p[0]; v.p.y = p[1]; v.p.z = p[2];
    return v;
}
mmd::Quaternionf quat_of(const float *p) {
    mmd::Quaternionf q;
    q.i = p[4]; q.j = p[5]; q.k = p[6]; q.e = p[7];
    return q;
}

void add_pose(const PoseIn &in, float *out) {
    if (!(in.e >= 1e-7f)) {                       // the bone-morph walk's skip, closed over NaN: the item is A's, every bit
        memcpy(out, in.a, sizeof in.a);
        return;
    }
    mmd::Quaternionf dq = quat_of(in.b);
    mmd::Vector3f dt = vec_of(in.b);
    if (in.has_ref) {
        dq = quat_of(in.b) * quat_of(in.r).Inverse();                                   // as poser_impl.inl:290
        dt = vec_of(in.b) - vec_of(in.r);
    }
    // Poser::ResetPosing, then one application (dt, dq) at rate e: poser_impl.inl:351-352
    mmd::Vector3f morph_translation;
    morph_translation.p.x = morph_translation.p.y = morph_translation.p.z = 0.0f;
    mmd::Quaternionf morph_rotation = mmd::Quaternionf::Identity();
    const float rate = in.e;
    morph_translation = morph_translation + dt * rate;
    morph_rotation = morph_rotation * mmd::SLerp(mmd::Quaternionf::Identity(), dq)[rate];
    // UpdateBoneTransform: poser_impl.inl:144-145
    const mmd::Quaternionf total_rotation = morph_rotation * quat_of(in.a);
    const mmd::Vector3f total_translation = morph_translation + vec_of(in.a);
    out[0] = total_translation.p.x; out[1] = total_translation.p.y; out[2] = total_translation.p.z;
    out[3] = 0.0f;
    out[4] = total_rotation.i; out[5] = total_rotation.j; out[6] = total_rotation.k; out[7] = total_rotation.e;
}

float add_rate(const RateIn &in) {
    if (!(in.e >= 1e-7f)) return in.a;
    const float d = in.has_ref ? in.b - in.r : in.b;
    return in.a + d * in.e;                                                             // vertex_image + offset * rate, :344
}

}  // namespace

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 3;
    uint32_t n[2];
    if (fread(n, 4, 2, f) != 2) return 4;
    std::vector<PoseIn> poses(n[0]);
    std::vector<RateIn> rates(n[1]);
    if (n[0] && fread(poses.data(), sizeof(PoseIn), n[0], f) != n[0]) return 4;
    if (n[1] && fread(rates.data(), sizeof(RateIn), n[1], f) != n[1]) return 4;
    fclose(f);
    std::vector<float> out(size_t(n[0]) * 8 + n[1]);
    for (uint32_t i = 0; i < n[0]; ++i) add_pose(poses[i], out.data() + size_t(i) * 8);
    for (uint32_t i = 0; i < n[1]; ++i) out[size_t(n[0]) * 8 + i] = add_rate(rates[i]);
    f = fopen(argv[2], "wb");
    if (!f) return 3;
    const bool ok = out.empty() || fwrite(out.data(), 4, out.size(), f) == out.size();
    return fclose(f) == 0 && ok ? 0 : 5;
}

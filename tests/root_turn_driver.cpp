// tests/root_turn_driver.cpp -- TEST INFRASTRUCTURE ONLY: mmdx_animator_root_motion_turn (include/mmdx.h) computed by the real libmmd.
// A stand-alone program:
//     root_turn_driver in.bin out.bin <root bone name, Shift-JIS bytes> <clip 0 .vmd> <clip 1 .vmd> ...
// (T, Q)(c, t) is Motion::GetBonePose(name, double time) (L/motion/motion_impl.inl:321-380): GetTranslation() and GetRotation();
// {0,0,0} and the identity for a clip outside the bank or a motion without that track (what MotionPlayer::SeekTime leaves after
// Poser::ResetPosing).  Every step of the header's text is libmmd's own operator: Quaternionf::Inverse (L/util/math_impl.inl:474-477),
// Quaternionf::operator* (:510-517), ToRotateMatrix (:540-563), mmd::rotate(Vector3f, Matrix4f) (:1032-1038), Vector3f's - and +,
// Quaternionf::Normalize (:457-465); the blend of the two sides is the lerp the reference applies between two keys
// (motion_impl.inl:364-372) and mmd::NLerp (:1260-1282), restated as in tests/motion_blend_driver.cpp.  The clocks are the
// project's own csrc/anim_math.hpp compiled for the host.  csrc/root_math.hpp is NOT included: this file states the steps of the
// header text on its own.  libmmd is #included by path at build time (tests/root_turn_ref.py compiles this file with g++ -O2
// -ffp-contract=off); nothing built from it is committed.  (L/ = 3rd_party/libmmd/include/mmd/)
//
// in.bin   u32 n, nc
//          table  f64 length[nc]; u32 mode[nc]; u32 next[nc]; f32 fade[nc]
//          rows   u32 clips_a[n], clips_b[n]; f64 times_a[n], times_b[n]; f32 weights[n], speed[n], fade_rate[n]; f64 dt[n];
//                 u32 axes[n]; f32 placements[n][8]; u32 flags[n] (MMDX_ROOT_NORMALIZE or 0)
// out.bin  f64 times[n][2][4] (side a, b x t0, t1, near, far; 0 where the instant is not sampled); u32 folded[n][2];
//          f32 T[n][2][4][3], Q[n][2][4][4] (0 and the identity where not sampled); f32 expect[n][8] (placements[i] after the call)

// The include order of oracle/ref_harness.cpp and of the viewer: <math.h> / <stdlib.h> before mmd.hxx.
#include <math.h>
#include <stdlib.h>

#include <mmd/mmd.hxx>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <exception>
#include <memory>
#include <string>
#include <vector>

#include "../simple_mmd_renderer_amd/csrc/anim_math.hpp"

namespace {

const uint32_t kNormalize = 1u << 14;          // MMDX_ROOT_NORMALIZE

template <typename T>
std::vector<T> take(std::FILE *f, size_t n) {
    std::vector<T> v(n);
    if (n && std::fread(v.data(), sizeof(T), n, f) != n) {
        std::fprintf(stderr, "root_turn_driver: input too short\n");
        std::exit(2);
    }
    return v;
}

template <typename T>
void put(std::FILE *f, const std::vector<T> &v) {
    if (!v.empty() && std::fwrite(v.data(), sizeof(T), v.size(), f) != v.size()) {
        std::fprintf(stderr, "root_turn_driver: write failed\n");
        std::exit(2);
    }
}

mmd::Vector3f zero3() {
    mmd::Vector3f v;
    v.v[0] = v.v[1] = v.v[2] = 0.f;
    return v;
}

struct Sample {
    mmd::Vector3f t = zero3();
    mmd::Quaternionf q = mmd::Quaternionf::Identity();
};

struct Delta {
    mmd::Vector3f d = zero3();
    mmd::Quaternionf q = mmd::Quaternionf::Identity();
};

struct Side {
    double t[4] = {0, 0, 0, 0};
    uint32_t folded = 0;
    Sample at[4];
    Delta delta;
};

// from `from` to `to`, in `from`'s frame
Delta leg(const Sample &from, const Sample &to) {
    Delta r;
    const mmd::Quaternionf qi = from.q.Inverse();
    r.q = qi * to.q;
    r.d = mmd::rotate(to.t - from.t, qi.ToRotateMatrix());
    return r;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc < 5) {
        std::fprintf(stderr, "usage: root_turn_driver in.bin out.bin root_name clip0.vmd [clip1.vmd ...]\n");
        return 2;
    }
    std::FILE *in = std::fopen(argv[1], "rb"), *out = std::fopen(argv[2], "wb");
    if (!in || !out) {
        std::fprintf(stderr, "root_turn_driver: cannot open the files\n");
        return 2;
    }
    const std::wstring key = mmd::ShiftJISToUTF16String(std::string(argv[3]));
    std::vector<std::unique_ptr<mmd::Motion>> motions;
    for (int k = 4; k < argc; ++k) {
        motions.emplace_back(new mmd::Motion);
        try {
            std::string p(argv[k]);
            mmd::FileReader file(std::wstring(p.begin(), p.end()));
            mmd::VmdReader(file).ReadMotion(*motions.back());
        } catch (const std::exception &) {
            std::fprintf(stderr, "root_turn_driver: cannot read %s\n", argv[k]);
            return 2;
        }
    }
    const std::vector<uint32_t> head = take<uint32_t>(in, 2);
    const size_t n = head[0], nc = head[1];
    if (nc != motions.size()) {
        std::fprintf(stderr, "root_turn_driver: %zu clips in the table, %zu files\n", nc, motions.size());
        return 2;
    }
    const auto length = take<double>(in, nc);
    const auto mode = take<uint32_t>(in, nc), next = take<uint32_t>(in, nc);
    const auto fade = take<float>(in, nc);
    const auto clips_a = take<uint32_t>(in, n), clips_b = take<uint32_t>(in, n);
    const auto times_a = take<double>(in, n), times_b = take<double>(in, n);
    const auto weights = take<float>(in, n), speed = take<float>(in, n), fade_rate = take<float>(in, n);
    const auto dt = take<double>(in, n);
    const auto axes = take<uint32_t>(in, n);
    const auto placements = take<float>(in, n * 8);
    const auto flags = take<uint32_t>(in, n);
    const mmdx::AnimClips table{length.data(), mode.data(), next.data(), fade.data(), uint32_t(nc)};

    auto TQ = [&](uint32_t c, double t) {
        Sample s;
        if (c >= nc || !motions[c]->IsBoneRegistered(key)) return s;
        const mmd::Motion::BonePose bp = motions[c]->GetBonePose(key, t);
        s.t = bp.GetTranslation();
        s.q = bp.GetRotation().q;
        return s;
    };
    auto side_of = [&](uint32_t c, double t0, double s) {
        Side sd;
        const double raw = t0 + s;
        sd.t[0] = t0;
        sd.t[1] = mmdx::anim_wrap(table, c, raw, &sd.folded);
        sd.at[0] = TQ(c, sd.t[0]);
        sd.at[1] = TQ(c, sd.t[1]);
        if (!sd.folded) {
            sd.delta = leg(sd.at[0], sd.at[1]);
        } else {
            const double L = length[c];
            if (raw >= L) sd.t[2] = L; else sd.t[3] = L;
            sd.at[2] = TQ(c, sd.t[2]);
            sd.at[3] = TQ(c, sd.t[3]);
            const Delta one = leg(sd.at[0], sd.at[2]), two = leg(sd.at[3], sd.at[1]);
            sd.delta.d = one.d + mmd::rotate(two.d, one.q.ToRotateMatrix());
            sd.delta.q = one.q * two.q;
        }
        return sd;
    };

    std::vector<double> o_times(n * 8, 0.0);
    std::vector<uint32_t> o_folded(n * 2, 0);
    std::vector<float> o_t(n * 24, 0.f), o_q(n * 32, 0.f), o_expect(n * 8, 0.f);
    for (size_t i = 0; i < n; ++i) {
        const float *place = placements.data() + i * 8;
        for (int k = 0; k < 8; ++k) o_expect[i * 8 + k] = place[k];
        for (int j = 0; j < 8; ++j) o_q[(i * 8 + j) * 4 + 3] = 1.f;
        if (dt[i] != dt[i]) continue;                                    // a NaN step writes nothing
        const double s = double(speed[i]) * dt[i];
        const float w = weights[i];
        const bool is_a = !(w >= 1e-7f), is_b = !is_a && w > 1.0f - 1e-7f;
        Side a, b;                                                       // a side that is not read stays {+0,+0,+0} and the identity
        if (!is_b) a = side_of(clips_a[i], times_a[i], s);
        if (!is_a && fade_rate[i] > 0.0f) b = side_of(clips_b[i], times_b[i], s);
        Delta m;
        if (is_a) {
            m = a.delta;
        } else if (is_b) {
            m = b.delta;
        } else {
            // the lerp between two keys (motion_impl.inl:364-372) and the NLerp of :375, between the two sides
            for (int k = 0; k < 3; ++k) m.d.v[k] = a.delta.d.v[k] * (1.0f - w) + b.delta.d.v[k] * w;
            mmd::Vector4f qa, qb;
            qa.q = a.delta.q;
            qb.q = b.delta.q;
            m.q = mmd::NLerp(qa, qb)[w].q;
        }
        for (int k = 0; k < 3; ++k)
            if (!(axes[i] & (1u << k))) m.d.v[k] = 0.0f;
        mmd::Vector4f h;
        for (int k = 0; k < 4; ++k) h.v[k] = place[4 + k];
        const mmd::Vector3f turned = mmd::rotate(m.d, h.q.ToRotateMatrix());      // the heading BEFORE the step
        mmd::Vector4f after;
        after.q = h.q * m.q;
        if (flags[i] & kNormalize) after.q = after.q.Normalize();
        for (int k = 0; k < 3; ++k) o_expect[i * 8 + k] = place[k] + turned.v[k];
        for (int k = 0; k < 4; ++k) o_expect[i * 8 + 4 + k] = after.v[k];
        const Side *sides[2] = {&a, &b};
        for (int sd = 0; sd < 2; ++sd) {
            o_folded[i * 2 + sd] = sides[sd]->folded;
            for (int j = 0; j < 4; ++j) {
                const size_t at = (i * 2 + sd) * 4 + j;
                o_times[at] = sides[sd]->t[j];
                mmd::Vector4f q;
                q.q = sides[sd]->at[j].q;
                for (int k = 0; k < 3; ++k) o_t[at * 3 + k] = sides[sd]->at[j].t.v[k];
                for (int k = 0; k < 4; ++k) o_q[at * 4 + k] = q.v[k];
            }
        }
    }
    put(out, o_times); put(out, o_folded); put(out, o_t); put(out, o_q); put(out, o_expect);
    std::fclose(in);
    if (std::fclose(out) != 0) return 2;
    return 0;
}

// tests/root_math_driver.cpp -- TEST INFRASTRUCTURE ONLY: csrc/root_math.hpp, the arithmetic of mmdx_animator_root_motion, compiled
// for the host.  A stand-alone program: `root_math_driver in.bin out.bin` reads rows of animator state, a step and a placement
// each, plus R -- the root bone's translation at the eight instants of every row, which on the device is eval_bone_pose -- and
// writes the instants, the fold flags and the placements after the call.  tests/test_root_motion_cpu.py builds it once plain and
// once under the sanitizers (tests/host_program.py: build(..., sanitize=True)) and compares the output, bit for bit, with the golden rows
// of the real libmmd and with tests/root_motion_ref.py.
// The two functions root_math.hpp takes from its caller are motion_blend.hpp's blend_side and blend_rate, which exist for the
// device only; the host forms below are those two, line for line.
//
// in.bin   u32 n, nc, with_r        with_r = 0: R is absent, only the instants are computed (expect = the placements unchanged)
//          table  f64 length[nc]; u32 mode[nc]; u32 next[nc]; f32 fade[nc]
//          rows   u32 clips_a[n], clips_b[n]; f64 times_a[n], times_b[n]; f32 weights[n], speed[n], fade_rate[n]; f64 dt[n];
//                 u32 axes[n]; f32 placements[n][8]
//          f32 R[n][2][4][3]          (with_r only)
// out.bin  f64 times[n][2][4] (0 where the instant is not sampled); u32 folded[n][2]; f32 expect[n][3]
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../simple_mmd_renderer_amd/csrc/root_math.hpp"

namespace {

template <typename T>
std::vector<T> take(std::FILE *f, size_t n) {
    std::vector<T> v(n);
    if (n && std::fread(v.data(), sizeof(T), n, f) != n) {
        std::fprintf(stderr, "root_math_driver: input too short\n");
        std::exit(2);
    }
    return v;
}

template <typename T>
void put(std::FILE *f, const std::vector<T> &v) {
    if (!v.empty() && std::fwrite(v.data(), sizeof(T), v.size(), f) != v.size()) {
        std::fprintf(stderr, "root_math_driver: write failed\n");
        std::exit(2);
    }
}

// motion_blend.hpp
uint32_t blend_side(float w) {
    if (!(w >= 1e-7f)) return mmdx::kRootSideA;
    if (w > 1.0f - 1e-7f) return mmdx::kRootSideB;
    return mmdx::kRootSideMix;
}
float blend_rate(const float a, const float b, const float w) { return a * (1.0f - w) + b * w; }

}  // namespace

int main(int argc, char **argv) {
    if (argc != 3) {
        std::fprintf(stderr, "usage: root_math_driver in.bin out.bin\n");
        return 2;
    }
    std::FILE *in = std::fopen(argv[1], "rb"), *out = std::fopen(argv[2], "wb");
    if (!in || !out) {
        std::fprintf(stderr, "root_math_driver: cannot open the files\n");
        return 2;
    }
    const std::vector<uint32_t> head = take<uint32_t>(in, 3);
    const size_t n = head[0], nc = head[1];
    const bool with_r = head[2] != 0;
    const auto length = take<double>(in, nc);
    const auto mode = take<uint32_t>(in, nc), next = take<uint32_t>(in, nc);
    const auto fade = take<float>(in, nc);
    const auto clips_a = take<uint32_t>(in, n), clips_b = take<uint32_t>(in, n);
    const auto times_a = take<double>(in, n), times_b = take<double>(in, n);
    const auto weights = take<float>(in, n), speed = take<float>(in, n), fade_rate = take<float>(in, n);
    const auto dt = take<double>(in, n);
    const auto axes = take<uint32_t>(in, n);
    const auto placements = take<float>(in, n * 8);
    const auto r_in = take<float>(in, with_r ? n * 24 : 0);
    const mmdx::AnimClips table{length.data(), mode.data(), next.data(), fade.data(), uint32_t(nc)};

    std::vector<double> o_times(n * 8, 0.0);
    std::vector<uint32_t> o_folded(n * 2, 0);
    std::vector<float> o_expect(n * 3, 0.f);
    for (size_t i = 0; i < n; ++i) {
        float pose[8];
        for (int k = 0; k < 8; ++k) pose[k] = placements[i * 8 + k];
        for (int k = 0; k < 3; ++k) o_expect[i * 3 + k] = pose[k];
        if (dt[i] != dt[i]) continue;
        const float w = weights[i];
        const uint32_t side = blend_side(w);
        const bool reads[2] = {side != mmdx::kRootSideB, side != mmdx::kRootSideA && fade_rate[i] > 0.0f};
        mmdx::RootVec d[2] = {{0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}};
        for (int sd = 0; sd < 2; ++sd) {
            mmdx::RootVec at[4] = {{0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}};
            uint32_t folded = 0;
            if (reads[sd]) {
                const mmdx::RootTimes rt = mmdx::root_times(table, sd ? clips_b[i] : clips_a[i], sd ? times_b[i] : times_a[i],
                                                            double(speed[i]) * dt[i]);
                folded = rt.folded;
                for (uint32_t j = 0; j < 4; ++j) {
                    if (j >= mmdx::kRootNear && !folded) continue;
                    o_times[(i * 2 + sd) * 4 + j] = mmdx::root_time_of(rt, j);
                    if (with_r) {
                        const float *r = r_in.data() + ((i * 2 + sd) * 4 + j) * 3;
                        at[j] = {r[0], r[1], r[2]};
                    }
                }
            }
            o_folded[i * 2 + sd] = folded;
            d[sd] = mmdx::root_displacement(at[mmdx::kRootT0], at[mmdx::kRootT1], at[mmdx::kRootNear], at[mmdx::kRootFar], folded);
        }
        const mmdx::RootVec m = mmdx::root_mask(mmdx::root_blend(d[0], d[1], side, w, blend_rate), axes[i]);
        mmdx::root_accumulate(m, pose);
        for (int k = 0; k < 3; ++k) o_expect[i * 3 + k] = pose[k];
    }
    put(out, o_times); put(out, o_folded); put(out, o_expect);
    std::fclose(in);
    if (std::fclose(out) != 0) return 2;
    return 0;
}

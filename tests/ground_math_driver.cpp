// ground_math_driver.cpp -- csrc/ground_math.hpp and csrc/ground_table.hpp built for the host: the lines the gfx950 kernels compile
// and the lines mmdx_ground_create runs, over a table of calls, by a stand-alone program (tests/ground_ref.py builds it through
// tests/host_program.py, plain and under the sanitizers, and compares what it writes with the numpy restatement).
//
//   ground_math_driver in.bin out.bin
//
// in.bin   u32 nx, nz, n_calls; f32 origin_x, origin_z, cell_x, cell_z; f32 heights[nz][nx]
//          per call: u32 kind (0 place, 1 targets), ni, n_feet, has_drop; f32 a, b (place: y_offset, unused; targets: max_step, max_drop)
//            place:   f32 placements[ni][8], then drop[ni] if has_drop
//            targets: f32 placements[ni][8], points[n_feet][ni][4] (point_stride 4, slab_stride ni*4)
// out.bin  f32 min_height, max_height
//          per call: place: f32 placements[ni][8] after it; targets: f32 targets[n_feet][ni][4], then drop[ni] if has_drop -- both
//          filled with the word 0xCDCDCDCD before the call
// Exit status 3 with the library's message on stderr when the table is refused.
//
//   ground_math_driver plan
//
// one planner call per line on stdin: cells -> threads nblocks
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../simple_mmd_renderer_amd/csrc/ground_math.hpp"
#include "../simple_mmd_renderer_amd/csrc/ground_table.hpp"

using namespace mmdx;

template <class T>
static std::vector<T> take(FILE *f, size_t n) {
    std::vector<T> v(n);
    if (n && fread(v.data(), sizeof(T), n, f) != n) {
        fprintf(stderr, "ground_math_driver: the input is short\n");
        exit(2);
    }
    return v;
}
template <class T>
static void put(FILE *f, const std::vector<T> &v) {
    if (!v.empty() && fwrite(v.data(), sizeof(T), v.size(), f) != v.size()) {
        fprintf(stderr, "ground_math_driver: cannot write\n");
        exit(2);
    }
}

static std::vector<float> sentinels(size_t n) {
    std::vector<float> v(n);
    if (n) memset(v.data(), 0xCD, n * sizeof(float));
    return v;
}

static int plan() {
    unsigned cells;
    while (scanf("%u", &cells) == 1) {
        const GroundShape s = plan_ground_launch(cells);
        printf("%u %u\n", s.threads, s.nblocks);
    }
    return 0;
}

int main(int argc, char **argv) {
    if (argc == 2 && !strcmp(argv[1], "plan")) return plan();
    if (argc != 3) {
        fprintf(stderr, "usage: ground_math_driver in.bin out.bin | ground_math_driver plan\n");
        return 2;
    }
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    if (!in || !out) {
        fprintf(stderr, "ground_math_driver: cannot open the files\n");
        return 2;
    }
    const std::vector<uint32_t> head = take<uint32_t>(in, 3);
    const std::vector<float> geo = take<float>(in, 4);
    const uint32_t n_calls = head[2];
    if (head[0] > kGroundMaxSamples || head[1] > kGroundMaxSamples) {
        fprintf(stderr, "ground_math_driver: a field too large to read\n");
        return 2;
    }
    const std::vector<float> heights = take<float>(in, size_t(head[0]) * head[1]);

    mmdx_ground_desc d{};
    d.struct_size = sizeof(d);
    d.nx = head[0]; d.nz = head[1];
    d.origin_x = geo[0]; d.origin_z = geo[1]; d.cell_x = geo[2]; d.cell_z = geo[3];
    d.heights = heights.data();
    GroundTable t;
    if (ground_table_build(&d, &t) != MMDX_OK) {
        fprintf(stderr, "ground_math_driver: %s\n", mmdx_last_error_string());
        return 3;
    }
    put(out, std::vector<float>{t.min_height, t.max_height});
    const float *H = t.heights.data();
    for (uint32_t c = 0; c < n_calls; ++c) {
        const std::vector<uint32_t> ch = take<uint32_t>(in, 4);
        const std::vector<float> par = take<float>(in, 2);
        const uint32_t kind = ch[0], ni = ch[1], nf = ch[2];
        const bool has_drop = ch[3] != 0;
        std::vector<float> pl = take<float>(in, size_t(ni) * kGroundPoseFloats);
        if (kind == 0) {
            const std::vector<float> drop = take<float>(in, has_drop ? ni : 0);
            for (uint32_t i = 0; i < ni; ++i)
                ground_place_instance(t.g, H, pl.data() + size_t(i) * kGroundPoseFloats, has_drop ? drop.data() + i : nullptr, par[0]);
            put(out, pl);
        } else {
            if (!nf || nf > kGroundMaxFeet) {
                fprintf(stderr, "ground_math_driver: n_feet\n");
                return 2;
            }
            const std::vector<float> pts = take<float>(in, size_t(nf) * ni * 4);
            std::vector<float> tgt = sentinels(size_t(nf) * ni * 4), drop = sentinels(has_drop ? ni : 0);
            for (uint32_t i = 0; i < ni; ++i)
                ground_targets_instance(t.g, H, pl.data() + size_t(i) * kGroundPoseFloats, pts.data() + size_t(i) * 4, size_t(ni) * 4, nf, par[0],
                                        par[1], tgt.data() + size_t(i) * 4, size_t(ni) * 4, has_drop ? drop.data() + i : nullptr);
            put(out, tgt);
            put(out, drop);
        }
    }
    fclose(in);
    if (fclose(out) != 0) return 2;
    return 0;
}

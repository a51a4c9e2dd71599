// aim_math_driver.cpp -- csrc/aim_math.hpp and csrc/aim_table.hpp built for the host: the lines the gfx950 kernel compiles and the
// lines mmdx_aim_set_create runs, over a table of calls, by a stand-alone program (tests/aim_ref.py builds it through
// tests/host_program.py, plain and under the sanitizers, and compares what it writes with the numpy restatement).
//
//   aim_math_driver in.bin out.bin
//
// in.bin   u32 nb, n_aims, n_links, ni, n_calls
//          i32 parent[nb], f32 rest[nb][3], u32 link_offset[n_aims + 1], u32 link_bone[n_links], f32 link_params[n_links][2],
//          u32 eye_bone[n_aims], f32 eye_point[n_aims][3], f32 forward[n_aims][3]
//          per call: f32 palettes[ni][nb][16], f32 targets[ni][4]
// out.bin  the table as built, per aim: u32 n_rows, u32 bone[L], f32 h[L][3], f32 sin_limit[L], u32 {bone, depth}[n_rows]
//          per call: f32 palettes[ni][nb][16] after it
// Exit status 3 with the library's message on stderr when the table is refused.
//
//   aim_math_driver plan
//
// one planner call per line on stdin: cells max_links env (MMDX_AIM_BLOCK as read, 0 = not set) -> block threads nblocks lds
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../simple_mmd_renderer_amd/csrc/aim_math.hpp"
#include "../simple_mmd_renderer_amd/csrc/aim_table.hpp"

using namespace mmdx;

template <class T>
static std::vector<T> take(FILE *f, size_t n) {
    std::vector<T> v(n);
    if (n && fread(v.data(), sizeof(T), n, f) != n) {
        fprintf(stderr, "aim_math_driver: the input is short\n");
        exit(2);
    }
    return v;
}
template <class T>
static void put(FILE *f, const std::vector<T> &v) {
    if (!v.empty() && fwrite(v.data(), sizeof(T), v.size(), f) != v.size()) {
        fprintf(stderr, "aim_math_driver: cannot write\n");
        exit(2);
    }
}

static int plan() {
    unsigned cells, max_links;
    int env;
    while (scanf("%u %u %d", &cells, &max_links, &env) == 3) {
        const AimShape s = plan_aim_launch(cells, max_links, env);
        printf("%u %u %u %u\n", s.block, s.threads, s.nblocks, s.lds);
    }
    return 0;
}

int main(int argc, char **argv) {
    if (argc == 2 && !strcmp(argv[1], "plan")) return plan();
    if (argc != 3) {
        fprintf(stderr, "usage: aim_math_driver in.bin out.bin | aim_math_driver plan\n");
        return 2;
    }
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    if (!in || !out) {
        fprintf(stderr, "aim_math_driver: cannot open the files\n");
        return 2;
    }
    const std::vector<uint32_t> head = take<uint32_t>(in, 5);
    const uint32_t nb = head[0], n_aims = head[1], nl = head[2], ni = head[3], n_calls = head[4];
    const std::vector<int32_t> parent = take<int32_t>(in, nb);
    const std::vector<float> rest = take<float>(in, size_t(nb) * 3);
    const std::vector<uint32_t> link_offset = take<uint32_t>(in, size_t(n_aims) + 1), link_bone = take<uint32_t>(in, nl);
    const std::vector<float> params = take<float>(in, size_t(nl) * 2);
    const std::vector<uint32_t> eye_bone = take<uint32_t>(in, n_aims);
    const std::vector<float> eye_point = take<float>(in, size_t(n_aims) * 3), forward = take<float>(in, size_t(n_aims) * 3);

    mmdx_aim_set_desc d{};
    d.struct_size = sizeof(d);
    d.n_aims = n_aims;
    d.link_offset = link_offset.data();
    d.link_bone = link_bone.data();
    d.link_params = params.data();
    d.eye_bone = eye_bone.data();
    d.eye_point = eye_point.data();
    d.forward = forward.data();
    AimTable t;
    if (aim_table_build(&d, nb, parent.data(), rest.data(), &t) != MMDX_OK) {
        fprintf(stderr, "aim_math_driver: %s\n", mmdx_last_error_string());
        return 3;
    }
    for (const AimAim &m : t.aims) {
        std::vector<uint32_t> bones, rows;
        std::vector<float> hs, sins;
        for (uint32_t l = m.first_link; l < m.first_link + m.n_links; ++l) {
            bones.push_back(t.links[l].bone);
            hs.insert(hs.end(), t.links[l].h, t.links[l].h + 3);
            sins.push_back(t.links[l].sin_limit);
        }
        for (uint32_t r = m.first_row; r < m.first_row + m.n_rows; ++r) rows.insert(rows.end(), {t.rows[r].bone, t.rows[r].depth});
        put(out, std::vector<uint32_t>{m.n_rows});
        put(out, bones);
        put(out, hs);
        put(out, sins);
        put(out, rows);
    }
    const size_t pal_floats = size_t(nb) * 16;
    for (uint32_t c = 0; c < n_calls; ++c) {
        std::vector<float> pal = take<float>(in, size_t(ni) * pal_floats);
        const std::vector<float> tgt = take<float>(in, size_t(ni) * 4);
        for (uint32_t i = 0; i < ni; ++i) aim_instance(t, pal.data() + i * pal_floats, tgt.data() + size_t(i) * 4);
        put(out, pal);
    }
    fclose(in);
    if (fclose(out) != 0) return 2;
    return 0;
}

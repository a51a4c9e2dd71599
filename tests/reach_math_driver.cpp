// reach_math_driver.cpp -- csrc/reach_math.hpp and csrc/reach_table.hpp built for the host: the lines the gfx950 kernel compiles and
// the lines mmdx_reach_set_create runs, over a table of calls, by a stand-alone program (tests/reach_ref.py builds it through
// tests/host_program.py, plain and under the sanitizers, and compares what it writes with the numpy restatement).
//
//   reach_math_driver in.bin out.bin
//
// in.bin   u32 nb, n_reaches, ni, n_calls
//          i32 parent[nb], f32 rest[nb][3], u32 bones[n_reaches][3], f32 tip_point[n_reaches][3], f32 pole[n_reaches][3],
//          f32 max_extension[n_reaches], u32 flags[n_reaches]
//          per call: f32 palettes[ni][nb][16], f32 targets[ni][4]
// out.bin  the table as built, per reach: u32 n_rows, f32 {ha, hb, hc}[3], u32 {bone, depth}[n_rows]
//          per call: f32 palettes[ni][nb][16] after it
// Exit status 3 with the library's message on stderr when the table is refused.
//
//   reach_math_driver plan
//
// one planner call per line on stdin: cells -> block threads nblocks lds
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../simple_mmd_renderer_amd/csrc/reach_math.hpp"
#include "../simple_mmd_renderer_amd/csrc/reach_table.hpp"

using namespace mmdx;

template <class T>
static std::vector<T> take(FILE *f, size_t n) {
    std::vector<T> v(n);
    if (n && fread(v.data(), sizeof(T), n, f) != n) {
        fprintf(stderr, "reach_math_driver: the input is short\n");
        exit(2);
    }
    return v;
}
template <class T>
static void put(FILE *f, const std::vector<T> &v) {
    if (!v.empty() && fwrite(v.data(), sizeof(T), v.size(), f) != v.size()) {
        fprintf(stderr, "reach_math_driver: cannot write\n");
        exit(2);
    }
}

static int plan() {
    unsigned cells;
    while (scanf("%u", &cells) == 1) {
        const ReachShape s = plan_reach_launch(cells);
        printf("%u %u %u %u\n", s.block, s.threads, s.nblocks, s.lds);
    }
    return 0;
}

int main(int argc, char **argv) {
    if (argc == 2 && !strcmp(argv[1], "plan")) return plan();
    if (argc != 3) {
        fprintf(stderr, "usage: reach_math_driver in.bin out.bin | reach_math_driver plan\n");
        return 2;
    }
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    if (!in || !out) {
        fprintf(stderr, "reach_math_driver: cannot open the files\n");
        return 2;
    }
    const std::vector<uint32_t> head = take<uint32_t>(in, 4);
    const uint32_t nb = head[0], nr = head[1], ni = head[2], n_calls = head[3];
    const std::vector<int32_t> parent = take<int32_t>(in, nb);
    const std::vector<float> rest = take<float>(in, size_t(nb) * 3);
    const std::vector<uint32_t> bones = take<uint32_t>(in, size_t(nr) * 3);
    const std::vector<float> tip = take<float>(in, size_t(nr) * 3), pole = take<float>(in, size_t(nr) * 3), ext = take<float>(in, nr);
    const std::vector<uint32_t> flags = take<uint32_t>(in, nr);

    mmdx_reach_set_desc d{};
    d.struct_size = sizeof(d);
    d.n_reaches = nr;
    d.bones = bones.data();
    d.tip_point = tip.data();
    d.pole = pole.data();
    d.max_extension = ext.data();
    d.flags = flags.data();
    ReachTable t;
    if (reach_table_build(&d, nb, parent.data(), rest.data(), &t) != MMDX_OK) {
        fprintf(stderr, "reach_math_driver: %s\n", mmdx_last_error_string());
        return 3;
    }
    for (const ReachReach &m : t.reaches) {
        std::vector<uint32_t> rows;
        std::vector<float> hs;
        hs.insert(hs.end(), m.ha, m.ha + 3);
        hs.insert(hs.end(), m.hb, m.hb + 3);
        hs.insert(hs.end(), m.hc, m.hc + 3);
        for (uint32_t r = m.first_row; r < m.first_row + m.n_rows; ++r) rows.insert(rows.end(), {t.rows[r].bone, t.rows[r].depth});
        put(out, std::vector<uint32_t>{m.n_rows});
        put(out, hs);
        put(out, rows);
    }
    const size_t pal_floats = size_t(nb) * 16;
    for (uint32_t c = 0; c < n_calls; ++c) {
        std::vector<float> pal = take<float>(in, size_t(ni) * pal_floats);
        const std::vector<float> tgt = take<float>(in, size_t(ni) * 4);
        for (uint32_t i = 0; i < ni; ++i) reach_instance(t, pal.data() + i * pal_floats, tgt.data() + size_t(i) * 4);
        put(out, pal);
    }
    fclose(in);
    if (fclose(out) != 0) return 2;
    return 0;
}

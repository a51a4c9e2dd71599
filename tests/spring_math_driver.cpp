// spring_math_driver.cpp -- csrc/spring_math.hpp and csrc/spring_table.hpp built for the host: the lines the gfx950 kernel compiles
// and the lines mmdx_spring_set_create runs, over a table of steps, by a stand-alone program (tests/spring_ref.py builds it through
// tests/host_program.py, plain and under the sanitizers, and compares what it writes with the numpy restatement).
//
//   spring_math_driver in.bin out.bin
//
// in.bin   u32 nb, n_chains, n_joints, n_colliders, has_tails, ni, n_steps, n_segments
//          i32 parent[nb], f32 rest[nb][3], u32 chain_offset[n_chains + 1], u32 joint_bone[n_joints], f32 tails[n_joints][3] when
//          has_tails, f32 chain_params[n_chains][4], u32 collider_bone[nc], f32 collider_sphere[nc][4], f32 gravity[3]
//          per segment: u32 steps, has_state; f32 state[ni][n_joints][6] when has_state (else: NaN in the first segment, the state
//          the previous segment left in a later one); per step: f32 dt, u32 reset, f32 palettes[ni][nb][16]
// out.bin  the table as built: u32 bone[n_joints], f32 h[n_joints][3], f32 t[n_joints][3], u32 {first, count, anchor}[n_chains]
//          per step: f32 palettes[ni][nb][16] and f32 state[ni][n_joints][6] after it
// Exit status 3 with the library's message on stderr when the table is refused.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../simple_mmd_renderer_amd/csrc/spring_math.hpp"
#include "../simple_mmd_renderer_amd/csrc/spring_table.hpp"

using namespace mmdx;

template <class T>
static std::vector<T> take(FILE *f, size_t n) {
    std::vector<T> v(n);
    if (n && fread(v.data(), sizeof(T), n, f) != n) {
        fprintf(stderr, "spring_math_driver: the input is short\n");
        exit(2);
    }
    return v;
}
template <class T>
static void put(FILE *f, const std::vector<T> &v) {
    if (!v.empty() && fwrite(v.data(), sizeof(T), v.size(), f) != v.size()) {
        fprintf(stderr, "spring_math_driver: cannot write\n");
        exit(2);
    }
}

int main(int argc, char **argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: spring_math_driver in.bin out.bin\n");
        return 2;
    }
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    if (!in || !out) {
        fprintf(stderr, "spring_math_driver: cannot open the files\n");
        return 2;
    }
    const std::vector<uint32_t> head = take<uint32_t>(in, 8);
    const uint32_t nb = head[0], n_chains = head[1], nj = head[2], nc = head[3], has_tails = head[4], ni = head[5], n_segments = head[7];
    const std::vector<int32_t> parent = take<int32_t>(in, nb);
    const std::vector<float> rest = take<float>(in, size_t(nb) * 3);
    const std::vector<uint32_t> chain_offset = take<uint32_t>(in, size_t(n_chains) + 1), joint_bone = take<uint32_t>(in, nj);
    const std::vector<float> tails = take<float>(in, has_tails ? size_t(nj) * 3 : 0), params = take<float>(in, size_t(n_chains) * 4);
    const std::vector<uint32_t> col_bone = take<uint32_t>(in, nc);
    const std::vector<float> col_sphere = take<float>(in, size_t(nc) * 4), gravity = take<float>(in, 3);

    mmdx_spring_set_desc d{};
    d.struct_size = sizeof(d);
    d.n_chains = n_chains;
    d.n_colliders = nc;
    d.max_instances = ni;
    d.chain_offset = chain_offset.data();
    d.joint_bone = joint_bone.data();
    d.joint_tail = has_tails ? tails.data() : nullptr;
    d.chain_params = params.data();
    d.collider_bone = col_bone.data();
    d.collider_sphere = col_sphere.data();
    for (int k = 0; k < 3; ++k) d.gravity[k] = gravity[k];
    SpringTable t;
    if (spring_table_build(&d, nb, parent.data(), rest.data(), &t) != MMDX_OK) {
        fprintf(stderr, "spring_math_driver: %s\n", mmdx_last_error_string());
        return 3;
    }
    std::vector<uint32_t> bones, rows;
    std::vector<float> hs, ts;
    for (const SpringJoint &e : t.joints) {
        bones.push_back(e.bone);
        hs.insert(hs.end(), e.h, e.h + 3);
        ts.insert(ts.end(), e.t, e.t + 3);
    }
    for (const SpringChain &c : t.chains) rows.insert(rows.end(), {c.first, c.count, c.anchor});
    put(out, bones);
    put(out, hs);
    put(out, ts);
    put(out, rows);

    const size_t state_floats = size_t(nj) * kSpringStateFloats, pal_floats = size_t(nb) * 16;
    std::vector<float> state(size_t(ni) * state_floats, std::nanf(""));
    for (uint32_t seg = 0; seg < n_segments; ++seg) {
        const std::vector<uint32_t> sh = take<uint32_t>(in, 2);
        if (sh[1]) state = take<float>(in, size_t(ni) * state_floats);
        for (uint32_t s = 0; s < sh[0]; ++s) {
            const float dt = take<float>(in, 1)[0];
            const uint32_t reset = take<uint32_t>(in, 1)[0];
            std::vector<float> pal = take<float>(in, size_t(ni) * pal_floats);
            for (uint32_t i = 0; i < ni; ++i) spring_step_instance(t, pal.data() + i * pal_floats, state.data() + i * state_floats, dt, reset != 0);
            put(out, pal);
            put(out, state);
        }
    }
    fclose(in);
    if (fclose(out) != 0) return 2;
    return 0;
}

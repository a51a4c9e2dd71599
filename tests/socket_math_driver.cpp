// tests/socket_math_driver.cpp -- the arithmetic header of mmdx_palette_sockets (simple_mmd_renderer_amd/csrc/socket_math.hpp, the
// very lines the gfx950 kernel compiles) and the host table builder (csrc/socket_table.hpp, what mmdx_socket_set_create uploads) on
// the CPU, as a stand-alone program.  Same rows in and out as tests/palette_sockets_driver.cpp: a line of stdin is the form of the
// offset (0 = none, 1 = pose, 2 = matrix), 16 floats of S, 4 of the rest position (three used) and 16 of an offset (a pose uses the
// first 8), each as the 8 hex digits of its bit pattern; a line of stdout is the 16 floats of the socket's matrix.  Every row is a
// one-socket desc that goes through socket_table_build -- a pose is expanded there, as in the library -- and then through socket_row
// per output row, all in heap buffers of exactly the size the code may touch, so an access past them is an AddressSanitizer report.
// Build: tests/host_program.py build(), plain and sanitize=True, from this file + csrc/error.cpp
// (tests/palette_sockets_ref.py).
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>

#include "../simple_mmd_renderer_amd/csrc/socket_table.hpp"

static float from_bits(uint32_t u) {
    float f;
    std::memcpy(&f, &u, 4);
    return f;
}
static uint32_t to_bits(float f) {
    uint32_t u;
    std::memcpy(&u, &f, 4);
    return u;
}

int main() {
    unsigned form;
    while (std::scanf("%u", &form) == 1) {
        float in[36];
        for (int k = 0; k < 36; ++k) {
            unsigned u;
            if (std::scanf("%x", &u) != 1) return 2;
            in[k] = from_bits(u);
        }
        const size_t no = form == 0 ? 0 : (form == 1 ? 8 : 16);
        std::unique_ptr<float[]> s(new float[16]), p(new float[3]), off(no ? new float[no] : nullptr), r(new float[16]);
        std::unique_ptr<uint32_t[]> bone(new uint32_t[1]);
        std::memcpy(s.get(), in, 16 * sizeof(float));
        std::memcpy(p.get(), in + 16, 3 * sizeof(float));
        if (no) std::memcpy(off.get(), in + 20, no * sizeof(float));
        bone[0] = 6;
        mmdx_socket_set_desc d{};
        d.struct_size = sizeof d;
        d.flags = form == 2 ? MMDX_SOCKET_OFFSET_MATRIX : 0;
        d.n_sockets = 1;
        d.bone = bone.get();
        d.rest_position = p.get();
        d.offset = off.get();
        std::vector<mmdx::SocketEntry> table;
        uint32_t n_offsets = 0;
        if (mmdx::socket_table_build(&d, 7, &table, &n_offsets) != MMDX_OK) return 3;
        if (table.size() != 1 || table[0].bone != 6 || n_offsets != (no ? 1u : 0u) || table[0].has_offset != n_offsets) return 4;
        std::unique_ptr<float[]> tp(new float[3]), to(no ? new float[16] : nullptr);
        std::memcpy(tp.get(), table[0].p, 3 * sizeof(float));
        if (no) std::memcpy(to.get(), table[0].o, 16 * sizeof(float));
        for (unsigned y = 0; y < 4; ++y) {
            std::unique_ptr<float[]> o(new float[4]);
            mmdx::socket_row(y, tp.get(), s.get(), to.get(), o.get());
            std::memcpy(r.get() + 4 * y, o.get(), 4 * sizeof(float));
        }
        for (int k = 0; k < 16; ++k) std::printf("%08x%c", to_bits(r[k]), k == 15 ? '\n' : ' ');
    }
    return 0;
}

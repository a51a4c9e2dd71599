// tests/place_math_driver.cpp -- the arithmetic header of mmdx_palette_place (simple_mmd_renderer_amd/csrc/place_math.hpp, the very
// lines the gfx950 kernel compiles) on the CPU, as a stand-alone program.  Same rows in and out as tests/palette_place_driver.cpp:
// a line of stdin is the form (0 = pose, 1 = matrix), 16 floats of S and 16 floats of a placement (a pose uses the first 8), each as
// the 8 hex digits of its bit pattern; a line of stdout is the 16 floats of S * W.  Every row goes through heap buffers of exactly
// the size the header may touch (16, 8 or 16, 16, 4 floats), so an access past them is an AddressSanitizer report.
// Build: tests/host_program.py build(), plain and sanitize=True (called from tests/palette_place_ref.py).
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>

#include "../simple_mmd_renderer_amd/csrc/place_math.hpp"

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
        float in[32];
        for (int k = 0; k < 32; ++k) {
            unsigned u;
            if (std::scanf("%x", &u) != 1) return 2;
            in[k] = from_bits(u);
        }
        const size_t np = form == 0 ? 8 : 16;
        std::unique_ptr<float[]> s(new float[16]), p(new float[np]), w(new float[16]), r(new float[16]);
        std::memcpy(s.get(), in, 16 * sizeof(float));
        std::memcpy(p.get(), in + 16, np * sizeof(float));
        if (form == 0)
            mmdx::place_matrix_from_pose(p.get(), w.get());
        else
            std::memcpy(w.get(), p.get(), 16 * sizeof(float));
        for (int y = 0; y < 4; ++y) {
            std::unique_ptr<float[]> o(new float[4]);
            mmdx::place_row(s[4 * y], s[4 * y + 1], s[4 * y + 2], s[4 * y + 3], w.get(), o.get());
            std::memcpy(r.get() + 4 * y, o.get(), 4 * sizeof(float));
        }
        for (int k = 0; k < 16; ++k) std::printf("%08x%c", to_bits(r[k]), k == 15 ? '\n' : ' ');
    }
    return 0;
}

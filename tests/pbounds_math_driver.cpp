// tests/pbounds_math_driver.cpp -- the arithmetic header of mmdx_palette_bounds (simple_mmd_renderer_amd/csrc/pbounds_math.hpp, the
// very lines the gfx950 kernel compiles) on the CPU, as a stand-alone program.  stdin: "n ni eps morph_scale pos_scale", then n
// table rows of 9 floats (lo, hi, reach), then ni * n matrices of 16 floats (instance-major: the matrix of each row's bone); every
// float as the 8 hex digits of its bit pattern.  stdout: ni rows of 6 floats.  Every row goes through heap buffers of exactly the
// size the header may touch, so an access past them is an AddressSanitizer report.
// Build: tests/host_program.py build(), plain and sanitize=True (called from tests/palette_bounds_ref.py).
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "../simple_mmd_renderer_amd/csrc/pbounds_math.hpp"

static bool read_float(float *f) {
    unsigned u;
    if (std::scanf("%x", &u) != 1) return false;
    const uint32_t v = u;
    std::memcpy(f, &v, 4);
    return true;
}
static uint32_t to_bits(float f) {
    uint32_t u;
    std::memcpy(&u, &f, 4);
    return u;
}

int main() {
    unsigned n, ni;
    float eps, ms, pos_scale;
    if (std::scanf("%u %u", &n, &ni) != 2 || !read_float(&eps) || !read_float(&ms) || !read_float(&pos_scale)) return 2;
    std::vector<std::unique_ptr<float[]>> lo, hi, reach;
    for (unsigned r = 0; r < n; ++r) {
        for (auto *v : {&lo, &hi, &reach}) {
            v->emplace_back(new float[3]);
            for (int c = 0; c < 3; ++c)
                if (!read_float(&v->back()[c])) return 2;
        }
    }
    for (unsigned i = 0; i < ni; ++i) {
        mmdx::PBoundsAcc acc;
        mmdx::pbounds_init(acc);
        for (unsigned r = 0; r < n; ++r) {
            std::unique_ptr<float[]> m(new float[16]), blo(new float[3]), bhi(new float[3]);
            for (int k = 0; k < 16; ++k)
                if (!read_float(&m[k])) return 2;
            mmdx::pbounds_row(lo[r].get(), hi[r].get(), reach[r].get(), ms, m.get(), eps, blo.get(), bhi.get());
            mmdx::pbounds_fold(acc, blo.get(), bhi.get());
        }
        std::unique_ptr<float[]> out(new float[6]);
        mmdx::pbounds_finish(acc.kmin, acc.kmax, acc.nan || n == 0, pos_scale, out.get());
        for (int c = 0; c < 6; ++c) std::printf("%08x%c", to_bits(out[c]), c == 5 ? '\n' : ' ');
    }
    return 0;
}

// bone_mask_driver.cpp -- csrc/bone_mask.hpp as a stand-alone program, for tests/test_row_blend_cpu.py to build under the sanitizers
// (tests/host_program.py: build(..., sanitize=True)) and run on the cases it gives mmdx_skeleton_subtree_mask:
//     bone_mask_driver NB parent[0] .. parent[NB-1] N_ROOTS root[0] .. root[N_ROOTS-1] inside outside
// prints "BAD k" when roots[k] is no bone (and checks that nothing was written), else the NB mask values, one per line, as the
// hexadecimal bit pattern of the float.  The arrays are heap allocations of exactly their sizes, so a read or write past either
// end is the sanitizer's to report.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>

#include "../simple_mmd_renderer_amd/csrc/bone_mask.hpp"

int main(int argc, char **argv) {
    int at = 1;
    auto next = [&]() -> const char * {
        if (at >= argc) { std::fprintf(stderr, "too few arguments\n"); std::exit(2); }
        return argv[at++];
    };
    const uint32_t nb = uint32_t(std::strtoul(next(), nullptr, 10));
    std::unique_ptr<int32_t[]> parent(new int32_t[nb]);
    for (uint32_t b = 0; b < nb; ++b) parent[b] = int32_t(std::strtol(next(), nullptr, 10));
    const uint32_t n_roots = uint32_t(std::strtoul(next(), nullptr, 10));
    std::unique_ptr<uint32_t[]> roots(new uint32_t[n_roots]);
    for (uint32_t r = 0; r < n_roots; ++r) roots[r] = uint32_t(std::strtoul(next(), nullptr, 10));
    const float inside = std::strtof(next(), nullptr), outside = std::strtof(next(), nullptr);
    std::unique_ptr<float[]> out(new float[nb]);
    const uint32_t untouched = 0x7FC12345u;
    for (uint32_t b = 0; b < nb; ++b) std::memcpy(&out[b], &untouched, 4);
    const int64_t bad = mmdx::subtree_mask(parent.get(), nb, roots.get(), n_roots, inside, outside, out.get());
    if (bad >= 0) {
        for (uint32_t b = 0; b < nb; ++b)
            if (std::memcmp(&out[b], &untouched, 4) != 0) { std::fprintf(stderr, "out[%u] written on a refusal\n", b); return 1; }
        std::printf("BAD %lld\n", static_cast<long long>(bad));
        return 0;
    }
    for (uint32_t b = 0; b < nb; ++b) {
        uint32_t bits;
        std::memcpy(&bits, &out[b], 4);
        std::printf("%08x\n", bits);
    }
    return 0;
}

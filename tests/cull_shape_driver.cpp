// CPU driver of the cull planner (simple_mmd_renderer_amd/csrc/cull_shape.cpp), built by tests/test_cull_bounds.py with g++ under
// ASan + UBSan from this file and cull_shape.cpp alone.
//   cull_shape_driver sweep     the planner over crowd sizes x forced forms x chunk overrides; every shape is checked against the
//                               rules the header states (no measured number besides the crossover constant); prints the row count
//   cull_shape_driver eval      one call per line on stdin: ni form chunk (the overrides as MMDX_CULL_FORM / MMDX_CULL_CHUNK give
//                               them, 0 = not set); its shape per line on stdout
#include <cinttypes>
#include <cstdio>
#include <cstring>

#include "../simple_mmd_renderer_amd/csrc/cull_shape.hpp"

using namespace mmdx;

namespace {

int sweep() {
    const uint32_t nis[] = {0, 1, 63, 64, 65, 200, 1023, 1024, 1025, 2500, 4095, 4096, 4097, 16384, 262144, 262145, 1u << 31, 0xFFFFFFFFu};
    const int forms[] = {-1, 0, 1, 2, 3};
    const int chunks[] = {-64, 0, 1, 63, 64, 65, 127, 128, 200, 256, 1000, 1023, 1024, 1025, 4096, 1 << 30};
    uint64_t rows = 0, failures = 0;
    for (uint32_t ni : nis)
        for (int form : forms)
            for (int chunk : chunks) {
                const CullShape s = plan_cull_launch(ni, CullOverrides{form, chunk});
                ++rows;
                bool ok = s.form == 1 || s.form == 2;
                if (form == 1 || form == 2) ok = ok && s.form == uint32_t(form);
                else ok = ok && s.form == (ni <= kCullCrossover ? 1u : 2u);
                ok = ok && s.chunk % 64 == 0 && s.chunk >= kCullMinChunk && s.chunk <= kCullMaxChunk && s.threads == s.chunk;
                if (chunk >= 64 && chunk <= 1024) ok = ok && s.chunk == uint32_t(chunk) / 64 * 64;
                if (chunk > 1024) ok = ok && s.chunk == 1024;
                if (chunk > 0 && chunk < 64) ok = ok && s.chunk == 64;
                // the chunks cover the crowd, the last one is not empty (except the one chunk of an empty crowd)
                ok = ok && s.nchunks >= 1 && uint64_t(s.nchunks) * s.chunk >= ni && (uint64_t(s.nchunks) - 1) * s.chunk < (ni ? ni : 1u);
                ok = ok && s.scratch_bytes == (s.form == 2 ? size_t(s.nchunks) * 16 : 0);
                if (!ok) {
                    ++failures;
                    std::fprintf(stderr, "ERROR ni=%" PRIu32 " form=%d chunk=%d -> form=%" PRIu32 " chunk=%" PRIu32 " nchunks=%" PRIu32 "\n", ni, form,
                                 chunk, s.form, s.chunk, s.nchunks);
                }
            }
    std::printf("rows=%" PRIu64 " failures=%" PRIu64 "\n", rows, failures);
    return failures ? 1 : 0;
}

int eval() {
    uint32_t ni;
    int form, chunk;
    while (std::scanf("%" SCNu32 " %d %d", &ni, &form, &chunk) == 3) {
        const CullShape s = plan_cull_launch(ni, CullOverrides{form, chunk});
        std::printf("form=%" PRIu32 " chunk=%" PRIu32 " threads=%" PRIu32 " nchunks=%" PRIu32 " scratch=%zu\n", s.form, s.chunk, s.threads,
                    s.nchunks, s.scratch_bytes);
    }
    return 0;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc == 2 && !std::strcmp(argv[1], "sweep")) return sweep();
    if (argc == 2 && !std::strcmp(argv[1], "eval")) return eval();
    std::fprintf(stderr, "usage: cull_shape_driver sweep | eval\n");
    return 2;
}

// CPU driver of the ordered solver's variant decision (simple_mmd_renderer_amd/csrc/solve_shape.hpp), built by
// tests/test_solve_dense.py with g++ under ASan + UBSan from this file alone (the decision is an inline function).
//   solve_shape_driver sweep    plan_solve_dense over nested x LDS sizes x workgroups x CU counts x MMDX_SOLVE_DENSE values; every
//                               answer is checked against the rules the header states, written out here a second time; prints the
//                               row count
//   solve_shape_driver eval     one call per line on stdin: nested lds workgroups cus env; 0 | 1 per line on stdout
#include <cinttypes>
#include <cstdio>
#include <cstring>

#include "../simple_mmd_renderer_amd/csrc/solve_shape.hpp"

using namespace mmdx;

namespace {

int sweep() {
    // 2 * (lds + 1024) <= 160 KB  <=>  lds <= 80 896: the bound, its neighbours, the 64 KB a kernel gets without asking, the 95 KB of
    // eight 6-link windows (tests/test_rig.py), the whole LDS of a CU
    const size_t ldss[] = {0, 4, 11776, 65536, 80892, 80895, 80896, 80897, 80900, 97280, 163840};
    const uint32_t cuss[] = {1, 64, 256, 304};
    const int envs[] = {-1, 0, 1, 2, -7};
    uint64_t rows = 0, failures = 0;
    for (int nested = 0; nested < 2; ++nested)
        for (size_t lds : ldss)
            for (uint32_t cus : cuss) {
                const uint32_t wgss[] = {1, 3, cus - 1, cus, cus + 1, 2 * cus, 1u << 20, 0xFFFFFFFFu};
                for (uint32_t wgs : wgss)
                    for (int env : envs) {
                        const bool got = plan_solve_dense(nested != 0, lds, wgs, cus, env);
                        ++rows;
                        bool want;
                        if (nested) want = false;                                    // under any env value
                        else if (2 * (uint64_t(lds) + 1024) > 160 * 1024) want = false;   // two workgroups do not fit a CU
                        else if (env == 1) want = true;                              // whenever it fits
                        else if (env == 0) want = false;                             // never
                        else want = wgs > cus;                                       // by crowd size
                        if (got != want) {
                            ++failures;
                            std::fprintf(stderr, "ERROR nested=%d lds=%zu wgs=%" PRIu32 " cus=%" PRIu32 " env=%d -> %d, want %d\n", nested, lds,
                                         wgs, cus, env, int(got), int(want));
                        }
                    }
            }
    std::printf("rows=%" PRIu64 " failures=%" PRIu64 "\n", rows, failures);
    return failures ? 1 : 0;
}

int eval() {
    int nested, env;
    unsigned long long lds;
    uint32_t wgs, cus;
    while (std::scanf("%d %llu %" SCNu32 " %" SCNu32 " %d", &nested, &lds, &wgs, &cus, &env) == 5)
        std::printf("%d\n", int(plan_solve_dense(nested != 0, size_t(lds), wgs, cus, env)));
    return 0;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc == 2 && !std::strcmp(argv[1], "sweep")) return sweep();
    if (argc == 2 && !std::strcmp(argv[1], "eval")) return eval();
    std::fprintf(stderr, "usage: solve_shape_driver sweep | eval\n");
    return 2;
}

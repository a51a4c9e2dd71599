// bone_mask.hpp -- mmdx_skeleton_subtree_mask (include/mmdx.h): the walk over a skeleton's parent array that fills a per-bone mask
// row for mmdx_pose_blend.  Host code with no HIP include: rig_api.cpp calls it, and the stand-alone CPU driver of the tests
// (tests/bone_mask_driver.cpp) compiles it under the sanitizers.
#pragma once

#include <cstdint>
#include <vector>

namespace mmdx {

// out[b] = inside when b or one of its ancestors is in roots[0 .. n_roots), else outside.  `parent` is mmdx_skeleton_desc.parent as
// the caller gave it: a value outside [0, nb) ends a chain, and a chain is followed for at most nb steps (a cycle ends there).
// Returns the position in `roots` of the first root >= nb (nothing is written then), or -1.
inline int64_t subtree_mask(const int32_t *parent, uint32_t nb, const uint32_t *roots, uint32_t n_roots, float inside, float outside,
                            float *out) {
    for (uint32_t r = 0; r < n_roots; ++r)
        if (roots[r] >= nb) return int64_t(r);
    std::vector<uint8_t> is_root(nb, 0);
    for (uint32_t r = 0; r < n_roots; ++r) is_root[roots[r]] = 1;
    for (uint32_t b = 0; b < nb; ++b) {
        bool in = false;
        uint32_t c = b;
        for (uint32_t step = 0; step <= nb; ++step) {        // b itself, then at most nb parents
            if (is_root[c]) { in = true; break; }
            const int32_t p = parent[c];
            if (p < 0 || uint32_t(p) >= nb || step == nb) break;
            c = uint32_t(p);
        }
        out[b] = in ? inside : outside;
    }
    return -1;
}

}  // namespace mmdx

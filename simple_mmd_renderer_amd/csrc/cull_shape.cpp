// cull_shape.cpp -- see cull_shape.hpp.
#include "cull_shape.hpp"

#include <algorithm>

namespace mmdx {

CullShape plan_cull_launch(uint32_t ni, const CullOverrides &ov) {
    CullShape s{};
    s.form = (ov.form == 1 || ov.form == 2) ? uint32_t(ov.form) : (ni <= kCullCrossover ? 1u : 2u);
    // Defaults (unmeasured, like the crossover): the one workgroup of form 1 brings as many lanes as a workgroup can have; form 2
    // takes smaller chunks so that a crowd just above the crossover already spreads over tens of CUs.
    uint32_t chunk = s.form == 1 ? kCullMaxChunk : 256u;
    if (ov.chunk > 0) chunk = std::min(std::max(uint32_t(ov.chunk) / 64u * 64u, kCullMinChunk), kCullMaxChunk);
    s.chunk = s.threads = chunk;
    s.nchunks = std::max<uint32_t>(1u, uint32_t((uint64_t(ni) + chunk - 1) / chunk));
    s.scratch_bytes = s.form == 2 ? size_t(s.nchunks) * 16 : 0;
    return s;
}

}  // namespace mmdx

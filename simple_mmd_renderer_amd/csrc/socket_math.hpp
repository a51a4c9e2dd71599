// socket_math.hpp -- the arithmetic of mmdx_palette_sockets (include/mmdx.h), once: the gfx950 kernel (socket_kernels.hip), the host
// table builder (socket_api.cpp) and a CPU driver (tests/socket_math_driver.cpp) compile these same lines, and
// tests/golden/palette_sockets_expect.npz (the real libmmd) pins them.  Every operation is binary32 in the order written; every
// build passes -ffp-contract=off, so nothing is fused.  The products are place_row of place_math.hpp, called and not restated.
//
// For a socket on bone b with rest position p, and S = that bone's skinning matrix in v[0..15] order:
//     G   = the identity with row 4 = {p.x, p.y, p.z, 1}        libmmd's global_offset_matrix_inv_ (L/motion/poser_impl.inl:36-37)
//     B   = G * S                                               Matrix4x4<float>::operator* (L/util/math_impl.inl:984-1003)
//     out = B, or O * B for a socket with a local offset O      (row-vector convention: O is the attachment's frame in the bone's)
// Every element is the left-to-right four-term sum, the rows where G is 0 and 1 included: no short circuits, so a -0 can become +0
// and an infinite element of S times a zero of G is NaN.
// What this is and is not: on a model-space palette B is the bone's model-space frame; on a palette that went through
// mmdx_palette_place it is the bone's world frame, because G * (S * W).  Rows 1-3 of B reproduce local_matrix_'s rows 1-3 bit for bit
// when S is finite, up to the sign of zero.  Row 4 is a recomputation and can differ from libmmd's private local_matrix_ row 4 in the
// last bits: the contract is the formula above, not that private field.  NaN sign and payload are outside the contract.
#pragma once

#include "place_math.hpp"

namespace mmdx {

// O of a pose-form offset {tx, ty, tz, (ignored), qx, qy, qz, qw}: what a placement of that form is to mmdx_palette_place.
MMDX_PLACE_FN void socket_offset_from_pose(const float *pose, float *o) { place_matrix_from_pose(pose, o); }

// Row r (0..3) of B = G * S.  p: 3 floats, s: 16 floats, b: 4 floats.
MMDX_PLACE_FN void socket_bone_row(unsigned r, const float *p, const float *s, float *b) {
    const bool last = r == 3;
    place_row(last ? p[0] : (r == 0 ? 1.0f : 0.0f), last ? p[1] : (r == 1 ? 1.0f : 0.0f), last ? p[2] : (r == 2 ? 1.0f : 0.0f),
              last ? 1.0f : 0.0f, s, b);
}

// Row r of a socket's matrix: of B, or -- offset != nullptr, 16 floats -- of O * B.  out: 4 floats.
MMDX_PLACE_FN void socket_row(unsigned r, const float *p, const float *s, const float *offset, float *out) {
    if (!offset) {
        socket_bone_row(r, p, s, out);
        return;
    }
    float b[16];
    for (unsigned y = 0; y < 4; ++y) socket_bone_row(y, p, s, b + 4 * y);
    // (selects with constant indices, not offset[4 * r + c]: in the kernel r differs per lane and O sits in scalar registers)
    float a[4];
    for (unsigned c = 0; c < 4; ++c) a[c] = r == 0 ? offset[c] : (r == 1 ? offset[4 + c] : (r == 2 ? offset[8 + c] : offset[12 + c]));
    place_row(a[0], a[1], a[2], a[3], b, out);
}

}  // namespace mmdx

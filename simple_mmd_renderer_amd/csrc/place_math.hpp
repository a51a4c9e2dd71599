// place_math.hpp -- the arithmetic of mmdx_palette_place (include/mmdx.h), once: the gfx950 kernel (place_kernels.hip) and a CPU
// driver (tests/place_math_driver.cpp) compile these same lines, and tests/golden/palette_place_expect.npz (the real libmmd) pins
// them.  Every operation is binary32 in the order written; both builds pass -ffp-contract=off, so nothing is fused.
// rig_kernels.hip keeps its own q_to_matrix / mul: moving them has changed existing kernels' code before.
#pragma once

#if defined(__HIPCC__)
#define MMDX_PLACE_FN __host__ __device__ __forceinline__
#else
#define MMDX_PLACE_FN inline
#endif

namespace mmdx {

// W of the pose form: pose = {tx, ty, tz, (ignored), qx, qy, qz, qw} -> w[16] in v[0..15] order.  Quaternion::ToRotateMatrix
// (L/util/math_impl.inl:540-563; i, j, k, e = x, y, z, w; not normalised), then row 4 = {tx, ty, tz, 1} as
// local_matrix_.r.v[3].downgrade.vector3d = translation leaves it (L/motion/poser_impl.inl:161-162).
MMDX_PLACE_FN void place_matrix_from_pose(const float *pose, float *w) {
    const float i = pose[4], j = pose[5], k = pose[6], e = pose[7];
    const float ii = i * i, jj = j * j, kk = k * k, ij = i * j, jk = j * k, ki = i * k, ie = i * e, je = j * e, ke = k * e;
    w[0] = 1.0f - 2.0f * (jj + kk); w[1] = 2.0f * (ij + ke);         w[2] = 2.0f * (ki - je);          w[3] = 0.0f;
    w[4] = 2.0f * (ij - ke);        w[5] = 1.0f - 2.0f * (kk + ii);  w[6] = 2.0f * (jk + ie);          w[7] = 0.0f;
    w[8] = 2.0f * (ki + je);        w[9] = 2.0f * (jk - ie);         w[10] = 1.0f - 2.0f * (ii + jj);  w[11] = 0.0f;
    w[12] = pose[0];                w[13] = pose[1];                 w[14] = pose[2];                  w[15] = 1.0f;
}

// One row of Matrix4x4::operator* (L/util/math_impl.inl:984-1003): o[c] = a1*w[c] + a2*w[4+c] + a3*w[8+c] + a4*w[12+c], left to
// right.  No short circuit for zeros or an identity W.
MMDX_PLACE_FN void place_row(float a1, float a2, float a3, float a4, const float *w, float *o) {
    o[0] = a1 * w[0] + a2 * w[4] + a3 * w[8] + a4 * w[12];
    o[1] = a1 * w[1] + a2 * w[5] + a3 * w[9] + a4 * w[13];
    o[2] = a1 * w[2] + a2 * w[6] + a3 * w[10] + a4 * w[14];
    o[3] = a1 * w[3] + a2 * w[7] + a3 * w[11] + a4 * w[15];
}

}  // namespace mmdx

// place_kernels.hip -- mmdx_palette_place on gfx950: out[i][b] = S[i][b] * W[i], Matrix4x4::operator* of libmmd (include/mmdx.h
// states the arithmetic; place_math.hpp holds it, shared with the CPU driver of the tests; this file is built with
// -ffp-contract=off like the rest, and models created with MMDX_CREATE_FAST_MATH run this same kernel).
//
// one lane per matrix ROW   the palette is ni * nb * 4 rows of 16 bytes.  A lane loads one row, computes row * W (16 multiplies, 12
//                           adds) and stores one row: a wave's loads and stores are 1 KB contiguous each, the kernel is a stream of
//                           one read and one write per byte.  A lane touches no row but its own, which is what makes in-place
//                           (out == palettes) safe; the two pointers are therefore NOT __restrict__.
// W[i] is wave-uniform      blockIdx.x = instance, blockIdx.y = a chunk of that instance's nb * 4 rows, so a workgroup never spans
//                           two instances.  The placement's address depends on blockIdx.x alone and is read before any store of
//                           the kernel: the compiler fetches it with scalar loads (8 or 16 dwords) and, in pose form, builds W in
//                           scalar/vector registers.  No LDS.
#include <hip/hip_runtime.h>

#include "place_kernels.hpp"
#include "place_math.hpp"

namespace mmdx {

namespace {

template <bool kMatrix>
__global__ __launch_bounds__(kPlaceThreads) void palette_place_kernel(const float4 *palettes, const float *__restrict__ placements,
                                                                      float4 *out, uint32_t rows) {
    const uint32_t i = blockIdx.x;
    const float *p = placements + size_t(i) * (kMatrix ? 16 : 8);
    float w[16];
    if (kMatrix) {
#pragma unroll
        for (int k = 0; k < 16; ++k) w[k] = p[k];
    } else {
        float pose[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) pose[k] = p[k];
        place_matrix_from_pose(pose, w);
    }
    const uint32_t r = blockIdx.y * blockDim.x + threadIdx.x;      // < 65535 * 256: no overflow
    if (r >= rows) return;
    const size_t at = size_t(i) * rows + r;
    const float4 a = palettes[at];
    float o[4];
    place_row(a.x, a.y, a.z, a.w, w, o);
    out[at] = make_float4(o[0], o[1], o[2], o[3]);
}

}  // namespace

hipError_t launch_palette_place(const PlaceLaunch &p, hipStream_t stream) {
    const uint32_t rows = p.nb * 4;
    const dim3 grid(p.ni, place_chunks(p.nb)), block(place_threads(p.nb));
    const float4 *in = reinterpret_cast<const float4 *>(p.palettes);
    float4 *out = reinterpret_cast<float4 *>(p.out);
    if (p.matrix)
        hipLaunchKernelGGL(palette_place_kernel<true>, grid, block, 0, stream, in, p.placements, out, rows);
    else
        hipLaunchKernelGGL(palette_place_kernel<false>, grid, block, 0, stream, in, p.placements, out, rows);
    return hipGetLastError();
}

}  // namespace mmdx

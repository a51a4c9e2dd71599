// socket_kernels.hip -- mmdx_palette_sockets on gfx950: out[s][i] = (O[s] *) G[s] * S[i][bone[s]], Matrix4x4::operator* of libmmd
// (include/mmdx.h states the arithmetic; socket_math.hpp holds it, shared with the host table builder and the CPU driver of the
// tests; this file is built with -ffp-contract=off like the rest, and models created with MMDX_CREATE_FAST_MATH run this same kernel).
//
// the socket is wave-uniform  blockIdx.y = socket: its table row {bone, p, has_offset, O} depends on blockIdx.y alone and never
//                             overlaps the output, so it arrives through scalar loads (24 dwords).
// four lanes per matrix       consecutive lanes are consecutive (instance, output row) pairs: lane 4k + r computes row r of the
//                             matrix of instance (select form: list position) k and stores its 16 bytes, so a wave's stores into
//                             slab s are 1 KB contiguous.  Each lane loads the whole 64-byte S it multiplies (the product has no
//                             short circuit, so every row of the result reads every row of S); the four lanes of a matrix share the
//                             line, and instances are NB * 64 bytes apart.  A lane writes no row but its own, so an id listed twice
//                             stores the same bytes twice.  No LDS, no atomics.
// palettes and out never overlap (socket_api.cpp refuses that), hence __restrict__.
#include <hip/hip_runtime.h>

#include "socket_kernels.hpp"
#include "socket_math.hpp"

namespace mmdx {

namespace {

template <bool kOffsets, bool kSelect>
__global__ __launch_bounds__(kSocketThreads) void palette_sockets_kernel(const float4 *__restrict__ palettes,
                                                                         const SocketEntry *__restrict__ table, float4 *__restrict__ out,
                                                                         uint32_t ni, uint32_t nb, uint32_t cells, const InstanceList list) {
    const SocketEntry &e = table[blockIdx.y];
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;      // < 2^23 * 4 + 256: no overflow
    const uint32_t k = t >> 2, r = t & 3u;
    uint32_t i = k;
    if (kSelect) {
        const ListedInstances li{list};
        const Lane ln = li.lane(k, li.used(cells));
        if (!ln.live) return;
        i = ln.row;
    } else if (k >= ni) {
        return;
    }
    const float4 *src = palettes + (size_t(i) * nb + e.bone) * 4;
    const float4 s0 = src[0], s1 = src[1], s2 = src[2], s3 = src[3];
    const float s[16] = {s0.x, s0.y, s0.z, s0.w, s1.x, s1.y, s1.z, s1.w, s2.x, s2.y, s2.z, s2.w, s3.x, s3.y, s3.z, s3.w};
    const float p[3] = {e.p[0], e.p[1], e.p[2]};
    float o[4];
    if (kOffsets && e.has_offset) {
        float off[16];
#pragma unroll
        for (int c = 0; c < 16; ++c) off[c] = e.o[c];
        socket_row(r, p, s, off, o);
    } else {
        socket_row(r, p, s, nullptr, o);
    }
    out[(size_t(blockIdx.y) * ni + i) * 4 + r] = make_float4(o[0], o[1], o[2], o[3]);
}

template <bool kOffsets>
void launch(const SocketLaunch &p, const InstanceList *list, uint32_t cells, hipStream_t stream) {
    const uint32_t n = list ? cells : p.ni;
    const dim3 grid(socket_chunks(n), p.ns), block(socket_threads(n));
    const float4 *in = reinterpret_cast<const float4 *>(p.palettes);
    float4 *out = reinterpret_cast<float4 *>(p.out);
    if (list)
        hipLaunchKernelGGL((palette_sockets_kernel<kOffsets, true>), grid, block, 0, stream, in, p.table, out, p.ni, p.nb, cells, *list);
    else
        hipLaunchKernelGGL((palette_sockets_kernel<kOffsets, false>), grid, block, 0, stream, in, p.table, out, p.ni, p.nb, n,
                           InstanceList{nullptr, nullptr, p.ni});
}

}  // namespace

hipError_t launch_palette_sockets(const SocketLaunch &p, const InstanceList *list, uint32_t cells, hipStream_t stream) {
    if (p.any_offset) launch<true>(p, list, cells, stream);
    else launch<false>(p, list, cells, stream);
    return hipGetLastError();
}

}  // namespace mmdx

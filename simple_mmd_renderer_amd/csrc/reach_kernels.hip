// reach_kernels.hip -- mmdx_palette_reach on gfx950 (include/mmdx.h states the arithmetic; reach_math.hpp holds it, shared with the
// CPU driver of the tests; this file is built with -ffp-contract=off like the rest).
//
// the workgroup   256 lanes own (reach = blockIdx.y, 16 consecutive instances, select form: list positions).
// phase A         lane g < 16 is instance g of the block: the target (one 16-byte load; a scalar load when one target serves
//                 everyone), the rows of a, b and c as 16-byte loads, steps 0-5 of the header in registers, and C_0, C_1, C_2 -- 12
//                 floats each, the fourth column is {0, 0, 0, 1} -- into LDS, instance fastest (consecutive lanes, consecutive
//                 banks), with the word "applied" behind them.
// barrier
// phase B         the aim's, restated (aim_kernels.hip stays as it is): all lanes loop over (instance of the block, subtree row,
//                 matrix row r), r fastest, then the subtree row: four consecutive lanes move one 64-byte palette row, runs of
//                 consecutive bones coalesce.  A lane does one 16-byte load, place_row against its instance's matrix of the row's
//                 depth (the same LDS words for the four lanes of a row, and for every row of that depth: a broadcast) and one
//                 16-byte store.
// In place: phase A reads rows of the reach's own subtree only (a, b, c), rows that no other workgroup writes (the subtrees of a set
// are disjoint, the ids of a call distinct); phase B rewrites them behind the barrier, every lane the 16 bytes it loaded.  The
// palette pointer is not __restrict__: it is read and written.  No atomics, no scratch, vector stores only.
#include <hip/hip_runtime.h>

#include "place_math.hpp"
#include "reach_kernels.hpp"

namespace mmdx {

namespace {

constexpr uint32_t kReachUnroll = 4;               // phase B: palette pieces a lane has in flight

__device__ __forceinline__ void reach_load_row(const float4 *src, float *r) {
    const float4 a = src[0], b = src[1], c = src[2], d = src[3];
    r[0] = a.x; r[1] = a.y; r[2] = a.z; r[3] = a.w; r[4] = b.x; r[5] = b.y; r[6] = b.z; r[7] = b.w;
    r[8] = c.x; r[9] = c.y; r[10] = c.z; r[11] = c.w; r[12] = d.x; r[13] = d.y; r[14] = d.z; r[15] = d.w;
}

__device__ __forceinline__ void reach_keep(const float *c, float *dst) {      // 12 floats of a matrix, instance fastest
#pragma unroll
    for (uint32_t r = 0; r < 4; ++r)
#pragma unroll
        for (uint32_t j = 0; j < 3; ++j) dst[(r * 3 + j) * kReachBlock] = c[4 * r + j];
}

template <bool kSelect>
__global__ __launch_bounds__(kReachThreads) void reach_kernel(const ReachLaunch p, const InstanceList list, uint32_t cells) {
    extern __shared__ float lds[];                                      // [3][12][16], then [16] "applied"
    uint32_t *applied_of = reinterpret_cast<uint32_t *>(lds + kReachDepths * kReachMatrixFloats * kReachBlock);
    const ReachReach &m = p.reaches[blockIdx.y];
    const uint32_t base = blockIdx.x * kReachBlock;                     // < 2^23 + 16
    const ListedInstances li{list};
    const uint32_t used = kSelect ? li.used(cells) : p.ni;
    if (base >= used) return;                                           // (uniform: the whole workgroup is behind the count)
    float4 *pal = reinterpret_cast<float4 *>(p.palettes);

    const uint32_t g = threadIdx.x;
    if (g < kReachBlock) {                                              // ---- phase A
        uint32_t i = base + g, applied = 0;
        bool live = i < used;
        if (kSelect) {
            const Lane ln = li.lane(base + g, used);
            live = ln.live;
            i = ln.row;
        }
        if (live) {
            float tgt[4];
            if (p.target_stride) {
                const float4 t4 = *reinterpret_cast<const float4 *>(p.targets + size_t(i) * p.target_stride);
                tgt[0] = t4.x; tgt[1] = t4.y; tgt[2] = t4.z; tgt[3] = t4.w;
            } else {
                tgt[0] = p.targets[0]; tgt[1] = p.targets[1]; tgt[2] = p.targets[2]; tgt[3] = p.targets[3];
            }
            const float w = reach_weight(tgt);
            if (w > 0.0f) {
                const float4 *rows = pal + size_t(i) * p.nb * 4;
                float ra[16], rb[16], rc[16], c0[16], c1[16], c2[16];
                reach_load_row(rows + size_t(m.a) * 4, ra);
                reach_load_row(rows + size_t(m.b) * 4, rb);
                reach_load_row(rows + size_t(m.c) * 4, rc);
                if (reach_solve(ra, rb, rc, m, tgt, w, c0, c1, c2)) {
                    applied = 1;
                    reach_keep(c0, lds + g);
                    reach_keep(c1, lds + kReachMatrixFloats * kReachBlock + g);
                    reach_keep(c2, lds + 2 * kReachMatrixFloats * kReachBlock + g);
                }
            }
        }
        applied_of[g] = applied;
    }
    __syncthreads();

    const uint32_t per = m.n_rows * 4, total = kReachBlock * per;       // ---- phase B  (total <= 16 * 2^20 * 4: kReachMaxBones)
    // kReachUnroll items to a lane and trip, every load of the trip requested before the first store: the palette pointer is read
    // and written, so the compiler keeps the order written here, and one load -> store round trip per trip is what a lane waits for.
    for (uint32_t item0 = threadIdx.x; item0 < total; item0 += kReachThreads * kReachUnroll) {
        float4 *at[kReachUnroll];
        float4 a[kReachUnroll];
        const float *src[kReachUnroll];
#pragma unroll
        for (uint32_t n = 0; n < kReachUnroll; ++n) {
            const uint32_t item = item0 + n * kReachThreads;
            at[n] = nullptr;
            if (item >= total) continue;
            const uint32_t gi = item / per, rem = item - gi * per;
            if (!applied_of[gi]) continue;                              // (dead positions and ids that are no instance included)
            const ReachRow s = p.rows[m.first_row + (rem >> 2)];
            uint32_t i = base + gi;
            if (kSelect) i = list.ids[i];                               // (a live position: phase A saw this id below n_rows)
            at[n] = pal + (size_t(i) * p.nb + s.bone) * 4 + (rem & 3u);
            a[n] = *at[n];
            src[n] = lds + size_t(s.depth) * kReachMatrixFloats * kReachBlock + gi;
        }
#pragma unroll
        for (uint32_t n = 0; n < kReachUnroll; ++n) {
            if (!at[n]) continue;
            float c[16], o[4];
#pragma unroll
            for (uint32_t rr = 0; rr < 4; ++rr) {
#pragma unroll
                for (uint32_t j = 0; j < 3; ++j) c[4 * rr + j] = src[n][(rr * 3 + j) * kReachBlock];
                c[4 * rr + 3] = rr == 3 ? 1.0f : 0.0f;
            }
            place_row(a[n].x, a[n].y, a[n].z, a[n].w, c, o);
            *at[n] = make_float4(o[0], o[1], o[2], o[3]);
        }
    }
}

}  // namespace

hipError_t launch_reach(const ReachLaunch &p, const ReachShape &shape, const InstanceList *list, uint32_t cells, hipStream_t stream) {
    const uint32_t n = list ? cells : p.ni;
    if (!n || !p.n_reaches) return hipSuccess;
    const dim3 grid(shape.nblocks, p.n_reaches), block(shape.threads);
    if (list)
        hipLaunchKernelGGL(reach_kernel<true>, grid, block, shape.lds, stream, p, *list, cells);
    else
        hipLaunchKernelGGL(reach_kernel<false>, grid, block, shape.lds, stream, p, InstanceList{nullptr, nullptr, p.ni}, n);
    return hipGetLastError();
}

}  // namespace mmdx

// aim_kernels.hip -- mmdx_palette_aim on gfx950 (include/mmdx.h states the arithmetic; aim_math.hpp holds it, shared with the CPU
// driver of the tests; this file is built with -ffp-contract=off like the rest).
//
// the workgroup   256 lanes own (aim = blockIdx.y, `block` = 16 or 64 consecutive instances, select form: list positions).
// phase A         lane g < block is instance g of the block: the target (one 16-byte load; a scalar load when one target serves
//                 everyone), the eye row and, link after link, the link's row as 16-byte loads, step 1 of the header in registers,
//                 and the cumulative matrix after every link -- 12 floats, the fourth column is {0, 0, 0, 1} -- into LDS, instance
//                 fastest (consecutive lanes, consecutive banks), with the index of the first applied link behind them.
// barrier
// phase B         all lanes loop over (instance of the block, subtree row, matrix row r), r fastest, then the subtree row: four
//                 consecutive lanes move one 64-byte palette row, runs of consecutive bones coalesce.  A lane does one 16-byte load,
//                 place_row against its instance's matrix of the row's depth (the same LDS words for the four lanes of a row, and for
//                 every row of that depth: a broadcast) and one 16-byte store.
// In place: phase A reads rows of the aim's own subtree only (links and eye), rows that no other workgroup writes (the subtrees of a
// set are disjoint, the ids of a call distinct); phase B rewrites them behind the barrier, every lane the 16 bytes it loaded.  The
// palette pointer is not __restrict__: it is read and written.  No atomics, no scratch, vector stores only.
#include <hip/hip_runtime.h>

#include "aim_kernels.hpp"
#include "place_math.hpp"

namespace mmdx {

namespace {

constexpr uint32_t kAimUnset = 0xFFFFFFFFu;        // the first applied link of an instance nothing is written for
constexpr uint32_t kAimUnroll = 4;                 // phase B: palette pieces a lane has in flight

__device__ __forceinline__ void load_row(const float4 *src, float *r) {
    const float4 a = src[0], b = src[1], c = src[2], d = src[3];
    r[0] = a.x; r[1] = a.y; r[2] = a.z; r[3] = a.w; r[4] = b.x; r[5] = b.y; r[6] = b.z; r[7] = b.w;
    r[8] = c.x; r[9] = c.y; r[10] = c.z; r[11] = c.w; r[12] = d.x; r[13] = d.y; r[14] = d.z; r[15] = d.w;
}

template <bool kSelect>
__global__ __launch_bounds__(kAimThreads) void aim_kernel(const AimLaunch p, const InstanceList list, uint32_t cells, uint32_t block) {
    extern __shared__ float lds[];                                      // [max_links][12][block], then [block] first applied links
    uint32_t *first_of = reinterpret_cast<uint32_t *>(lds + size_t(p.max_links) * kAimMatrixFloats * block);
    const AimAim &m = p.aims[blockIdx.y];
    const uint32_t base = blockIdx.x * block;                           // < 2^23 + 64
    const ListedInstances li{list};
    const uint32_t used = kSelect ? li.used(cells) : p.ni;
    if (base >= used) return;                                           // (uniform: the whole workgroup is behind the count)
    float4 *pal = reinterpret_cast<float4 *>(p.palettes);

    const uint32_t g = threadIdx.x;
    if (g < block) {                                                    // ---- phase A
        uint32_t i = base + g, first = kAimUnset;
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
            const float w = aim_weight(tgt);
            if (w > 0.0f) {
                const float4 *rows = pal + size_t(i) * p.nb * 4;
                const float e[3] = {m.e[0], m.e[1], m.e[2]}, f[3] = {m.f[0], m.f[1], m.f[2]};
                float q[16], c[16];
                load_row(rows + size_t(m.eye_bone) * 4, q);
                for (uint32_t l = 0; l < m.n_links; ++l) {
                    const AimLink &k = p.links[m.first_link + l];
                    float pr[16];
                    load_row(rows + size_t(k.bone) * 4, pr);
                    if (aim_link(pr, q, k, e, f, tgt, w, c, first != kAimUnset) && first == kAimUnset) first = l;
                    if (first != kAimUnset) {
                        float *dst = lds + size_t(l) * kAimMatrixFloats * block + g;
#pragma unroll
                        for (uint32_t r = 0; r < 4; ++r)
#pragma unroll
                            for (uint32_t j = 0; j < 3; ++j) dst[(r * 3 + j) * block] = c[4 * r + j];
                    }
                }
            }
        }
        first_of[g] = first;
    }
    __syncthreads();

    const uint32_t per = m.n_rows * 4, total = block * per;             // ---- phase B  (total <= 64 * 2^20 * 4: kAimMaxBones)
    // kAimUnroll items to a lane and trip, every load of the trip requested before the first store: the palette pointer is read and
    // written, so the compiler keeps the order written here, and one load -> store round trip per trip is what a lane waits for.
    for (uint32_t item0 = threadIdx.x; item0 < total; item0 += kAimThreads * kAimUnroll) {
        float4 *at[kAimUnroll];
        float4 a[kAimUnroll];
        const float *src[kAimUnroll];
#pragma unroll
        for (uint32_t n = 0; n < kAimUnroll; ++n) {
            const uint32_t item = item0 + n * kAimThreads;
            at[n] = nullptr;
            if (item >= total) continue;
            const uint32_t gi = item / per, rem = item - gi * per;
            const AimRow s = p.rows[m.first_row + (rem >> 2)];
            if (s.depth < first_of[gi]) continue;                       // (kAimUnset is above every depth)
            uint32_t i = base + gi;
            if (kSelect) i = list.ids[i];                               // (a live position: phase A saw this id below n_rows)
            at[n] = pal + (size_t(i) * p.nb + s.bone) * 4 + (rem & 3u);
            a[n] = *at[n];
            src[n] = lds + size_t(s.depth) * kAimMatrixFloats * block + gi;
        }
#pragma unroll
        for (uint32_t n = 0; n < kAimUnroll; ++n) {
            if (!at[n]) continue;
            float c[16], o[4];
#pragma unroll
            for (uint32_t rr = 0; rr < 4; ++rr) {
#pragma unroll
                for (uint32_t j = 0; j < 3; ++j) c[4 * rr + j] = src[n][(rr * 3 + j) * block];
                c[4 * rr + 3] = rr == 3 ? 1.0f : 0.0f;
            }
            place_row(a[n].x, a[n].y, a[n].z, a[n].w, c, o);
            *at[n] = make_float4(o[0], o[1], o[2], o[3]);
        }
    }
}

}  // namespace

hipError_t launch_aim(const AimLaunch &p, const AimShape &shape, const InstanceList *list, uint32_t cells, hipStream_t stream) {
    const uint32_t n = list ? cells : p.ni;
    if (!n || !p.n_aims) return hipSuccess;
    const dim3 grid(shape.nblocks, p.n_aims), block(shape.threads);
    if (list)
        hipLaunchKernelGGL(aim_kernel<true>, grid, block, shape.lds, stream, p, *list, cells, shape.block);
    else
        hipLaunchKernelGGL(aim_kernel<false>, grid, block, shape.lds, stream, p, InstanceList{nullptr, nullptr, p.ni}, n, shape.block);
    return hipGetLastError();
}

}  // namespace mmdx

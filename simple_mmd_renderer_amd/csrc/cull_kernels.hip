// cull_kernels.hip -- mmdx_cull_bounds on gfx950: the boxes of mmdx_deform_batched_bounds against up to 16 planes and up to 3 LOD
// distances, compacted into up to 4 instance lists IN ASCENDING INSTANCE ORDER (include/mmdx.h states the arithmetic; it is part of
// the contract and holds because this file is built with -ffp-contract=off like the rest).
//
// classify      one lane per instance.  A row is six consecutive floats = 24 bytes at a 4-byte aligned address, which global loads
//               of any width accept on gfx950: the compiler reads it as one 16-byte and one 8-byte load.  Planes, eye, margin and
//               distances are the same for every lane: scalar loads, from the view in device memory or from the kernel arguments.
// compaction    no atomic decides an order.  Within a wave: one ballot per level, the lane's rank = mbcnt of its level's ballot.
//               Across the waves of a workgroup: the waves' per-level counts in LDS, each wave adds up the waves before it.
// form 1        cull_walk_kernel, ONE workgroup: walks the crowd chunk by chunk and carries the four running bases in registers.
// form 2        cull_count_kernel writes per-chunk, per-level counts to the handle's scratch; in cull_scatter_kernel the workgroup of
//               chunk c sums the counts of chunks [0, c), classifies its chunk again (same arithmetic, same result) and scatters; the
//               last chunk's workgroup writes out_counts.
// No workgroup ever waits for another one: no look-back, no spinning, no flags -- the only ordering between workgroups is the kernel
// boundary between the count and the scatter launch.
#include <hip/hip_runtime.h>

#include "cull_kernels.hpp"

namespace mmdx {

namespace {

constexpr uint32_t kMaxWaves = kCullMaxChunk / 64;      // waves per workgroup at the largest chunk
constexpr uint32_t kLods = MMDX_CULL_MAX_LODS;

struct CullScalars {
    uint32_t ni, list_stride, chunk, nchunks;
};

// m(a, b) of the contract: a NaN in `a` gives b, a NaN in `b` gives NaN (not fmaxf)
__device__ __forceinline__ float m2(float a, float b) { return a > b ? a : b; }

// What the view holds besides its planes and distances, clamped as the header says a view that nobody could check is clamped
struct ViewHead {
    uint32_t n_planes, n_lods;
    float ex, ey, ez, margin;
};
__device__ __forceinline__ ViewHead view_head(const mmdx_cull_view &v) {
    ViewHead h;
    h.n_planes = min(v.n_planes, uint32_t(MMDX_CULL_MAX_PLANES));
    h.n_lods = min(max(v.n_lods, 1u), kLods);
    h.ex = v.eye[0]; h.ey = v.eye[1]; h.ez = v.eye[2];
    h.margin = v.margin;
    return h;
}

// The level of instance i (0 .. n_lods-1), or MMDX_CULLED
__device__ __forceinline__ uint32_t classify(const mmdx_cull_view &v, const ViewHead &h, const float *__restrict__ bounds, uint64_t i) {
    const float *row = bounds + i * 6;
    const float mnx = row[0], mny = row[1], mnz = row[2], mxx = row[3], mxy = row[4], mxz = row[5];
    const float lx = mnx - h.margin, ly = mny - h.margin, lz = mnz - h.margin;
    const float hx = mxx + h.margin, hy = mxy + h.margin, hz = mxz + h.margin;
    bool culled = false;
    for (uint32_t p = 0; p < h.n_planes; ++p) {
        const float a = v.planes[p][0], b = v.planes[p][1], c = v.planes[p][2], d = v.planes[p][3];
        const float px = a >= 0.0f ? hx : lx, py = b >= 0.0f ? hy : ly, pz = c >= 0.0f ? hz : lz;
        const float s = ((a * px + b * py) + c * pz) + d;
        culled |= s < 0.0f;
    }
    const float dx = m2(m2(mnx - h.ex, h.ex - mxx), 0.0f);
    const float dy = m2(m2(mny - h.ey, h.ey - mxy), 0.0f);
    const float dz = m2(m2(mnz - h.ez, h.ez - mxz), 0.0f);
    const float d2 = (dx * dx + dy * dy) + dz * dz;
    uint32_t level = 0;
    for (uint32_t k = 0; k + 1 < h.n_lods; ++k) {
        const float t = v.lod_distance[k];
        level += d2 >= t * t ? 1u : 0u;
    }
    return culled ? MMDX_CULLED : level;
}

__device__ __forceinline__ uint32_t pick4(uint32_t k, uint32_t a, uint32_t b, uint32_t c, uint32_t d) {
    return k == 0 ? a : (k == 1 ? b : (k == 2 ? c : d));
}

// The wave's ballots of one chunk: which lanes hold a visible instance of each level
struct Ballots {
    unsigned long long m[kLods];
};
__device__ __forceinline__ Ballots ballots_of(bool live, uint32_t cls) {
    Ballots b;
#pragma unroll
    for (uint32_t l = 0; l < kLods; ++l) b.m[l] = __ballot(live && cls == l);
    return b;
}
// lanes 0..3 of every wave publish the wave's count of their level
__device__ __forceinline__ void publish_counts(const Ballots &b, uint32_t lane, uint32_t *wave_counts /* [kLods] of this wave */) {
    if (lane < kLods) {
        const unsigned long long mine = lane == 0 ? b.m[0] : (lane == 1 ? b.m[1] : (lane == 2 ? b.m[2] : b.m[3]));
        wave_counts[lane] = uint32_t(__popcll(mine));
    }
}
// the lane's rank among the lanes of its wave that hold the same level
__device__ __forceinline__ uint32_t rank_in_wave(const Ballots &b, uint32_t cls) {
    const unsigned long long mine = cls == 0 ? b.m[0] : (cls == 1 ? b.m[1] : (cls == 2 ? b.m[2] : b.m[3]));
    return __builtin_amdgcn_mbcnt_hi(uint32_t(mine >> 32), __builtin_amdgcn_mbcnt_lo(uint32_t(mine), 0u));
}

// After the barrier behind publish_counts: per level, the instances in the waves before this one and in the whole chunk
__device__ __forceinline__ void wave_prefix(const uint32_t (*counts)[kLods], uint32_t nwaves, uint32_t wave, uint32_t before[kLods],
                                            uint32_t total[kLods]) {
#pragma unroll
    for (uint32_t l = 0; l < kLods; ++l) before[l] = total[l] = 0;
    for (uint32_t w = 0; w < nwaves; ++w) {
#pragma unroll
        for (uint32_t l = 0; l < kLods; ++l) {
            const uint32_t c = counts[w][l];
            total[l] += c;
            before[l] += w < wave ? c : 0u;
        }
    }
}

// The lane's instance goes to its list (a position at or behind list_stride cannot happen while bounds and view hold still between
// the count and the scatter launch; the test keeps a caller's race from becoming a store outside the lists)
__device__ __forceinline__ void scatter(uint32_t *__restrict__ out_ids, uint32_t *__restrict__ out_levels, const CullScalars &s, bool live,
                                        uint64_t i, uint32_t cls, uint32_t pos) {
    if (!live) return;
    if (out_levels) out_levels[i] = cls;
    if (cls != MMDX_CULLED && pos < s.list_stride) out_ids[size_t(cls) * s.list_stride + pos] = uint32_t(i);
}

// ---- form 1: one workgroup ------------------------------------------------------------------------------------------------------
template <bool DEV>
__global__ __launch_bounds__(kCullMaxChunk) void cull_walk_kernel(const float *__restrict__ bounds, const mmdx_cull_view *__restrict__ view_dev,
                                                                  const mmdx_cull_view view_arg, uint32_t *__restrict__ out_ids,
                                                                  uint32_t *__restrict__ out_counts, uint32_t *__restrict__ out_levels,
                                                                  const CullScalars s) {
    // two sets of wave counts: chunk k+1 may publish while a slow wave still reads chunk k's (one barrier per chunk)
    __shared__ uint32_t counts[2][kMaxWaves][kLods];
    const mmdx_cull_view &v = DEV ? *view_dev : view_arg;
    const ViewHead h = view_head(v);
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, nwaves = s.chunk >> 6;
    uint32_t base[kLods] = {0, 0, 0, 0};
    for (uint32_t c = 0; c < s.nchunks; ++c) {
        const uint64_t i = uint64_t(c) * s.chunk + tid;
        const bool live = i < s.ni;
        const uint32_t cls = live ? classify(v, h, bounds, i) : MMDX_CULLED;
        const Ballots b = ballots_of(live, cls);
        publish_counts(b, lane, counts[c & 1u][wave]);
        __syncthreads();
        uint32_t before[kLods], total[kLods];
        wave_prefix(counts[c & 1u], nwaves, wave, before, total);
        const uint32_t pos = pick4(cls, base[0] + before[0], base[1] + before[1], base[2] + before[2], base[3] + before[3]) +
                             rank_in_wave(b, cls);
        scatter(out_ids, out_levels, s, live, i, cls, pos);
#pragma unroll
        for (uint32_t l = 0; l < kLods; ++l) base[l] += total[l];
    }
    if (tid < kLods) out_counts[tid] = tid < h.n_lods ? pick4(tid, base[0], base[1], base[2], base[3]) : 0u;
}

// ---- form 2: count, then scatter ------------------------------------------------------------------------------------------------
template <bool DEV>
__global__ __launch_bounds__(kCullMaxChunk) void cull_count_kernel(const float *__restrict__ bounds, const mmdx_cull_view *__restrict__ view_dev,
                                                                   const mmdx_cull_view view_arg, uint32_t *__restrict__ chunk_counts,
                                                                   const CullScalars s) {
    __shared__ uint32_t counts[kMaxWaves][kLods];
    const mmdx_cull_view &v = DEV ? *view_dev : view_arg;
    const ViewHead h = view_head(v);
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, nwaves = s.chunk >> 6;
    const uint64_t i = uint64_t(blockIdx.x) * s.chunk + tid;
    const bool live = i < s.ni;
    const uint32_t cls = live ? classify(v, h, bounds, i) : MMDX_CULLED;
    const Ballots b = ballots_of(live, cls);
    publish_counts(b, lane, counts[wave]);
    __syncthreads();
    if (tid < kLods) {
        uint32_t sum = 0;
        for (uint32_t w = 0; w < nwaves; ++w) sum += counts[w][tid];
        chunk_counts[size_t(blockIdx.x) * kLods + tid] = sum;
    }
}

template <bool DEV>
__global__ __launch_bounds__(kCullMaxChunk) void cull_scatter_kernel(const float *__restrict__ bounds, const mmdx_cull_view *__restrict__ view_dev,
                                                                     const mmdx_cull_view view_arg, const uint32_t *__restrict__ chunk_counts,
                                                                     uint32_t *__restrict__ out_ids, uint32_t *__restrict__ out_counts,
                                                                     uint32_t *__restrict__ out_levels, const CullScalars s) {
    __shared__ uint32_t counts[kMaxWaves][kLods];      // this chunk's instances per wave and level
    __shared__ uint32_t earlier[kMaxWaves][kLods];     // each wave's share of the sum over the chunks before this one
    const mmdx_cull_view &v = DEV ? *view_dev : view_arg;
    const ViewHead h = view_head(v);
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, nwaves = s.chunk >> 6, c = blockIdx.x;
    // the chunks before this one, dealt over the lanes; then summed over the wave
    uint4 acc = make_uint4(0, 0, 0, 0);
    const uint4 *cc = reinterpret_cast<const uint4 *>(chunk_counts);
    for (uint32_t j = tid; j < c; j += s.chunk) {
        const uint4 q = cc[j];
        acc.x += q.x; acc.y += q.y; acc.z += q.z; acc.w += q.w;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        acc.x += __shfl_xor(acc.x, d); acc.y += __shfl_xor(acc.y, d); acc.z += __shfl_xor(acc.z, d); acc.w += __shfl_xor(acc.w, d);
    }
    if (lane < kLods) earlier[wave][lane] = pick4(lane, acc.x, acc.y, acc.z, acc.w);
    const uint64_t i = uint64_t(c) * s.chunk + tid;
    const bool live = i < s.ni;
    const uint32_t cls = live ? classify(v, h, bounds, i) : MMDX_CULLED;
    const Ballots b = ballots_of(live, cls);
    publish_counts(b, lane, counts[wave]);
    __syncthreads();
    uint32_t before[kLods], total[kLods], base[kLods] = {0, 0, 0, 0};
    wave_prefix(counts, nwaves, wave, before, total);
    for (uint32_t w = 0; w < nwaves; ++w) {
#pragma unroll
        for (uint32_t l = 0; l < kLods; ++l) base[l] += earlier[w][l];
    }
    const uint32_t pos = pick4(cls, base[0] + before[0], base[1] + before[1], base[2] + before[2], base[3] + before[3]) + rank_in_wave(b, cls);
    scatter(out_ids, out_levels, s, live, i, cls, pos);
    if (c + 1 == s.nchunks && tid < kLods)
        out_counts[tid] = tid < h.n_lods ? pick4(tid, base[0] + total[0], base[1] + total[1], base[2] + total[2], base[3] + total[3]) : 0u;
}

}  // namespace

hipError_t launch_cull(const CullLaunch &c, const CullShape &shape, hipStream_t stream) {
    const CullScalars s{c.ni, c.list_stride, shape.chunk, shape.nchunks};
    const bool dev = c.view_dev != nullptr;
    static const mmdx_cull_view no_view{};
    const mmdx_cull_view &arg = dev ? no_view : *c.view_host;
    const dim3 block(shape.threads);
    if (shape.form == 1) {
        hipLaunchKernelGGL(dev ? cull_walk_kernel<true> : cull_walk_kernel<false>, dim3(1), block, 0, stream, c.bounds, c.view_dev, arg,
                           c.out_ids, c.out_counts, c.out_levels, s);
        return hipGetLastError();
    }
    hipLaunchKernelGGL(dev ? cull_count_kernel<true> : cull_count_kernel<false>, dim3(shape.nchunks), block, 0, stream, c.bounds, c.view_dev,
                       arg, c.scratch, s);
    if (hipError_t e = hipGetLastError()) return e;
    hipLaunchKernelGGL(dev ? cull_scatter_kernel<true> : cull_scatter_kernel<false>, dim3(shape.nchunks), block, 0, stream, c.bounds,
                       c.view_dev, arg, static_cast<const uint32_t *>(c.scratch), c.out_ids, c.out_counts, c.out_levels, s);
    return hipGetLastError();
}

}  // namespace mmdx

// events_kernels.hip -- mmdx_animator_events on gfx950 (include/mmdx.h states the arithmetic; events_math.hpp holds it, shared with
// the CPU driver of the tests; this file is built with -ffp-contract=off like the rest).
//
// the masks     animator_events_kernel, one lane per instance.  The seven state arrays the call reads are loaded coalesced, 36 bytes
//               per instance (a wave: 256 or 512 contiguous bytes of each); nothing of the animator is written.  dt arrives as in
//               animator_advance_kernel: a kernel argument or one double in device memory (a wave-uniform address).  The clip table
//               and the marker table are gathered through the lane's clip ids -- a crowd plays a handful of clips, so they stay in
//               the caches -- and the clip's markers are scanned, not searched (events_math.hpp says why).  out_fired is stored
//               coalesced.  A NaN step needs no path of its own: every mask is 0.
// the lists     no atomic decides an order (the pattern of cull_kernels.hip).  The same launch writes per-chunk, per-list counts to
//               the set's scratch: one ballot per list, __popcll, the waves' counts in LDS.  events_scatter_kernel follows: the
//               workgroup of chunk c sums the counts of chunks [0, c) -- every wave for itself, so nothing but the wave counts goes
//               through LDS --, reads out_fired (and levels) of its chunk back, applies events_in_list again (same words, same
//               answer), ranks each lane with mbcnt of its list's ballot plus the waves before it, and scatters; the last chunk's
//               workgroup writes out_counts.  No workgroup ever waits for another one: the only ordering between workgroups is the
//               kernel boundary.
#include <hip/hip_runtime.h>

#include "events_kernels.hpp"

namespace mmdx {

namespace {

constexpr uint32_t kMaxWaves = kEventsMaxChunk / 64;
constexpr uint32_t kLists = kEventsMaxLists;
static_assert(kLists == 4, "the counts of a chunk travel as one uint4");

struct ListArgs {
    uint32_t mask[kLists];
    uint32_t list_stride, nchunks;
};

// The wave's ballots: which lanes hold an instance of each list
struct Ballots {
    unsigned long long m[kLists];
};
__device__ __forceinline__ Ballots ballots_of(bool live, uint32_t fired, const ListArgs &l, bool has_levels, uint32_t level) {
    Ballots b;
#pragma unroll
    for (uint32_t k = 0; k < kLists; ++k) b.m[k] = __ballot(live && events_in_list(fired, l.mask[k], has_levels, level));
    return b;
}
// lanes 0..3 of every wave publish the wave's count of their list
__device__ __forceinline__ void publish_counts(const Ballots &b, uint32_t lane, uint32_t *wave_counts /* [kLists] of this wave */) {
    if (lane < kLists) {
        const unsigned long long mine = lane == 0 ? b.m[0] : (lane == 1 ? b.m[1] : (lane == 2 ? b.m[2] : b.m[3]));
        wave_counts[lane] = uint32_t(__popcll(mine));
    }
}
__device__ __forceinline__ uint32_t rank_in_wave(unsigned long long ballot) {
    return __builtin_amdgcn_mbcnt_hi(uint32_t(ballot >> 32), __builtin_amdgcn_mbcnt_lo(uint32_t(ballot), 0u));
}

template <bool LISTS>
__global__ __launch_bounds__(kEventsMaxChunk) void animator_events_kernel(const EventsLaunch e, const ListArgs l, double dt,
                                                                           const double *__restrict__ dt_dev) {
    if (dt_dev) dt = *dt_dev;
    const uint32_t tid = threadIdx.x, chunk = blockDim.x;
    const uint64_t i = uint64_t(blockIdx.x) * chunk + tid;
    const bool live = i < e.ni;
    uint32_t fired = 0u;
    if (live) {
        fired = events_fired(e.clips, e.markers, e.clips_a[i], e.clips_b[i], e.times_a[i], e.times_b[i], e.weights[i], e.speed[i],
                             e.fade_rate[i], dt, e.dominant);
        e.out_fired[i] = fired;
    }
    if (LISTS) {
        __shared__ uint32_t counts[kMaxWaves][kLists];
        const uint32_t lane = tid & 63u, wave = tid >> 6, nwaves = chunk >> 6;
        const bool has_levels = e.levels != nullptr;
        const uint32_t level = (live && has_levels) ? e.levels[i] : 0u;
        const Ballots b = ballots_of(live, fired, l, has_levels, level);
        publish_counts(b, lane, counts[wave]);
        __syncthreads();
        if (tid < kLists) {
            uint32_t sum = 0;
            for (uint32_t w = 0; w < nwaves; ++w) sum += counts[w][tid];
            e.chunk_counts[size_t(blockIdx.x) * kLists + tid] = sum;
        }
    }
}

__global__ __launch_bounds__(kEventsMaxChunk) void events_scatter_kernel(const uint32_t *__restrict__ fired_in, const uint32_t *__restrict__ levels,
                                                                          const uint32_t *__restrict__ chunk_counts, uint32_t *__restrict__ out_ids,
                                                                          uint32_t *__restrict__ out_counts, uint32_t ni, const ListArgs l) {
    __shared__ uint32_t counts[kMaxWaves][kLists];      // this chunk's instances per wave and list
    const uint32_t tid = threadIdx.x, chunk = blockDim.x, lane = tid & 63u, wave = tid >> 6, nwaves = chunk >> 6, c = blockIdx.x;
    // the chunks before this one, dealt over the lanes of every wave, then summed over the wave: each wave holds the whole sum
    uint4 base = make_uint4(0, 0, 0, 0);
    const uint4 *cc = reinterpret_cast<const uint4 *>(chunk_counts);
    for (uint32_t j = lane; j < c; j += 64u) {
        const uint4 q = cc[j];
        base.x += q.x; base.y += q.y; base.z += q.z; base.w += q.w;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        base.x += __shfl_xor(base.x, d); base.y += __shfl_xor(base.y, d); base.z += __shfl_xor(base.z, d); base.w += __shfl_xor(base.w, d);
    }
    const uint64_t i = uint64_t(c) * chunk + tid;
    const bool live = i < ni;
    const bool has_levels = levels != nullptr;
    const uint32_t fired = live ? fired_in[i] : 0u;
    const uint32_t level = (live && has_levels) ? levels[i] : 0u;
    const Ballots b = ballots_of(live, fired, l, has_levels, level);
    publish_counts(b, lane, counts[wave]);
    __syncthreads();
    const uint32_t start[kLists] = {base.x, base.y, base.z, base.w};
    uint32_t total[kLists];
#pragma unroll
    for (uint32_t k = 0; k < kLists; ++k) {
        uint32_t before = 0, all = 0;
        for (uint32_t w = 0; w < nwaves; ++w) {
            const uint32_t n = counts[w][k];
            all += n;
            before += w < wave ? n : 0u;
        }
        total[k] = start[k] + all;
        // (a position at or behind list_stride cannot happen while out_fired and levels hold still between the two launches; the
        // test keeps a caller's race from becoming a store outside the lists)
        const uint32_t pos = start[k] + before + rank_in_wave(b.m[k]);
        if (((b.m[k] >> lane) & 1ull) && pos < l.list_stride) out_ids[size_t(k) * l.list_stride + pos] = uint32_t(i);
    }
    if (c + 1 == l.nchunks && tid < kLists)
        out_counts[tid] = tid == 0 ? total[0] : (tid == 1 ? total[1] : (tid == 2 ? total[2] : total[3]));
}

}  // namespace

hipError_t launch_animator_events(const EventsLaunch &e, uint32_t chunk, double dt, const double *dt_dev, hipStream_t stream) {
    if (!e.ni) return hipSuccess;
    const uint32_t nchunks = (e.ni + chunk - 1) / chunk;
    ListArgs l{{0, 0, 0, 0}, e.list_stride, nchunks};
    for (uint32_t k = 0; k < e.n_lists && k < kLists; ++k) l.mask[k] = e.list_mask[k];
    const dim3 grid(nchunks), block(chunk);
    if (!e.n_lists) {
        hipLaunchKernelGGL(animator_events_kernel<false>, grid, block, 0, stream, e, l, dt, dt_dev);
        return hipGetLastError();
    }
    hipLaunchKernelGGL(animator_events_kernel<true>, grid, block, 0, stream, e, l, dt, dt_dev);
    if (hipError_t err = hipGetLastError()) return err;
    hipLaunchKernelGGL(events_scatter_kernel, grid, block, 0, stream, static_cast<const uint32_t *>(e.out_fired), e.levels,
                       static_cast<const uint32_t *>(e.chunk_counts), e.out_ids, e.out_counts, e.ni, l);
    return hipGetLastError();
}

}  // namespace mmdx

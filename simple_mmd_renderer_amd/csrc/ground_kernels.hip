// ground_kernels.hip -- mmdx_ground_place and mmdx_ground_targets on gfx950 (include/mmdx.h states the arithmetic; ground_math.hpp
// holds it, shared with the CPU driver of the tests; this file is built with -ffp-contract=off like the rest, and models created
// with MMDX_CREATE_FAST_MATH run these same kernels).
//
// one lane per instance   (select form: per list position.)  A workgroup is one wave of 64 instances; the field's description is a
//                         kernel argument, so cell and fraction are computed from scalar registers.
// place                   a lane reads its placement's x and z (and its drop), gathers the four corners of its cell (4-byte loads,
//                         two per row of the field) and stores one float, placements[i][1].  A failed sample or drop stores nothing.
// targets                 a lane loops over the feet: three 4-byte loads of the point (strided: a sockets slab has a point every 64
//                         bytes), the four-corner gather, one 16-byte store into slab f.  The least hf - h0 lives in the lane's
//                         registers across the loop: no cross-lane reduction, no atomics, the same bits on every run.
// Neither output overlaps an input (ground_table.hpp refuses that), hence __restrict__; placements of the place call are read and
// written by the same lane only.  No LDS, no scratch, vector stores only.
#include <hip/hip_runtime.h>

#include "ground_kernels.hpp"

namespace mmdx {

namespace {

// the instance of this lane; false: nothing to do (behind the end or the count, or an id that is no instance)
template <bool kSelect>
__device__ __forceinline__ bool ground_lane(const InstanceList &list, uint32_t cells, uint32_t ni, uint32_t &i) {
    const uint32_t k = blockIdx.x * kGroundThreads + threadIdx.x;          // < 2^23 + 64
    if (kSelect) {
        const ListedInstances li{list};
        const Lane ln = li.lane(k, li.used(cells));
        i = ln.row;
        return ln.live;
    }
    i = k;
    return k < ni;
}

template <bool kSelect>
__global__ __launch_bounds__(kGroundThreads) void ground_place_kernel(const GroundPlaceLaunch p, const InstanceList list, uint32_t cells) {
    uint32_t i;
    if (!ground_lane<kSelect>(list, cells, p.ni, i)) return;
    const float *__restrict__ H = p.heights;
    ground_place_instance(p.g, H, p.placements + size_t(i) * kGroundPoseFloats, p.drop ? p.drop + i : nullptr, p.y_offset);
}

template <bool kSelect>
__global__ __launch_bounds__(kGroundThreads) void ground_targets_kernel(const GroundTargetsLaunch p, const InstanceList list, uint32_t cells) {
    uint32_t i;
    if (!ground_lane<kSelect>(list, cells, p.ni, i)) return;
    const float *__restrict__ H = p.heights;
    const float *__restrict__ pl = p.placements + size_t(i) * kGroundPoseFloats;
    const float *__restrict__ pts = p.points + size_t(i) * p.point_stride;
    float *__restrict__ out = p.out_targets + size_t(i) * 4;
    float *__restrict__ drop = p.out_drop ? p.out_drop + i : nullptr;
    ground_targets_instance(p.g, H, pl, pts, p.slab_stride, p.n_feet, p.max_step, p.max_drop, out, size_t(p.ni) * 4, drop);
}

}  // namespace

hipError_t launch_ground_place(const GroundPlaceLaunch &p, const GroundShape &shape, const InstanceList *list, uint32_t cells,
                               hipStream_t stream) {
    const uint32_t n = list ? cells : p.ni;
    if (!n) return hipSuccess;
    const dim3 grid(shape.nblocks), block(shape.threads);
    if (list)
        hipLaunchKernelGGL(ground_place_kernel<true>, grid, block, 0, stream, p, *list, cells);
    else
        hipLaunchKernelGGL(ground_place_kernel<false>, grid, block, 0, stream, p, InstanceList{nullptr, nullptr, p.ni}, n);
    return hipGetLastError();
}

hipError_t launch_ground_targets(const GroundTargetsLaunch &p, const GroundShape &shape, const InstanceList *list, uint32_t cells,
                                 hipStream_t stream) {
    const uint32_t n = list ? cells : p.ni;
    if (!n) return hipSuccess;
    const dim3 grid(shape.nblocks), block(shape.threads);
    if (list)
        hipLaunchKernelGGL(ground_targets_kernel<true>, grid, block, 0, stream, p, *list, cells);
    else
        hipLaunchKernelGGL(ground_targets_kernel<false>, grid, block, 0, stream, p, InstanceList{nullptr, nullptr, p.ni}, n);
    return hipGetLastError();
}

}  // namespace mmdx

// row_blend_kernels.hip -- mmdx_pose_blend / mmdx_rate_blend on gfx950: per (instance, item) the blend of two evaluated rows at the
// effective weight weights[i] * mask[item] (include/mmdx.h states the contract).  The arithmetic is blend_side / blend_pose /
// blend_rate of motion_blend.hpp, called and not restated; this file is built with -ffp-contract=off like the rest, and models
// created with MMDX_CREATE_FAST_MATH run these same kernels.
//
// one lane per item          poses: a lane loads its 32-byte pose of A (two 16-byte loads), of B only where its side needs B, and
//                            stores 32 bytes; a wave's traffic is 2 KB contiguous per array.  rates: one float per lane.  A lane
//                            touches no item but its own and reads it before it stores, which is what makes out == a and out == b
//                            safe; a, b and out are therefore NOT __restrict__.
// the row is wave-uniform    blockIdx.x = instance (select form: list position, through ListedInstances), blockIdx.y = a chunk of the
//                            row, so a workgroup never spans two instances.  The list entry, the weight and the mask id depend on
//                            blockIdx.x alone and are read once (weights, mask_ids and masks never overlap out: scalar loads).
// rows that hold their result  a lane whose item of `out` is already the result (side A with out == a, side B with out == b) neither
//                            loads nor stores it, and with out == a a workgroup whose weight is 0 or NaN returns before any other
//                            load: the effective weight is then 0 or NaN whatever the mask holds.  No LDS.
#include <hip/hip_runtime.h>

#include "motion_blend.hpp"
#include "row_blend_kernels.hpp"

namespace mmdx {

namespace {

// the row a workgroup works on: false = none (a dead list position, or an in-place row that already holds its result)
template <bool kSelect>
__device__ __forceinline__ bool blend_row(const InstanceList &list, const float *__restrict__ weights, bool in_place_a, uint32_t &i,
                                          float &w) {
    i = blockIdx.x;
    if (kSelect) {
        const ListedInstances li{list};
        const Lane ln = li.lane(blockIdx.x, li.used(gridDim.x));
        if (!ln.live) return false;
        i = ln.row;
    }
    w = weights[i];
    return !(in_place_a && (w == 0.0f || w != w));
}

// the effective weight of item j of instance i: one binary32 multiply (by 1.0f without a mask: exactly w)
__device__ __forceinline__ float effective_weight(float w, const uint32_t *__restrict__ mask_ids, const float *__restrict__ masks,
                                                  uint32_t n_masks, uint32_t items, uint32_t i, uint32_t j) {
    const uint32_t m = mask_ids ? mask_ids[i] : kMaskNone;
    float mv = 1.0f;
    if (m != kMaskNone) mv = m < n_masks ? masks[size_t(m) * items + j] : 0.0f;
    return w * mv;
}

template <bool kSelect>
__global__ __launch_bounds__(kRowBlendThreads) void pose_blend_kernel(const float4 *a, const float4 *b, float4 *out,
                                                                      const float *__restrict__ weights,
                                                                      const uint32_t *__restrict__ mask_ids,
                                                                      const float *__restrict__ masks, uint32_t items,
                                                                      uint32_t n_masks, const InstanceList list) {
    uint32_t i;
    float w;
    if (!blend_row<kSelect>(list, weights, out == a, i, w)) return;
    const uint32_t j = blockIdx.y * blockDim.x + threadIdx.x;      // < 65535 * 256: no overflow
    if (j >= items) return;
    const float e = effective_weight(w, mask_ids, masks, n_masks, items, i, j);
    const uint32_t side = blend_side(e);
    if ((side == kBlendA && out == a) || (side == kBlendB && out == b)) return;
    const size_t at = (size_t(i) * items + j) * 2;
    const float4 *src = side == kBlendB ? b : a;
    float4 t = src[at], q = src[at + 1];
    if (side == kBlendMix) blend_pose(t, q, b[at], b[at + 1], e);
    out[at] = t;
    out[at + 1] = q;
}

template <bool kSelect>
__global__ __launch_bounds__(kRowBlendThreads) void rate_blend_kernel(const float *a, const float *b, float *out,
                                                                      const float *__restrict__ weights,
                                                                      const uint32_t *__restrict__ mask_ids,
                                                                      const float *__restrict__ masks, uint32_t items,
                                                                      uint32_t n_masks, const InstanceList list) {
    uint32_t i;
    float w;
    if (!blend_row<kSelect>(list, weights, out == a, i, w)) return;
    const uint32_t j = blockIdx.y * blockDim.x + threadIdx.x;
    if (j >= items) return;
    const float e = effective_weight(w, mask_ids, masks, n_masks, items, i, j);
    const uint32_t side = blend_side(e);
    if ((side == kBlendA && out == a) || (side == kBlendB && out == b)) return;
    const size_t at = size_t(i) * items + j;
    float r = side == kBlendB ? b[at] : a[at];
    if (side == kBlendMix) r = blend_rate(r, b[at], e);
    out[at] = r;
}

}  // namespace

hipError_t launch_pose_blend(const RowBlendLaunch &p, const InstanceList *list, uint32_t cells, hipStream_t stream) {
    const dim3 grid(list ? cells : p.ni, row_blend_chunks(p.items)), block(row_blend_threads(p.items));
    const float4 *a = reinterpret_cast<const float4 *>(p.a), *b = reinterpret_cast<const float4 *>(p.b);
    float4 *out = reinterpret_cast<float4 *>(p.out);
    if (list)
        hipLaunchKernelGGL(pose_blend_kernel<true>, grid, block, 0, stream, a, b, out, p.weights, p.mask_ids, p.masks, p.items,
                           p.n_masks, *list);
    else
        hipLaunchKernelGGL(pose_blend_kernel<false>, grid, block, 0, stream, a, b, out, p.weights, p.mask_ids, p.masks, p.items,
                           p.n_masks, InstanceList{nullptr, nullptr, p.ni});
    return hipGetLastError();
}

hipError_t launch_rate_blend(const RowBlendLaunch &p, const InstanceList *list, uint32_t cells, hipStream_t stream) {
    const dim3 grid(list ? cells : p.ni, row_blend_chunks(p.items)), block(row_blend_threads(p.items));
    if (list)
        hipLaunchKernelGGL(rate_blend_kernel<true>, grid, block, 0, stream, p.a, p.b, p.out, p.weights, p.mask_ids, p.masks, p.items,
                           p.n_masks, *list);
    else
        hipLaunchKernelGGL(rate_blend_kernel<false>, grid, block, 0, stream, p.a, p.b, p.out, p.weights, p.mask_ids, p.masks, p.items,
                           p.n_masks, InstanceList{nullptr, nullptr, p.ni});
    return hipGetLastError();
}

}  // namespace mmdx

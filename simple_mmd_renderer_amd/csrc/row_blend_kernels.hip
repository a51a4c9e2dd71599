// row_blend_kernels.hip -- mmdx_pose_blend / mmdx_rate_blend (and mmdx_rate_add, at the end) on gfx950: per (instance, item) the blend of two evaluated rows at the
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

// mmdx_rate_add: out = a + d * e with d = b, or b - refs[r] under a reference; the shape, the early returns and the in-place rule are
// those above.  An item whose effective weight fails e >= 1e-7f, and every item of a row whose reference id is neither below n_refs
// nor kRefNone, is A's: neither b nor refs is read for it.
template <bool kSelect>
__global__ __launch_bounds__(kRowBlendThreads) void rate_add_kernel(const float *a, const float *b, float *out,
                                                                    const float *__restrict__ weights,
                                                                    const uint32_t *__restrict__ mask_ids,
                                                                    const float *__restrict__ masks,
                                                                    const uint32_t *__restrict__ ref_ids,
                                                                    const float *__restrict__ refs, uint32_t items, uint32_t n_masks,
                                                                    uint32_t n_refs, const InstanceList list) {
    uint32_t i;
    float w;
    if (!blend_row<kSelect>(list, weights, out == a, i, w)) return;
    const uint32_t r = ref_ids ? ref_ids[i] : kRefNone;
    const bool row_is_a = r != kRefNone && r >= n_refs;
    if (row_is_a && out == a) return;
    const uint32_t j = blockIdx.y * blockDim.x + threadIdx.x;
    if (j >= items) return;
    const float e = effective_weight(w, mask_ids, masks, n_masks, items, i, j);
    const bool mix = !row_is_a && e >= 1e-7f;
    if (!mix && out == a) return;
    const size_t at = size_t(i) * items + j;
    float v = a[at];
    if (mix) {
        float d = b[at];
        if (r != kRefNone) d = d - refs[size_t(r) * items + j];
        v = v + d * e;
    }
    out[at] = v;
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

hipError_t launch_rate_add(const RowAddLaunch &p, const InstanceList *list, uint32_t cells, hipStream_t stream) {
    const RowBlendLaunch &q = p.rows;
    const dim3 grid(list ? cells : q.ni, row_blend_chunks(q.items)), block(row_blend_threads(q.items));
    if (list)
        hipLaunchKernelGGL(rate_add_kernel<true>, grid, block, 0, stream, q.a, q.b, q.out, q.weights, q.mask_ids, q.masks, p.ref_ids,
                           p.refs, q.items, q.n_masks, p.n_refs, *list);
    else
        hipLaunchKernelGGL(rate_add_kernel<false>, grid, block, 0, stream, q.a, q.b, q.out, q.weights, q.mask_ids, q.masks, p.ref_ids,
                           p.refs, q.items, q.n_masks, p.n_refs, InstanceList{nullptr, nullptr, q.ni});
    return hipGetLastError();
}

}  // namespace mmdx

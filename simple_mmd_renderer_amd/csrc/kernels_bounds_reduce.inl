// kernels_bounds_reduce.inl -- the kernels that fold the partial bounds of deform_kernel<..., BOUNDS> (kernels_bounds.inl) into
// out[i][6].  A piece of kernels.hip (included inside namespace mmdx { namespace {), in the bit-exact build only.

// ---- per-instance bounds from the partials of deform_kernel<..., BOUNDS>: one wave per instance, out[i][6] -----------------------
// (min / max only: the same kernel serves fast-math models)  The workgroup's wave reduces the partials of cell ln.cell into row ln.row.
__device__ __forceinline__ void bounds_reduce_body(const float *part, float *out, uint32_t units, const Lane ln) {
    const uint32_t lane = threadIdx.x;
    const float *src = part + size_t(ln.cell) * units * 6;
    float mn[3], mx[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) mn[c] = mx[c] = __builtin_nanf("");
    for (uint32_t u = lane; u < units; u += 64) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            mn[c] = bound_op<false>(mn[c], src[size_t(u) * 6 + c]);
            mx[c] = bound_op<true>(mx[c], src[size_t(u) * 6 + 3 + c]);
        }
    }
    const float v = wave_bounds6(mn, mx, lane);
    if (lane < 6) out[size_t(ln.row) * 6 + lane] = v;
}

__global__ __launch_bounds__(64) void bounds_reduce_kernel(const float *part, float *out, uint32_t units) {
    bounds_reduce_body(part, out, units, {blockIdx.x, blockIdx.x, true});
}

// The same behind a select launch: partials by list position, block j writes row ids[j] -- live positions with an id inside the
// call's arrays only, every other row of `out` keeps what it held.
__global__ __launch_bounds__(64) void bounds_reduce_select_kernel(const float *part, float *out, uint32_t units, uint32_t ni,
                                                                  const uint32_t *ids, const uint32_t *count, uint32_t n_ids) {
    const ListedInstances sel = {{ids, count, ni}};
    const Lane ln = sel.lane(blockIdx.x, sel.used(n_ids));
    if (ln.live) bounds_reduce_body(part, out, units, ln);
}

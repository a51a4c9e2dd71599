// kernels_bench.inl -- the streaming copy, fill and store-pattern kernels behind the ceilings bench.py prints.
// A piece of kernels.hip (included inside namespace mmdx { namespace {), in the bit-exact build only.

// ---- streaming copy / fill: the practical HBM ceiling printed next to the roofline ---------------
// Every workgroup owns one contiguous 4 KiB chunk, workgroups in address order: the shape that
// reached the highest store rate on MI355X in tools/archive/probes/bw_probe (a few-thousand-block grid-stride loop
// is 30 % slower).
__global__ __launch_bounds__(kThreads) void copy_kernel(float4 *dst, const float4 *src, size_t n) {
    const size_t i = size_t(blockIdx.x) * kThreads + threadIdx.x;
    if (i < n) dst[i] = src[i];
}
__global__ __launch_bounds__(kThreads) void fill_kernel(float4 *dst, size_t n) {
    const size_t i = size_t(blockIdx.x) * kThreads + threadIdx.x;
    if (i < n) dst[i] = make_float4(1.f, 2.f, 3.f, 4.f);
}

// Store-only replay of the deform kernel's output pattern: workgroup = (512-vertex tile, group of 16
// instances) writing one piece (6 KiB for SoA) into each output array per instance.  Its rate is BIMODAL
// on MI355X: for some placements of the arrays it runs at the linear-fill rate, for others ~25 % below,
// and the deform kernel follows it (tools/archive/probes/alloc_kernel_probe.py).  Used as the ceiling bench.py prints
// and as the probe of mmdx_crowd_output_alloc().
__global__ __launch_bounds__(kThreads) void pattern_fill_kernel(float4 *a, float4 *b, uint32_t nv,
                                                                uint32_t ni, uint32_t ntiles, uint32_t bpva,
                                                                uint32_t bpvb, uint32_t pitch) {
    const uint32_t tile = blockIdx.x % ntiles, grp = blockIdx.x / ntiles;
    const uint32_t v0 = tile * kTileVerts, nvt = min(kTileVerts, nv - v0);
    // callers keep pitch * bytes-per-vertex % 16 == 0; the 16-byte pieces of a ragged last tile are rounded down (never past
    // the instance's NV vertices)
    const uint32_t pa = nvt * bpva / 16, pb = nvt * bpvb / 16;
    const float4 v = make_float4(1.f, 2.f, 3.f, 4.f);
    for (uint32_t g = grp * 16; g < min(ni, grp * 16 + 16); ++g) {
        const size_t base_a = (size_t(g) * pitch + v0) * bpva / 16, base_b = (size_t(g) * pitch + v0) * bpvb / 16;
        for (uint32_t q = threadIdx.x; q < pa + pb; q += kThreads) {
            store16(q < pa ? a + base_a + q : b + base_b + (q - pa), v);      // the deform kernel's store instruction (nt)
        }
    }
}

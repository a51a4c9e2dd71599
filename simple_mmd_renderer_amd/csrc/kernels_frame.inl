// kernels_frame.inl -- frame_kernel: one frame of one model, laid out for latency.
// A piece of kernels.hip (included inside namespace mmdx { namespace {), compiled with it, plain and fast-math.

// ---- ONE frame of ONE model (ni == 1): the reference's per-frame call (main.cpp:1821) -------------------------------------
// A single frame is a few megabytes: its run time is the latency chain of a workgroup, not bandwidth.  So, unlike the crowd
// kernel: a workgroup is a PART of a tile (THREADS sorted slots, one per lane: config 2's 98 tiles become 392 workgroups of two
// waves, on every CU), requests are issued in latency order (setup_fused1), and every lane stores its own vertex straight from
// registers to its original index -- no LDS image, no second barrier; the scattered 12-byte stores of 1.2 MB merge in L2.
// Same arithmetic, same order.
template <int THREADS, int LAYOUT, int MORPH, bool F16>
__global__ __launch_bounds__(THREADS) void frame_kernel(const DeformParams p) {
    constexpr uint32_t kParts = kTileVerts / THREADS;
    constexpr uint32_t BH = F16 ? 16u : 8u;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x;
    const uint32_t tile = blockIdx.x / kParts, part = blockIdx.x - tile * kParts;
    const TileHdr &th = p.tiles[tile];
    if (part * THREADS >= th.nv) return;                       // the whole workgroup: nothing of this tile left for it
    float4 *pal = reinterpret_cast<float4 *>(smem);
    float *wl = reinterpret_cast<float *>(smem + p.w_off);
    Slot sl[1];
    RowHead<F16, BH> hd[1];
    setup_fused1<THREADS, LAYOUT, MORPH, F16, 1, BH>(p, th, pal, wl, 0u, 1u, 1u, tid, part * THREADS, sl, hd);
    __syncthreads();
    const Slot &q = sl[0];
    if (!q.act) return;
    v2f cxy = q.pxy;
    float cz = q.pz;
    if constexpr (MORPH == kMorphFused1) {
        // vertex_image = 0; for each applied entry: image = image + offset*rate (poser_impl.inl:340-346); coordinate = base + image
        v2f dxy = v2f{0.f, 0.f};
        float dz = 0.f;
        row_consume<F16, BH>(p.entries, q.rb, q.rlen, hd[0], [&](float ox, float oy, float oz, uint32_t slot) {
            const float w = wl[slot];
            if (!(w < kMorphEps)) { dxy = dxy + v2f{ox, oy} * w; dz = dz + oz * w; }
        });
        cxy = q.pxy + dxy; cz = q.pz + dz;
        if (p.morphed) {   // kept (sorted order) for later calls that declare the rates unchanged
            float *mo = p.morphed + (size_t(th.v0) + part * THREADS + uint32_t(tid)) * 3;
            mo[0] = cxy.x; mo[1] = cxy.y; mo[2] = cz;
        }
    }
    const M12 m = skin_matrix(q, pal);
    v2f oxy, rxy;
    float oz, rz;
    xform_pos(m, cxy, cz, oxy, oz);
    xform_nrm(m, q.nxy, q.nz, rxy, rz);
    oxy = oxy * p.pos_scale;                                   // a separate multiply after the transform (main.cpp:848-850)
    oz = oz * p.pos_scale;
    // original vertex index -- or, for MMDX_CREATE_TILE_ORDER models, the vertex's sorted slot
    const size_t v = size_t(th.v0) + (p.tile_order ? part * THREADS + uint32_t(tid) : q.perm);
    if constexpr (LAYOUT == MMDX_OUT_SOA) {
        float *A = reinterpret_cast<float *>(p.out_a) + v * 3, *B = reinterpret_cast<float *>(p.out_b) + v * 3;
        A[0] = oxy.x; A[1] = oxy.y; A[2] = oz;
        B[0] = rxy.x; B[1] = rxy.y; B[2] = rz;
    } else if constexpr (LAYOUT == MMDX_OUT_VERTEX32) {
        float *A = reinterpret_cast<float *>(p.out_a) + v * 8;
        if (p.out_aligned) {
            reinterpret_cast<float4 *>(A)[0] = make_float4(oxy.x, oxy.y, oz, rxy.x);
            reinterpret_cast<float4 *>(A)[1] = make_float4(rxy.y, rz, q.uv.x, q.uv.y);
        } else {
            A[0] = oxy.x; A[1] = oxy.y; A[2] = oz; A[3] = rxy.x; A[4] = rxy.y; A[5] = rz; A[6] = q.uv.x; A[7] = q.uv.y;
        }
    } else {
        unsigned short *A = reinterpret_cast<unsigned short *>(p.out_a) + v * 3;
        float *B = reinterpret_cast<float *>(p.out_b) + v * 3;
        A[0] = f2h(oxy.x); A[1] = f2h(oxy.y); A[2] = f2h(oz);
        B[0] = rxy.x; B[1] = rxy.y; B[2] = rz;
    }
}

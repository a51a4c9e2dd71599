// kernels_pack.inl -- pack_kernel, the second shape of the per-instance-morph mode (opt-in: MMDX_FUSED_PACK=1), with its
// launcher, the PK_* timing diagnostics included.
// A piece of kernels.hip (included inside namespace mmdx { namespace {), compiled with it, plain and fast-math.

// ---- per-instance morph weights, second shape (round 4): packs of 4 instances, walk and skinning in SEPARATE phases -------------
// deform_kernel<512, ., kMorphFused4> holds, at the same time, the walk's accumulators for 8 instances, the entries in flight, the
// vertex's skin data and the blend's matrices: 126 VGPRs, two 8-wave workgroups per CU, and its counters say it waits (VALU issue
// 59 %, LDS 50 % of the cycles, waves parked 53 % of their life: profiles/r03/fused_gather_pmc.csv).  This kernel is laid out from
// the register budget down -- 80 VGPRs, three workgroups per CU, six waves per SIMD:
//   * a PACK is 4 instances (one float4 of slot weights per table entry): 12 accumulator registers;
//   * WALK phase: the row is consumed through a rolling window of 4 entries in flight (no second register set, no copies);
//     at its end `coordinate = base + image` (poser_impl.inl:407) of instances 1..3 goes to LDS (`mp`, component-major: every
//     access is lane-consecutive), instance 0's stays in registers -- the accumulators are dead before the first matrix is read;
//   * SKIN phase, per instance: the vertex's coordinate comes back from LDS (the thread's own words: no barrier), blend + transform
//     as in deform_kernel, results scattered to the output images, ONE barrier, coalesced 16-byte copy-out.  The position image of
//     instance j is the `mp` region of instance j (its coordinates were read before the previous instance's barrier: everybody is
//     done with them), the normal image is double buffered -- 48.6 KB of LDS for 8 instances of the 50k model.
// Same operations in the same order as the reference (and as deform_kernel): bit-identical results.
constexpr int kPkThreads = 512;
constexpr int kPkWaves = 6;       // waves per SIMD the register allocation is held to (__launch_bounds__)

// The vertex's static data as the pack kernel keeps it across its loops: 14 registers (load_slot's Slot: 21).
struct PackSlot {
    v2f pxy, nxy;
    float pz, nz;
    float w0, w1, w2, w3;
    uint32_t b01, b23;        // palette entries of the vertex's bones (float4 index inside one instance's palette), two per register
    uint32_t meta;            // perm | deform class << 10 | active << 12
};
__device__ __forceinline__ PackSlot pack_slot(const Slot &q) {
    PackSlot s;
    s.pxy = q.pxy; s.nxy = q.nxy; s.pz = q.pz; s.nz = q.nz;
    s.w0 = q.w0; s.w1 = q.w1; s.w2 = q.w2; s.w3 = q.w3;
    s.b01 = q.b0 | (q.b1 << 16); s.b23 = q.b2 | (q.b3 << 16);
    s.meta = q.perm | (uint32_t(q.cls) << 10) | (q.act ? 1u << 12 : 0u);
    return s;
}
// skin_matrix() from the packed form.  `b01` / `b23` arrive through an opaque copy made inside the instance loop, so that the
// unpacked indices are not hoisted out of it as four loop-invariant registers.
__device__ __forceinline__ M12 skin_matrix_packed(uint32_t cls, uint32_t b01, uint32_t b23, float w0, float w1, float w2, float w3,
                                                  const float4 *P) {
    M12 m;
    if (cls == 0) {
        m = load_m12(P, b01 & 0xffffu);
    } else if (cls == 1) {
        const M12 a = load_m12(P, b01 >> 16), e = load_m12(P, b01 & 0xffffu);      // Lerp(S[b1], S[b0])[w]
        m = blend2(a, e, 1.0f - w0, w0);
        const bool lo = w0 < kLerpLo, hi = w0 > kLerpHi;
        if (__builtin_amdgcn_ballot_w64(lo || hi) != 0) {
            if (lo) m = a;
            else if (hi) m = e;
        }
    } else {
        {
            const M12 a = load_m12(P, b01 & 0xffffu), b = load_m12(P, b01 >> 16);
            m = mul_add(a, w0, b, w1);
        }
        __builtin_amdgcn_sched_barrier(0);
        {
            const M12 c = load_m12(P, b23 & 0xffffu);
            m = add_mul(m, c, w2);
        }
        __builtin_amdgcn_sched_barrier(0);
        {
            const M12 d = load_m12(P, b23 >> 16);
            m = add_mul(m, d, w3);
        }
    }
    return m;
}

template <int LAYOUT, bool F16, bool FIN>
__global__ __launch_bounds__(kPkThreads, kPkWaves) void pack_kernel(const DeformParams p) {
    static_assert(LAYOUT == MMDX_OUT_SOA || LAYOUT == MMDX_OUT_SOA_POS16, "two output arrays");
    static_assert(kTileVerts == 512, "one sorted slot per lane");
    using Raw = typename RawEntry<F16>::type;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x;
    uint32_t tile, grp;
    if (!map_workgroup(p, tile, grp)) return;       // padding workgroup
    const TileHdr &th = p.tiles[tile];
    const uint32_t v0 = th.v0, nvt = th.nv;
    // Instances of this workgroup: p.group / 4 quads.  Blocked: consecutive quads.  Interleaved (default): quad k of the workgroup is
    // quad grp + k * ngroups of the crowd, so that the workgroups running at the same time (neighbouring grp) write neighbouring
    // instances -- chip-wide the stores then sweep a few contiguous megabytes of each output array, as the crowd kernel's do.
    const bool ilv = p.interleave != 0;
    const uint32_t nquads = (p.ni + 3u) >> 2, qstep = ilv ? p.ngroups : 1u;
    const uint32_t quad0 = ilv ? grp : grp * (p.group >> 2);
    const uint32_t npacks = quad0 < nquads ? min(p.group >> 2, (nquads - quad0 + qstep - 1) / qstep) : 0u;
    const uint32_t gcount = npacks * kPkPack;        // group instances incl. the slack of a ragged last quad (never written out)
    auto first_instance = [&](uint32_t g0) { return (quad0 + (g0 >> 2) * qstep) * 4u; };
    stagger_start(p);
    float4 *pal = reinterpret_cast<float4 *>(smem);
    float4 *wq = reinterpret_cast<float4 *>(smem + p.w_off);
    unsigned char *mp = smem + p.mp_off;             // kPkPack regions
    unsigned char *imgB = smem + p.stage_off;        // 2 normal images, BEHIND mp (CopyFast wants image B after image A)
    const uint32_t wstride = p.ns + 1;
    auto pack_weight = [&](uint32_t g0, uint32_t i) {
        return reinterpret_cast<const float4 *>(p.wslot)[size_t(quad0 + (g0 >> 2) * qstep) * wstride + i];
    };
    // the lane's row of the morph table: lane `tid & 63` of the wave's slice (lanes past the tile's last vertex walk their
    // slice's padding: dummy slot, weight 0), padded length wave-uniform -> a scalar.  The row is the same for every pack.
    const uint2 sl2 = p.ell[(v0 + uint32_t(tid)) >> 6];
    const uint32_t rbase = sl2.x + (uint32_t(tid) & 63u);
    const uint32_t rlen = __builtin_amdgcn_readfirstlane(sl2.y);
    const uint32_t last = rlen ? rlen - 1 : 0u;
    Raw e[4];                                        // rolling window over the row: four entries in flight
    auto row_head = [&]() {
        uint32_t rb = rbase;      // (opaque copies like this one keep loop-invariant address arithmetic and operand splats from being
        asm volatile("" : "+v"(rb));   // carried around the loops in registers: they are recomputed where they are used)
#pragma unroll
        for (uint32_t i = 0; i < 4; ++i) e[i] = rlen ? row_entry<F16>(p.entries, rb, min(i, last)) : Raw{};
    };

    // set-up: the group's palettes, the first pack's slot weights, the head of the row, the vertex's static data
    // (one piece after the other: interleaved, their loads in flight would claim more registers than the loops below ever need,
    // and the allocator would answer by spilling the vertex's skin data for the whole kernel)
    stage_palettes<kPkThreads>(p, th, pal, quad0 * 4u, 1u, gcount, tid, qstep);
    __builtin_amdgcn_sched_barrier(0);
    for (uint32_t i = tid; i < wstride; i += kPkThreads) wq[i] = pack_weight(0, i);
    __builtin_amdgcn_sched_barrier(0);
    PackSlot ps;
    {
        Slot q;
        load_slot<LAYOUT, kMorphFused4, F16>(p, th, uint32_t(tid), q);
        ps = pack_slot(q);
    }
    __builtin_amdgcn_sched_barrier(0);
    row_head();
    const bool wreg = wstride <= uint32_t(kPkThreads);
    constexpr uint32_t kAlignVerts = LAYOUT == MMDX_OUT_SOA_POS16 ? 8u : 4u;
    const bool al = p.out_aligned != 0;
    const bool fast = al && nvt == kTileVerts && p.pitch % kAlignVerts == 0 && v0 % kAlignVerts == 0;
    __syncthreads();

#ifdef PK_STAMPS
    // diagnostic build: where a wave's cycles go (s_memtime, one record of 8 counters per wave; never in the product)
    unsigned long long st_acc[6] = {0, 0, 0, 0, 0, 0}, st_t = __builtin_amdgcn_s_memtime();
    const unsigned long long st_begin = st_t;
#define PK_STAMP(k) do { const unsigned long long n_ = __builtin_amdgcn_s_memtime(); st_acc[k] += n_ - st_t; st_t = n_; } while (0)
#else
#define PK_STAMP(k) do { } while (0)
#endif
    uint32_t buf = 0;
    for (uint32_t g0 = 0; g0 < gcount; g0 += kPkPack) {
        PK_STAMP(0);
        // ---- WALK: vertex_image = 0; for each applied entry: image = image + offset*rate (poser_impl.inl:340-346), 4 instances --
        v2f axy[kPkPack], az01 = v2f{0.f, 0.f}, az23 = v2f{0.f, 0.f};
#pragma unroll
        for (uint32_t j = 0; j < kPkPack; ++j) axy[j] = v2f{0.f, 0.f};
        auto apply = [&](const Raw r) {
            float ox, oy, oz;
            uint32_t slot;
            if constexpr (F16) {
                ox = h2f(r.x & 0xffffu); oy = h2f(r.x >> 16); oz = h2f(r.y & 0xffffu); slot = r.y >> 16;
            } else {
                ox = r.x; oy = r.y; oz = r.z; slot = __float_as_uint(r.w);
            }
            const float4 w = wq[slot];
            const v2f oxy = v2f{ox, oy}, ozz = v2f{oz, oz};
            if constexpr (FIN) {
                // a skipped slot weighs +0 exactly and a sum that started at +0 is never -0: with finite offsets
                // "image + offset*0" leaves the image bit for bit unchanged -- no branch
                axy[0] += oxy * w.x; axy[1] += oxy * w.y; axy[2] += oxy * w.z; axy[3] += oxy * w.w;
                az01 += ozz * v2f{w.x, w.y};
                az23 += ozz * v2f{w.z, w.w};
            } else {
                const v2f t0 = axy[0] + oxy * w.x, t1 = axy[1] + oxy * w.y, t2 = axy[2] + oxy * w.z, t3 = axy[3] + oxy * w.w;
                const v2f u01 = az01 + ozz * v2f{w.x, w.y}, u23 = az23 + ozz * v2f{w.z, w.w};
                const bool k0 = w.x < kMorphEps, k1 = w.y < kMorphEps, k2 = w.z < kMorphEps, k3 = w.w < kMorphEps;
                axy[0] = k0 ? axy[0] : t0; axy[1] = k1 ? axy[1] : t1; axy[2] = k2 ? axy[2] : t2; axy[3] = k3 ? axy[3] : t3;
                az01 = v2f{k0 ? az01.x : u01.x, k1 ? az01.y : u01.y};
                az23 = v2f{k2 ? az23.x : u23.x, k3 ? az23.y : u23.y};
            }
        };
#ifdef PK_SKIP_WALK          // timing diagnostic only (wrong results): what the kernel costs without its walk
        if (false) {
#else
        if (rlen) {
#endif
            // Entry j+4 is requested as soon as entry j has been consumed.  The steady-state loop has no branch in its body (a
            // refill past the row's end re-reads the last entry, which is never applied twice): the compiler counts the loads in
            // flight and waits for exactly the oldest one.  The window's first four entries were requested by the set-up / in
            // front of the previous pack's last stores.
            uint32_t rb = rbase;
            asm volatile("" : "+v"(rb));
            uint32_t j = 0;
            for (; j + 4 < rlen; j += 4) {
#pragma unroll
                for (uint32_t i = 0; i < 4; ++i) {
                    apply(e[i]);
                    e[i] = row_entry<F16>(p.entries, rb, min(j + 4 + i, last));
                    // one entry at a time: interleaving the four entries' products would need the registers that hold the vertex's
                    // skin data, which would then be spilled here and RELOADED between the instances' stores (see SKIN)
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
            apply(e[0]);
            if (j + 1 < rlen) apply(e[1]);
            if (j + 2 < rlen) apply(e[2]);
            if (j + 3 < rlen) apply(e[3]);
        }
        // the next pack's slot weights: requested now, in LDS after this pack's instances
        const bool more = g0 + kPkPack < gcount;
        float4 wnext = make_float4(0.f, 0.f, 0.f, 0.f);
        if (more && wreg && uint32_t(tid) < wstride) wnext = pack_weight(g0 + kPkPack, uint32_t(tid));
        // coordinate = base + image (poser_impl.inl:407): instance 0 in registers, 1..3 to this thread's words of mp
        v2f cxy = ps.pxy + axy[0];
        float cz = ps.pz + az01.x;
        {
            int t = tid;
            asm volatile("" : "+v"(t));
            float *m1 = reinterpret_cast<float *>(mp + 1 * kPkRegion), *m2 = reinterpret_cast<float *>(mp + 2 * kPkRegion),
                  *m3 = reinterpret_cast<float *>(mp + 3 * kPkRegion);
            const v2f c1 = ps.pxy + axy[1], c2 = ps.pxy + axy[2], c3 = ps.pxy + axy[3];
            m1[t] = c1.x; m1[kTileVerts + t] = c1.y; m1[2 * kTileVerts + t] = ps.pz + az01.y;
            m2[t] = c2.x; m2[kTileVerts + t] = c2.y; m2[2 * kTileVerts + t] = ps.pz + az23.x;
            m3[t] = c3.x; m3[kTileVerts + t] = c3.y; m3[2 * kTileVerts + t] = ps.pz + az23.y;
        }
        PK_STAMP(1);
        // ---- SKIN: the pack's instances, one barrier each.  No vector-memory LOAD may sit in here: it would have to wait for the
        // previous instance's stores to drain (vmcnt is in order), microseconds under a saturated HBM. ---------------------------
        auto instance = [&](const uint32_t j, auto last_tag) {
            constexpr bool kLast = decltype(last_tag)::value;       // the pack's fourth instance: the next walk's row head goes out with it
            const uint32_t inst = first_instance(g0) + j;
            const size_t vbase = size_t(inst) * p.pitch + v0;
            const uint32_t sh4 = al ? uint32_t((vbase * 3) & 3) : 0u, sh8 = al ? uint32_t((vbase * 3) & 7) : 0u;
            unsigned char *ia = mp + j * kPkRegion, *ib = imgB + buf * kSoaImgBytes;
            // (in place: the values stay in their registers, the compiler merely stops treating them as loop invariants -- whose
            // derived values it would otherwise carry around the loops in registers of their own)
            asm volatile("" : "+v"(ps.meta), "+v"(ps.b01), "+v"(ps.b23), "+v"(ps.w0), "+v"(ps.w1), "+v"(ps.w2), "+v"(ps.w3), "+v"(ps.nxy),
                         "+v"(ps.nz));
            const uint32_t meta = ps.meta, b01 = ps.b01, b23 = ps.b23;
            const float w0 = ps.w0, w1 = ps.w1, w2 = ps.w2, w3 = ps.w3, nx = ps.nxy.x, ny = ps.nxy.y, nz = ps.nz;
            int t = tid;
            asm volatile("" : "+v"(t));
            if (meta >> 12) {
                const M12 m = skin_matrix_packed((meta >> 10) & 3u, b01, b23, w0, w1, w2, w3, pal + size_t(g0 + j) * p.pal_stride);
                v2f oxy, rxy;
                float oz, rz;
                xform_pos(m, cxy, cz, oxy, oz);
                xform_nrm(m, v2f{nx, ny}, nz, rxy, rz);
                oxy = oxy * p.pos_scale;                 // a separate multiply after the transform (main.cpp:848-850)
                oz = oz * p.pos_scale;
                const uint32_t perm3 = (meta & 1023u) * 3;
                float *B = reinterpret_cast<float *>(ib) + sh4 + perm3;
                if constexpr (LAYOUT == MMDX_OUT_SOA) {
                    float *A = reinterpret_cast<float *>(ia) + sh4 + perm3;
                    A[0] = oxy.x; A[1] = oxy.y; A[2] = oz;
                } else {
                    unsigned short *A = reinterpret_cast<unsigned short *>(ia) + sh8 + perm3;
                    A[0] = f2h(oxy.x); A[1] = f2h(oxy.y); A[2] = f2h(oz);
                }
                B[0] = rxy.x; B[1] = rxy.y; B[2] = rz;
            }
            if (!kLast) {                   // the next instance's coordinate, before anybody may overwrite it with that instance's image
                const float *mn = reinterpret_cast<const float *>(mp + (j + 1) * kPkRegion);
                cxy = v2f{mn[t], mn[kTileVerts + t]};
                cz = mn[2 * kTileVerts + t];
            }
            PK_STAMP(2);
            __syncthreads();
            PK_STAMP(3);
            // the head of the row for the next pack's walk goes out IN FRONT of the pack's last stores: its round trip then runs
            // beside their drain instead of behind it
            if constexpr (kLast) { if (more) row_head(); }
            if constexpr (LAYOUT == MMDX_OUT_SOA) {
                float *oa = reinterpret_cast<float *>(p.out_a), *ob = reinterpret_cast<float *>(p.out_b);
                if (fast)
                    copy_out_fast<kPkThreads, kTileVerts * 12 / 16, kTileVerts * 12 / 16>(
                        ia, uint32_t(ib - ia), reinterpret_cast<float4 *>(oa + vbase * 3), reinterpret_cast<float4 *>(ob + vbase * 3), t);
                else
                    copy_out2<kPkThreads, float, float>(ia, oa, vbase * 3, sh4, nvt * 3, ib, ob, vbase * 3, sh4, nvt * 3, al, t);
            } else {
                unsigned short *oa = reinterpret_cast<unsigned short *>(p.out_a);
                float *ob = reinterpret_cast<float *>(p.out_b);
                if (fast)
                    copy_out_fast<kPkThreads, kTileVerts * 6 / 16, kTileVerts * 12 / 16>(
                        ia, uint32_t(ib - ia), reinterpret_cast<float4 *>(oa + vbase * 3), reinterpret_cast<float4 *>(ob + vbase * 3), t);
                else
                    copy_out2<kPkThreads, unsigned short, float>(ia, oa, vbase * 3, sh8, nvt * 3, ib, ob, vbase * 3, sh4, nvt * 3, al, t);
            }
            buf ^= 1u;
            PK_STAMP(4);
        };
#ifdef PK_SKIP_SKIN
        if (cz == 12345.678f && cxy.x == 9.75f) instance(0, std::true_type{});      // (keeps the walk's results alive)
#else
#pragma unroll 1
        for (uint32_t j = 0; j + 1 < kPkPack; ++j) {
            if (first_instance(g0) + j >= p.ni) break;
            instance(j, std::false_type{});
        }
        if (first_instance(g0) + kPkPack - 1 < p.ni) instance(kPkPack - 1, std::true_type{});
#endif
        if (more) {
            // every wave has left this pack's walk (it passed the instances' barriers): the weights can be replaced.  The barrier
            // also closes the last instance's copy-out reads before the next walk's coordinates land in mp.
            if (wreg) {
                if (uint32_t(tid) < wstride) wq[tid] = wnext;
            } else {
                for (uint32_t i = tid; i < wstride; i += kPkThreads) wq[i] = pack_weight(g0 + kPkPack, i);
            }
            __syncthreads();
        }
        PK_STAMP(5);
    }
#ifdef PK_STAMPS
    if ((tid & 63) == 0 && p.stamps) {
        unsigned long long *o = p.stamps + (size_t(blockIdx.x) * 8 + (uint32_t(tid) >> 6)) * 8;
        for (int k = 0; k < 6; ++k) o[k] = st_acc[k];
        o[6] = st_begin; o[7] = st_t;
    }
#endif
}

// The instantiation for a call: kernels.hip, among the other dispatch functions -- the order in which those first name the kernel
// templates is the order of the instantiations in the code object.
KernelFn pick_pack(int layout, bool f16, bool finite);

hipError_t launch_pack(int layout, bool f16, const DeformParams &p, uint32_t ntiles, size_t lds_bytes, hipStream_t stream) {
    KernelFn fn = pick_pack(layout, f16, p.finite_offsets != 0);
    if (!fn || kTileVerts != 512) return hipErrorInvalidValue;
    DeformParams q = p;
    const dim3 grid = xcd_grid(q, ntiles, p.ni);
#ifdef PK_STAMPS
    static unsigned long long *stamps = nullptr;
    static size_t stamps_n = 0;
    const size_t need = size_t(grid.x) * 64;
    if (stamps_n < need) { if (stamps) (void)hipFree(stamps); (void)hipMalloc(&stamps, need * 8); stamps_n = need; }
    (void)hipMemsetAsync(stamps, 0, need * 8, stream);
    q.stamps = stamps;
#endif
    hipLaunchKernelGGL(fn, grid, dim3(kPkThreads), lds_bytes, stream, q);
#ifdef PK_STAMPS
    {
        static int calls = 0;
        if (++calls % 16 == 0) {            // now and then: wait, fetch, print the means (diagnostic build only)
            (void)hipStreamSynchronize(stream);
            std::vector<unsigned long long> h(need);
            (void)hipMemcpy(h.data(), stamps, need * 8, hipMemcpyDeviceToHost);
            const char *names[6] = {"sync/top", "walk", "skin", "barrier", "copy-out", "pack-end"};
            for (int w : {0, 3, 7}) {
                double acc[6] = {0, 0, 0, 0, 0, 0}, life = 0; size_t n = 0;
                unsigned long long t0 = ~0ull, t1 = 0;
                for (size_t b = 0; b < grid.x; ++b) {
                    const unsigned long long *r = h.data() + (b * 8 + w) * 8;
                    if (!r[7]) continue;
                    for (int k = 0; k < 6; ++k) acc[k] += double(r[k]);
                    life += double(r[7] - r[6]); ++n;
                    t0 = std::min(t0, r[6]); t1 = std::max(t1, r[7]);
                }
                if (!n) continue;
                std::fprintf(stderr, "pk-stamps wave %d: n=%zu life %.0f ticks |", w, n, life / n);
                for (int k = 0; k < 6; ++k) std::fprintf(stderr, " %s %.0f (%.0f%%)", names[k], acc[k] / n, 100.0 * acc[k] / life);
                std::fprintf(stderr, " | kernel span %llu ticks\n", t1 - t0);
            }
        }
    }
#endif
    return hipGetLastError();
}

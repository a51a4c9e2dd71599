// kernels_setup.inl -- how a workgroup of the deform kernels finds its work and stages it: the XCD-aware mapping (device side and
// the grid the host launches for it), static vertex data into registers, bone palettes into LDS, the latency-ordered set-up of the
// one-set-of-rates kernels, the start stagger.
// A piece of kernels.hip (included inside namespace mmdx { namespace {), compiled with it, plain and fast-math.

// ---- pieces shared by the deform kernels ------------------------------------------------------------
// XCD-aware work mapping (speed only, never correctness): workgroup ids are dealt round-robin over
// the 8 XCDs, each with a private 4 MiB L2.  XCD x gets a CONTIGUOUS range of tiles for all
// instance groups, tile index fastest, so the ~96 workgroups resident on one XCD are (its ~12 tiles)
// x (8 groups): a tile's static streams and the palette rows neighbouring tiles share are fetched
// into that L2 once instead of once per XCD.  Tiles left over by ntiles % 8 are split by groups.
// Returns false for a padding workgroup.
// (Round 3 tried walking an XCD's tiles in CHUNKS -- few tiles x all their instance groups resident together, so that the
// per-instance-morph kernels fetch a tile's morph-table slice into L2 once per launch instead of once per group: config 5 x 64
// and config 2 x 64 unchanged within noise, config 3' 7 % slower at 1-2 tiles per chunk; profiles/r03/xcd_chunk_sweep.txt.)
__device__ __forceinline__ bool map_workgroup(const DeformParams &p, uint32_t &tile, uint32_t &grp) {
    const uint32_t xcd = blockIdx.x & 7u, k = blockIdx.x >> 3;
    const uint32_t T = p.ntiles >> 3, main_count = T * p.ngroups;
    if (k < main_count) {
        grp = k / T;
        tile = xcd * T + (k - grp * T);
        return true;
    }
    const uint32_t r = xcd * p.rem_per_xcd + (k - main_count);
    if (r >= (p.ntiles & 7u) * p.ngroups) return false;
    const uint32_t rt = r / p.ngroups;
    tile = 8u * T + rt;
    grp = r - rt * p.ngroups;
    return true;
}

// The host side of map_workgroup: the three fields it reads (groups of q.group instances over `count` instances or list positions)
// and the grid they describe -- per XCD, the main tiles x groups plus its share of the left-over tiles' groups, padded to equal.
dim3 xcd_grid(DeformParams &q, uint32_t ntiles, uint32_t count) {
    q.ntiles = ntiles;
    q.ngroups = (count + q.group - 1) / q.group;
    q.rem_per_xcd = ((ntiles & 7u) * q.ngroups + 7u) / 8u;
    return dim3(8u * ((ntiles >> 3) * q.ngroups + q.rem_per_xcd));
}

// static per-vertex data of sorted slot s of tile `th` -> registers
template <int LAYOUT, int MORPH, bool F16>
__device__ __forceinline__ void load_slot(const DeformParams &p, const TileHdr &th, uint32_t s, Slot &q) {
    const uint32_t n1 = th.n1, n12 = th.n1 + th.n2;
    q.act = s < th.nv;
    q.cls = s < n1 ? 0 : (s < n12 ? 1 : 2);
    q.pxy = q.nxy = q.uv = v2f{0.f, 0.f};
    q.pz = q.nz = 0.f;
    q.w0 = q.w1 = q.w2 = q.w3 = 0.f;
    q.b0 = q.b1 = q.b2 = q.b3 = 0;
    q.perm = 0; q.rb = q.rlen = 0;
    if (!q.act) return;
    const size_t gs = size_t(th.v0) + s;
    if constexpr (MORPH == kMorphShared) {
        q.pxy = v2f{p.morphed[gs * 3], p.morphed[gs * 3 + 1]}; q.pz = p.morphed[gs * 3 + 2];
    } else if constexpr (F16) {
        const uint2 r = reinterpret_cast<const uint2 *>(p.spos)[gs];
        q.pxy = v2f{h2f(r.x & 0xffffu), h2f(r.x >> 16)}; q.pz = h2f(r.y & 0xffffu);
    } else {
        const float *sp = reinterpret_cast<const float *>(p.spos) + gs * 3;
        q.pxy = v2f{sp[0], sp[1]}; q.pz = sp[2];
    }
    q.nxy = v2f{p.snrm[gs * 3], p.snrm[gs * 3 + 1]}; q.nz = p.snrm[gs * 3 + 2];
    if constexpr (LAYOUT == MMDX_OUT_VERTEX32) {
        const float2 uv = reinterpret_cast<const float2 *>(p.suv)[gs];
        q.uv = v2f{uv.x, uv.y};
    }
    q.perm = p.perm[gs];
    if constexpr (MORPH == kMorphFused1 || MORPH == kMorphFused4) {
        const uint2 sl2 = p.ell[gs >> 6];            // slice of this wave-slot (wave-uniform)
        q.rb = sl2.x + uint32_t(gs & 63); q.rlen = sl2.y;
    }
    if (q.cls == 0) {
        q.b0 = uint32_t(p.skin1[th.skin1_off + s]) * 3;
    } else if (q.cls == 1) {
        const uint32_t i = th.skin2_off + (s - n1);
        const uint32_t ids = p.skin2_ids[i];
        q.b0 = (ids & 0xffffu) * 3; q.b1 = (ids >> 16) * 3;
        q.w0 = p.skin2_w[i];
    } else {
        const uint32_t i = th.skin4_off + (s - n12);
        const uint2 ids = p.skin4_ids[i];
        const float4 w = p.skin4_w[i];
        q.b0 = (ids.x & 0xffffu) * 3; q.b1 = (ids.x >> 16) * 3;
        q.b2 = (ids.y & 0xffffu) * 3; q.b3 = (ids.y >> 16) * 3;
        q.w0 = w.x; q.w1 = w.y; q.w2 = w.z; q.w3 = w.w;
    }
}

// A word of the instance list of a select launch (the live count, the id of a workgroup's current instance) at a wave-uniform
// address, read through the constant address space: the list is never written while the kernel runs, and said this way the load
// is a scalar one (s_load_dword) wherever it stands -- behind the stagger's sleep or the previous instance's stores the compiler
// would otherwise take a vector load plus readfirstlane.
__device__ __forceinline__ uint32_t uniform_u32(const uint32_t *q) {
    return *reinterpret_cast<const __attribute__((address_space(4))) uint32_t *>(reinterpret_cast<uintptr_t>(q));
}

// bone palettes of `count` instances (first one `inst0`, then every `istep`-th) -> LDS: only the tile's bones,
// in the pair layout load_m12 reads.  One wave-instruction fetches ONE bone for 16 instances (lane = instance x
// matrix row: sixteen 64-byte pieces); the bone id is wave-uniform, so it comes through the scalar cache and the
// palette loads do not wait for a vector load of the bone list first -- one dependent round trip less in a
// set-up phase that runs while the CU's memory pipeline is full of other workgroups' stores.
// `qstep` != 0: the group is made of instance QUADS qstep quads apart (pack_kernel's interleaved mapping): group instance g is
// instance inst0 + (g >> 2) * 4 * qstep + (g & 3); instances past the crowd's end are left out.
// SEL (select launches): inst0 / istep are list positions, the instance is p.sel_ids[position] (one load per lane, in front of the
// palette rows it addresses: set-up only); ids >= p.ni are left out like instances past the crowd's end.
template <int THREADS, bool SEL = false>
__device__ __forceinline__ void stage_palettes(const DeformParams &p, const TileHdr &th, float4 *pal, uint32_t inst0,
                                               uint32_t istep, uint32_t count, int tid, uint32_t qstep = 0u) {
    const uint32_t nbt = th.nbt;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(uint32_t(tid) >> 6), lane = uint32_t(tid) & 63u;
    const uint32_t gl = lane >> 2, r = lane & 3u;
    const uint32_t *bones = p.bone_list + th.bone_off;
    for (uint32_t g0 = 0; g0 < count; g0 += 16) {
        const uint32_t g = g0 + gl;
        uint32_t inst = inst0 + (g < count ? g : 0u) * istep;
        if (qstep) inst = inst0 + (g >> 2) * 4u * qstep + (g & 3u);
        if constexpr (SEL) inst = p.sel_ids[inst];          // (g >= count reads position inst0: inside the live prefix)
        const bool on = g < count && inst < p.ni;
        const float *src = p.palettes + size_t(on ? inst : inst0) * p.nb * 16 + r * 4;     // (off: never dereferenced)
        float *dst = reinterpret_cast<float *>(pal + size_t(g) * p.pal_stride);
#pragma unroll 4
        for (uint32_t lb = wave; lb < nbt; lb += THREADS / 64) {
            const uint32_t bone = bones[lb];                 // wave-uniform: scalar load
            if (on) {
                const float4 row = *reinterpret_cast<const float4 *>(src + size_t(bone) * 16);
                // entry = {m00 m01 | m10 m11} {m20 m21 | m30 m31} {m02 m12 | m22 m32}; this lane holds row r
                float *e = dst + lb * 12;
                *reinterpret_cast<float2 *>(e + (r >> 1) * 4 + (r & 1u) * 2) = make_float2(row.x, row.y);
                e[8 + r] = row.z;
            }
        }
    }
}

// Set-up of the one-set-of-rates kernel (kMorphFused1: a single-model frame, small crowds with a shared facial state), ordered
// for LATENCY: such a launch is a handful of workgroups whose run time is the length of their chain of dependent memory round
// trips (config 2, one frame: 9.6 MB in ~8 us).  Everything that depends on the tile header only is requested first (static
// vertex data, bone ids of the palette rows, slot tables), then everything that depends on those (the first BH entries of the
// threads' morph rows, the palette rows, the morph rates), and only then does anything wait: two round trips instead of the six
// or seven of "palettes, then weights, then vertices, then rows".  One batch of kPalBatch palette rows / kWgtBatch slots per
// thread is handled this way; what does not fit (large groups, thousands of slots) follows in plain loops.
constexpr int kPalBatch = 4, kWgtBatch = 4;

// SEL (select launches): inst0 / istep are list positions; a row of an id >= p.ni is staged as zeros (its instance is never skinned).
template <int THREADS, int LAYOUT, int MORPH, bool F16, int VPT, uint32_t BH, bool SEL = false>
__device__ __forceinline__ void setup_fused1(const DeformParams &p, const TileHdr &th, float4 *pal, float *wl, uint32_t inst0,
                                             uint32_t istep, uint32_t gcount, int tid, uint32_t slot_base, Slot (&sl)[VPT],
                                             RowHead<F16, BH> (&hd)[VPT]) {
    constexpr bool kWalk = MORPH == kMorphFused1;         // kMorphNone: palettes and static data only
    const uint32_t nb4 = th.nbt * 4u, rows = gcount * nb4, ns = p.ns;
    const uint32_t *bones = p.bone_list + th.bone_off;
    const bool flat = p.fused_rates == nullptr;          // slot weights already evaluated (p.wslot)
    // palette row e = (instance g of the group, tile bone lb, matrix row r): e = (g * nbt + lb) * 4 + r
    auto row_src = [&](uint32_t e, uint32_t bone) {
        const uint32_t g = gcount == 1 ? 0u : e / nb4;
        uint32_t inst = inst0 + g * istep;
        if constexpr (SEL) {
            inst = p.sel_ids[inst];
            if (inst >= p.ni) inst = 0u;                     // a skipped id: any readable row, never used
        }
        return reinterpret_cast<const float4 *>(p.palettes + size_t(inst) * p.nb * 16 + size_t(bone) * 16 + (e & 3u) * 4);
    };
    auto row_put = [&](uint32_t e, const float4 row) {
        const uint32_t g = gcount == 1 ? 0u : e / nb4, rem = e - g * nb4, lb = rem >> 2, r = rem & 3u;
        // entry = {m00 m01 | m10 m11} {m20 m21 | m30 m31} {m02 m12 | m22 m32}; this element is row r
        float *en = reinterpret_cast<float *>(pal + size_t(g) * p.pal_stride) + lb * 12;
        *reinterpret_cast<float2 *>(en + (r >> 1) * 4 + (r & 1u) * 2) = make_float2(row.x, row.y);
        en[8 + r] = row.z;
    };
    auto chain = [&](float r, uint32_t c0, uint32_t c1) {     // slot_weight() from the rate of the slot's top-level morph on
        bool skip = r < kMorphEps;
        for (uint32_t c = c0; !skip && c < c1; ++c) {
            r = p.chain_rate[c] * r;
            skip = r < kMorphEps;
        }
        return skip ? 0.f : r;
    };

    // ---- round trip 1: static vertex data, bone ids, slot tables ---------------------------------------------------------
#pragma unroll
    for (int k = 0; k < VPT; ++k) load_slot<LAYOUT, MORPH, F16>(p, th, slot_base + uint32_t(tid) + uint32_t(k) * THREADS, sl[k]);
    uint32_t bone[kPalBatch];
#pragma unroll
    for (int i = 0; i < kPalBatch; ++i) {
        const uint32_t e = uint32_t(tid) + uint32_t(i) * THREADS;
        bone[i] = e < rows ? bones[((gcount == 1 ? e : e % nb4)) >> 2] : 0u;
    }
    uint32_t top[kWgtBatch], c0[kWgtBatch], c1[kWgtBatch];
    float wv[kWgtBatch];
#pragma unroll
    for (int i = 0; i < kWgtBatch; ++i) {
        const uint32_t sidx = uint32_t(tid) + uint32_t(i) * THREADS;
        top[i] = c0[i] = c1[i] = 0u;
        wv[i] = 0.f;
        if (kWalk && sidx < ns) {
            if (flat) wv[i] = p.wslot[sidx];
            else { top[i] = p.slot_top[sidx]; c0[i] = p.chain_off[sidx]; c1[i] = p.chain_off[sidx + 1]; }
        }
    }
    // ---- round trip 2: the heads of the morph rows, the palette rows, the rates ---------------------------------------------
    if constexpr (kWalk) {
#pragma unroll
        for (int k = 0; k < VPT; ++k) row_prefetch<F16, BH>(p.entries, sl[k].rb, sl[k].rlen, hd[k]);
    }
    float4 row[kPalBatch];
#pragma unroll
    for (int i = 0; i < kPalBatch; ++i) {
        const uint32_t e = uint32_t(tid) + uint32_t(i) * THREADS;
        row[i] = e < rows ? *row_src(e, bone[i]) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    if (kWalk && !flat) {
#pragma unroll
        for (int i = 0; i < kWgtBatch; ++i)
            if (uint32_t(tid) + uint32_t(i) * THREADS < ns) wv[i] = p.fused_rates[top[i]];
    }
    // ---- into LDS -----------------------------------------------------------------------------------------------------------
#pragma unroll
    for (int i = 0; i < kPalBatch; ++i) {
        const uint32_t e = uint32_t(tid) + uint32_t(i) * THREADS;
        if (e < rows) row_put(e, row[i]);
    }
    if constexpr (kWalk) {
#pragma unroll
        for (int i = 0; i < kWgtBatch; ++i) {
            const uint32_t sidx = uint32_t(tid) + uint32_t(i) * THREADS;
            if (sidx <= ns) wl[sidx] = sidx < ns ? (flat ? wv[i] : chain(wv[i], c0[i], c1[i])) : 0.f;   // slot ns = table padding, weight 0
        }
    }
    // ---- what did not fit the first batch -------------------------------------------------------------------------------------
    for (uint32_t e = uint32_t(kPalBatch) * THREADS + uint32_t(tid); e < rows; e += THREADS)
        row_put(e, *row_src(e, bones[(e % nb4) >> 2]));
    if constexpr (kWalk) {
        for (uint32_t sidx = uint32_t(kWgtBatch) * THREADS + uint32_t(tid); sidx <= ns; sidx += THREADS)
            wl[sidx] = sidx < ns ? (flat ? p.wslot[sidx] : slot_weight(p.fused_rates, p.slot_top, p.chain_off, p.chain_rate, sidx)) : 0.f;
    }
}

// Workgroups of one CU that run the same program start together and stay in step: all in their walk (vector-memory loads), then
// all in their stores.  First-round workgroups are therefore started out of phase: residency slot k of a CU (blocks are dealt
// round-robin over the 8 XCDs, then over an XCD's 32 CUs: observed, speed only) sleeps k * stagger * 64 cycles first.  Later
// workgroups inherit the offset of the one whose place they take.
__device__ __forceinline__ void stagger_start(const DeformParams &p) {
    if (p.stagger == 0u || p.slots_per_cu < 2u) return;
    const uint32_t round = blockIdx.x >> 8;                 // 8 XCDs x 32 CUs
    if (round >= p.slots_per_cu) return;
    for (uint32_t k = 0; k < round * p.stagger; k += 100) __builtin_amdgcn_s_sleep(100);
}

// kernels_deform.inl -- deform_kernel, the crowd kernel (every morph mode; 256- and 512-thread, tile-order, write-through, bounds
// and select flavours), and skin_instance, the one instance it skins and writes out per step of its loop.
// A piece of kernels.hip (included inside namespace mmdx { namespace {), compiled with it, plain and fast-math.

// One instance: skin the thread's slots with the palette at P (LDS), scatter the results to the LDS image `img`
// (undoing the class sort), ONE workgroup barrier, then write the image out with coalesced 16-byte stores.
// `inst` = the instance's index in the output arrays, cxy / cz = the (morphed) positions of the thread's slots.
// BOUNDS: also the min / max of the positions as written (pos_scale applied, binary16 widened back), reduced over the wave in
// registers, then over the workgroup through `bo.lds` across the barrier the image already needs (tile order: no barrier, one
// partial per wave).
template <int THREADS, int LAYOUT, int VPT, bool TILE, bool ALL_FAST, bool WT = false, bool BOUNDS = false>
__device__ __forceinline__ void skin_instance(const DeformParams &p, const Slot (&sl)[VPT], const float4 *P,
                                              unsigned char *img, uint32_t inst, uint32_t v0, uint32_t nvt,
                                              const v2f (&cxy)[VPT], const float (&cz)[VPT], int tid,
                                              BoundsOut bo = BoundsOut{nullptr, nullptr}) {
    const size_t vbase = size_t(inst) * p.pitch + v0;  // first output vertex of this tile
    const bool al = p.out_aligned != 0;
    const uint32_t sh4 = al ? uint32_t((vbase * 3) & 3) : 0u;
    const uint32_t sh8 = al ? uint32_t((vbase * 3) & 7) : 0u;
    float bmn[3], bmx[3];
    if constexpr (BOUNDS) {
#pragma unroll
        for (int c = 0; c < 3; ++c) bmn[c] = bmx[c] = __builtin_nanf("");
    }
#pragma unroll
    for (int k = 0; k < VPT; ++k) {
        const Slot &q = sl[k];
        if (!q.act) continue;
        const M12 m = skin_matrix(q, P);
        v2f oxy, rxy;
        float oz, rz;
        xform_pos(m, cxy[k], cz[k], oxy, oz);
        xform_nrm(m, q.nxy, q.nz, rxy, rz);
        // pos_scale is a separate multiply after the transform (main.cpp:848-850); x*1.0f == x
        oxy = oxy * p.pos_scale;
        oz = oz * p.pos_scale;
        if constexpr (BOUNDS) {
            float w[3] = {oxy.x, oxy.y, oz};
            if constexpr (LAYOUT == MMDX_OUT_SOA_POS16) {
#pragma unroll
                for (int c = 0; c < 3; ++c) w[c] = h2f(f2h(w[c]));      // the value as stored
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) { bmn[c] = bound_op<false>(bmn[c], w[c]); bmx[c] = bound_op<true>(bmx[c], w[c]); }
        }
        if constexpr (TILE) {
            // MMDX_CREATE_TILE_ORDER (a compile-time variant: the default kernels' code is untouched by it): the vertex keeps its sorted slot in the output -- consecutive lanes write consecutive
            // vertices (12 / 32 / 6 bytes apart) straight from registers: no image, no barrier, no wave waits for another
            const size_t v = vbase + uint32_t(tid) + uint32_t(k) * THREADS;
            if constexpr (LAYOUT == MMDX_OUT_SOA) {
                float *A = reinterpret_cast<float *>(p.out_a) + v * 3, *B = reinterpret_cast<float *>(p.out_b) + v * 3;
                store3(A, oxy.x, oxy.y, oz);
                store3(B, rxy.x, rxy.y, rz);
            } else if constexpr (LAYOUT == MMDX_OUT_VERTEX32) {
                float *A = reinterpret_cast<float *>(p.out_a) + v * 8;
                if (al) {
                    store16(reinterpret_cast<float4 *>(A), make_float4(oxy.x, oxy.y, oz, rxy.x));
                    store16(reinterpret_cast<float4 *>(A) + 1, make_float4(rxy.y, rz, q.uv.x, q.uv.y));
                } else {
                    A[0] = oxy.x; A[1] = oxy.y; A[2] = oz; A[3] = rxy.x; A[4] = rxy.y; A[5] = rz; A[6] = q.uv.x; A[7] = q.uv.y;
                }
            } else {
                unsigned short *A = reinterpret_cast<unsigned short *>(p.out_a) + v * 3;
                float *B = reinterpret_cast<float *>(p.out_b) + v * 3;
                A[0] = f2h(oxy.x); A[1] = f2h(oxy.y); A[2] = f2h(oz);
                B[0] = rxy.x; B[1] = rxy.y; B[2] = rz;
            }
            continue;
        }
        if constexpr (LAYOUT == MMDX_OUT_SOA) {
            float *A = reinterpret_cast<float *>(img) + sh4 + q.perm * 3;
            float *B = reinterpret_cast<float *>(img + kSoaImgBytes) + sh4 + q.perm * 3;
            A[0] = oxy.x; A[1] = oxy.y; A[2] = oz;
            B[0] = rxy.x; B[1] = rxy.y; B[2] = rz;
        } else if constexpr (LAYOUT == MMDX_OUT_VERTEX32) {
            float4 *I = reinterpret_cast<float4 *>(img) + q.perm * 2;
            I[0] = make_float4(oxy.x, oxy.y, oz, rxy.x);
            I[1] = make_float4(rxy.y, rz, q.uv.x, q.uv.y);
        } else {
            unsigned short *A = reinterpret_cast<unsigned short *>(img) + sh8 + q.perm * 3;
            float *B = reinterpret_cast<float *>(img + kP16ImgBytes) + sh4 + q.perm * 3;
            A[0] = f2h(oxy.x); A[1] = f2h(oxy.y); A[2] = f2h(oz);
            B[0] = rxy.x; B[1] = rxy.y; B[2] = rz;
        }
    }
    if constexpr (BOUNDS) {
        const uint32_t lane = uint32_t(tid) & 63u, wave = uint32_t(tid) >> 6;
        const float v = wave_bounds6(bmn, bmx, lane);
        if (lane < 6) (TILE ? bo.out : bo.lds)[wave * 6 + lane] = v;
    }
    if constexpr (TILE) return;
    __syncthreads();
    if constexpr (BOUNDS) {
        // the waves' partials -> this (instance, tile)'s.  The words of this parity are rewritten two instances later, after the
        // next instance's barrier, which no wave passes before these reads are done.
        if (tid < 6) {
            float r = bo.lds[tid];
#pragma unroll
            for (int w = 1; w < THREADS / 64; ++w)
                r = tid < 3 ? bound_op<false>(r, bo.lds[w * 6 + tid]) : bound_op<true>(r, bo.lds[w * 6 + tid]);
            bo.out[tid] = r;
        }
    }
    // ALL_FAST: the kernel found, once per workgroup, that every instance of this full tile starts on a 16-byte boundary; the
    // generic copy-out is then not even compiled into the instance loop (1-2 % of the crowd step: measured)
    const bool fast = ALL_FAST || (al && nvt == kTileVerts && sh4 == 0 && sh8 == 0);
    if constexpr (LAYOUT == MMDX_OUT_SOA) {
        float *oa = reinterpret_cast<float *>(p.out_a), *ob = reinterpret_cast<float *>(p.out_b);
        if (fast)
            copy_out_fast<THREADS, kTileVerts * 12 / 16, kTileVerts * 12 / 16, WT>(
                img, kSoaImgBytes, reinterpret_cast<float4 *>(oa + vbase * 3),
                reinterpret_cast<float4 *>(ob + vbase * 3), tid);
        else
            copy_out2<THREADS, float, float>(img, oa, vbase * 3, sh4, nvt * 3, img + kSoaImgBytes, ob,
                                             vbase * 3, sh4, nvt * 3, al, tid);
    } else if constexpr (LAYOUT == MMDX_OUT_VERTEX32) {
        float *oa = reinterpret_cast<float *>(p.out_a);
        if (fast)
            copy_out_fast<THREADS, kTileVerts * 32 / 16, 0>(
                img, 0u, reinterpret_cast<float4 *>(oa + vbase * 8), nullptr, tid);
        else
            copy_out2<THREADS, float, float>(img, oa, vbase * 8, 0u, nvt * 8, img, oa, 0, 0u, 0u, al,
                                             tid);
    } else {
        unsigned short *oa = reinterpret_cast<unsigned short *>(p.out_a);
        float *ob = reinterpret_cast<float *>(p.out_b);
        if (fast)
            copy_out_fast<THREADS, kTileVerts * 6 / 16, kTileVerts * 12 / 16>(
                img, kP16ImgBytes, reinterpret_cast<float4 *>(oa + vbase * 3),
                reinterpret_cast<float4 *>(ob + vbase * 3), tid);
        else
            copy_out2<THREADS, unsigned short, float>(img, oa, vbase * 3, sh8, nvt * 3,
                                                      img + kP16ImgBytes, ob, vbase * 3, sh4, nvt * 3,
                                                      al, tid);
    }
}

// ---- the deformation kernel ----------------------------------------------------------------------
// THREADS = 512: one sorted slot per lane, 8 waves per workgroup; THREADS = 256: two slots per lane.
// BOUNDS: the flavour of mmdx_deform_batched_bounds -- the same outputs, bit for bit, plus 6 floats of partial bounds per (instance,
// tile), per (instance, tile, wave) for tile-order outputs, in p.bounds, which bounds_reduce_kernel folds into [NI][6].  Only with
// WT = false: bounds calls store cached (api.cpp), no write-through bounds variant is built.
// (A template parameter of this kernel, not a device function shared by two kernels: that wrapping alone moved the register
// allocation of the per-instance-morph kernels by +-2 VGPRs; this way BOUNDS = false is the previous kernel's code.)
// SELECT: the flavour of mmdx_deform_batched_select -- the workgroup's instances come from a list in device memory: list position j
// -> instance p.sel_ids[j] for the palette staging, the output base and nothing else (slot weights and partial bounds are indexed
// by j).  The live count is one word (scalar load, once per workgroup); a workgroup whose positions lie behind it returns before
// it stages anything; an id >= p.ni is skipped.  List positions are dealt over the workgroups like the instances of the plain
// crowd call: interleaved (g*ngroups + grp) with p.sel_interleave, else blocked (grp*group + g; always for per-instance rates,
// whose slot weights are packed by quads of positions).  Interleaved is the default: a short live prefix then keeps every
// workgroup of the grid busy with a few instances, and re-reading the tile's static streams per few instances (they stay in the
// XCD's L2) measured cheaper than running a quarter of the workgroups with full groups.
// Like BOUNDS a compile-time flavour, so that without it the kernel is the previous kernel's code.  It travels as a bit of the
// morph-mode argument (kMorphSelect), not as one more template parameter: the names of the existing instantiations, which the
// resource listings and their checks go by, stay what they were.
template <int THREADS, int LAYOUT, int MORPH_MODE, bool F16, bool TILE, bool WT = false, bool BOUNDS = false>
__global__ __launch_bounds__(THREADS) void deform_kernel(const DeformParams p) {
    constexpr int MORPH = MORPH_MODE & 3;
    constexpr bool SELECT = (MORPH_MODE & kMorphSelect) != 0;
    constexpr int VPT = int(kTileVerts) / THREADS;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x;
    uint32_t tile, grp;
    if (!map_workgroup(p, tile, grp)) return;       // padding workgroup
    if constexpr (MORPH == kMorphFused4) stagger_start(p);
    const TileHdr &th = p.tiles[tile];
    const uint32_t v0 = th.v0, nvt = th.nv;
    // Instances of this workgroup.  Blocked: grp*group + g.  Interleaved (crowd modes): g*ngroups + grp,
    // so that the workgroups running at the same time (neighbouring grp) write NEIGHBOURING instances:
    // chip-wide the stores then sweep a few contiguous megabytes of each output array, like a linear
    // fill, instead of 8+ streams 9.6 MB apart.
    // (SELECT: inst0 / istep / gcount count list positions of the live prefix)
    const bool ilv = (MORPH == kMorphNone || MORPH == kMorphShared || MORPH == kMorphFused1) &&
                     (SELECT ? p.sel_interleave != 0 : p.interleave != 0);
    const uint32_t inst0 = ilv ? grp : grp * p.group;
    const uint32_t istep = ilv ? p.ngroups : 1u;
    uint32_t gcount;
    if constexpr (SELECT) {
        const uint32_t nlive = p.sel_count ? min(uniform_u32(p.sel_count), p.sel_n) : p.sel_n;
        // (no "a < b ? min(g, b - a) : 0" here: this compiler turns it into a saturating subtraction whose scalar form wraps)
        const uint32_t end = min(inst0 + p.group, nlive);       // blocked: the first position behind this workgroup's live ones
        gcount = ilv ? min(p.group, (nlive + p.ngroups - 1u - grp) / p.ngroups)       // grp < ngroups: no wrap; 0 when nlive <= grp
                     : (end > inst0 ? end - inst0 : 0u);
    } else {
        gcount = ilv ? (p.ni > grp ? min(p.group, (p.ni - grp + p.ngroups - 1) / p.ngroups) : 0u)
                     : min(p.group, p.ni - inst0);
    }
    if constexpr (SELECT) {
        // nothing live here.  (A small crowd with shared rates walks its morphs in this kernel and workgroup 0 of every tile
        // keeps the morphed positions for later MMDX_MORPH_UNCHANGED calls: those stay, with no instance to write.)
        if (gcount == 0 && !(MORPH == kMorphFused1 && grp == 0 && p.morphed)) return;
    }
    float4 *pal = reinterpret_cast<float4 *>(smem);
    unsigned char *stage = smem + p.stage_off;
    constexpr uint32_t kStage = stage_bytes(LAYOUT);

    Slot sl[VPT];
    // kMorphFused1: entries of a morph row in flight per lane (a single frame is latency-bound and has the registers)
    constexpr uint32_t BH = MORPH == kMorphFused1 ? (F16 ? 16u : 8u) : kRowAhead;
    RowHead<F16, BH> hd[VPT];
    // kMorphFused4: slot weights of one PACK of instances (kQuads quads of four) at a time; the first pack's are
    // requested here, under the set-up's other loads
    constexpr int kQuads = VPT == 1 ? 2 : 1, kPack = 4 * kQuads;
    const uint32_t wstride = p.ns + 1, wcount = uint32_t(kQuads) * wstride;
    // float4 i of the weights of the pack that starts at group instance g0 (a missing second quad reads as zeros:
    // weight +0 adds nothing, bit for bit; its instances are never written out)
    auto pack_weight = [&](uint32_t g0, uint32_t i) {
        const float4 *src = reinterpret_cast<const float4 *>(p.wslot) + size_t((inst0 + g0) / 4) * wstride;
        return (i < wstride || g0 + 4 < gcount) ? src[i] : make_float4(0.f, 0.f, 0.f, 0.f);
    };
    if constexpr (MORPH == kMorphFused1) {
        // palettes, slot weights (ONE set of morph rates for the whole launch; group morphs flattened in here when the raw
        // rates are passed), static vertex data and the heads of the morph rows, in latency order
        setup_fused1<THREADS, LAYOUT, kMorphFused1, F16, VPT, BH, SELECT>(p, th, pal, reinterpret_cast<float *>(smem + p.w_off), inst0, istep,
                                                                   gcount, tid, 0u, sl, hd);
    } else {
        // 1. bone palettes of the group's instances -> LDS: only the tile's bones, in the pair layout
        stage_palettes<THREADS, SELECT>(p, th, pal, inst0, istep, gcount, tid);
        // 2. morph slot weights of the first pack -> LDS
        if constexpr (MORPH == kMorphFused4) {
            float4 *wq0 = reinterpret_cast<float4 *>(smem + p.w_off);
            for (uint32_t i = tid; i < wcount && gcount; i += THREADS) wq0[i] = pack_weight(0, i);
        }
        // 3. static per-vertex data -> registers (sorted slot s = tid + k*THREADS)
#pragma unroll
        for (int k = 0; k < VPT; ++k) load_slot<LAYOUT, MORPH, F16>(p, th, uint32_t(tid) + uint32_t(k) * THREADS, sl[k]);
    }
    __syncthreads();

    uint32_t buf = 0;
    // Every output piece of this workgroup starts on a 16-byte boundary and the tile is full (all but the last tile when the
    // instance pitch -- NV for dense outputs -- is a multiple of 4, 8 for the f16 layout): decided once, the instance loop below
    // is instantiated twice.
    constexpr uint32_t kAlignVerts = LAYOUT == MMDX_OUT_SOA_POS16 ? 8u : (LAYOUT == MMDX_OUT_SOA ? 4u : 1u);
    const bool all_fast = !TILE && p.out_aligned != 0 && nvt == kTileVerts && p.pitch % kAlignVerts == 0 && v0 % kAlignVerts == 0;
    auto instances = [&](auto all_fast_tag) {
    constexpr bool kAllFast = decltype(all_fast_tag)::value;
    // the image is double buffered: the next instance writes the other one, so one barrier per instance is enough
    auto run_instance = [&](uint32_t g, const v2f (&cxy)[VPT], const float (&cz)[VPT]) {
        uint32_t sel_inst = 0u;
        if constexpr (SELECT) {
            sel_inst = uniform_u32(p.sel_ids + (inst0 + g * istep));
            // An id outside the call's arrays: skipped by the whole workgroup (no barrier missed).  (Per-instance rates: a pack
            // made of skipped ids only passes no instance barrier, so a fast wave may replace the pack's slot weights while a slow
            // one still walks with them -- into accumulators that no instance will read.)
            if (sel_inst >= p.ni) return;
        }
        BoundsOut bo{nullptr, nullptr};
        if constexpr (BOUNDS) {
            constexpr uint32_t kUnits = TILE ? uint32_t(THREADS) / 64u : 1u;    // partials per (instance, tile)
            bo.lds = reinterpret_cast<float *>(smem + p.bounds_off) + buf * 48u;
            bo.out = p.bounds + (size_t(inst0 + g * istep) * p.ntiles + tile) * kUnits * 6u;
        }
        if constexpr (SELECT)
            skin_instance<THREADS, LAYOUT, VPT, TILE, kAllFast, WT, BOUNDS>(p, sl, pal + size_t(g) * p.pal_stride, stage + buf * kStage,
                                                                       sel_inst, v0, nvt, cxy, cz, tid, bo);
        else
        skin_instance<THREADS, LAYOUT, VPT, TILE, kAllFast, WT, BOUNDS>(p, sl, pal + size_t(g) * p.pal_stride, stage + buf * kStage,
                                                                   inst0 + g * istep, v0, nvt, cxy, cz, tid, bo);
        buf ^= 1u;
    };

    // 4. the group's instances
    if constexpr (MORPH == kMorphNone || MORPH == kMorphShared) {
        v2f cxy[VPT];
        float cz[VPT];
#pragma unroll
        for (int k = 0; k < VPT; ++k) { cxy[k] = sl[k].pxy; cz[k] = sl[k].pz; }
        for (uint32_t g = 0; g < gcount; ++g) run_instance(g, cxy, cz);
    } else if constexpr (MORPH == kMorphFused1) {
        // vertex_image = 0; for each applied entry: image = image + offset*rate
        // (poser_impl.inl:340-346); coordinate = base + image (:407)
        const float *wl = reinterpret_cast<const float *>(smem + p.w_off);
        v2f cxy[VPT];
        float cz[VPT];
#pragma unroll
        for (int k = 0; k < VPT; ++k) {
            v2f dxy = v2f{0.f, 0.f};
            float dz = 0.f;
            row_consume<F16, BH>(p.entries, sl[k].rb, sl[k].rlen, hd[k], [&](float ox, float oy, float oz, uint32_t slot) {
                const float w = wl[slot];
                if (!(w < kMorphEps)) { dxy = dxy + v2f{ox, oy} * w; dz = dz + oz * w; }
            });
            cxy[k] = sl[k].pxy + dxy; cz[k] = sl[k].pz + dz;
            // the morphed positions are kept (sorted order) for later calls that declare the rates unchanged; the record of
            // which rates `morphed` belongs to (morph_apply_kernel) no longer holds
            if (k == 0 && grp == 0 && tile == 0 && tid == 0 && p.morphed && p.morph_seen) p.morph_seen[kSeenValid] = 0u;
            if (grp == 0 && p.morphed && sl[k].act) {
                float *mo = p.morphed + (size_t(v0) + uint32_t(tid) + uint32_t(k) * THREADS) * 3;
                mo[0] = cxy[k].x; mo[1] = cxy[k].y; mo[2] = cz[k];
            }
        }
        // the group's instances: one for a single-model frame; for a crowd with a shared facial state every workgroup
        // repeats its tile's short walk (the table stays in its XCD's L2) instead of waiting for a separate morph pass
        for (uint32_t g = 0; g < gcount; ++g) run_instance(g, cxy, cz);
    } else {
        // Slot weights of kQuads instance quads live in LDS at a time (kQuads x (NS+1) x float4): one pass over
        // a vertex's morph row then serves 4*kQuads instances, so the table is walked (and its L2 latency paid)
        // that much less often.  One slot per lane (512 threads) has the registers for two quads; two slots per
        // lane do not (a third wave per SIMD is worth more there: measured).  The accumulators pair x with y of ONE instance; pairing two
        // instances per component instead (three packed multiply-adds per entry and instance pair, a quarter fewer
        // instructions) measured 10 % slower: v_pk_mul_f32 / v_pk_add_f32 occupy the SIMD for two passes, so the
        // arithmetic time is the same and the position fix-up comes on top.
        float4 *wq = reinterpret_cast<float4 *>(smem + p.w_off);
        // The first pack's weights were staged during the set-up.  When one float4 per thread covers a pack's weights,
        // the NEXT pack's are fetched into a register before this pack's instances are skinned and reach LDS after
        // them: their load round trip is hidden and one barrier separates the packs.  (Otherwise: staged between the
        // packs.)
        // (The head of the next pack's walk is NOT requested in front of a pack's last stores, as pack_kernel does: here it costs
        // 144 VGPRs instead of 118 (f32), i.e. one workgroup per CU instead of two, and could hide the first round trip only --
        // every later request of the walk still queues behind those stores.  LAB_NOTES R4.2.)
        const bool wreg = wcount <= uint32_t(THREADS);
        for (uint32_t g0 = 0; g0 < gcount;) {       // (the pack loop continues only behind a whole pack that another follows)
            v2f dxy[VPT][kPack];
            float dz[VPT][kPack];
#pragma unroll
            for (int k = 0; k < VPT; ++k) {
#pragma unroll
                for (int j = 0; j < kPack; ++j) { dxy[k][j] = v2f{0.f, 0.f}; dz[k][j] = 0.f; }
                auto weights = [&](uint32_t slot, float (&w)[kPack]) {
                    const float4 a4 = wq[slot];
                    w[0] = a4.x; w[1] = a4.y; w[2] = a4.z; w[3] = a4.w;
                    if constexpr (kQuads == 2) {
                        const float4 b4 = wq[wstride + slot];
                        w[4] = b4.x; w[5] = b4.y; w[6] = b4.z; w[7] = b4.w;
                    }
                };
                auto walk = [&](auto body) { fused4_walk<F16, !TILE>(p.entries, sl[k].rb, sl[k].rlen, body); };
#ifdef FUSED4_SKIP_WALK       // timing diagnostic only (wrong results): this kernel without its walk
                if (false) {
#else
                if (p.finite_offsets) {
#endif
                    // A skipped slot carries w = +0 exactly (flatten_kernel) and a running sum that
                    // started at +0 can never be -0, so with FINITE offsets "image + offset*0" leaves
                    // the image bit-for-bit unchanged: the skip needs no branch.
                    walk([&](float ox, float oy, float oz, uint32_t slot) {
                        float w[kPack];
                        weights(slot, w);
                        const v2f oxy = v2f{ox, oy};
                        // z of two instances per packed instruction: (dz_j, dz_j+1) += (oz, oz) * (w_j, w_j+1) -- the weights of
                        // an instance quad arrive as such pairs, and each half is the same IEEE mul / add as one at a time
                        // (round 3: -2 % config 5 x 64, -1.5 % config 2 x 64, config 3' even; profiles/r03/walk_zpair_ab.txt)
                        const v2f ozz = v2f{oz, oz};
#pragma unroll
                        for (int j = 0; j < kPack; j += 2) {
                            dxy[k][j] += oxy * w[j]; dxy[k][j + 1] += oxy * w[j + 1];
                            const v2f zz = v2f{dz[k][j], dz[k][j + 1]} + ozz * v2f{w[j], w[j + 1]};
                            dz[k][j] = zz.x; dz[k][j + 1] = zz.y;
                        }
                    });
                } else {
#ifndef FUSED4_SKIP_WALK
                    walk([&](float ox, float oy, float oz, uint32_t slot) {
                        float w[kPack];
                        weights(slot, w);
                        const v2f oxy = v2f{ox, oy};
#pragma unroll
                        for (int j = 0; j < kPack; ++j)
                            if (!(w[j] < kMorphEps)) { dxy[k][j] += oxy * w[j]; dz[k][j] += oz * w[j]; }
                    });
#endif
                }
            }
            const bool more = g0 + kPack < gcount;
            float4 wnext = make_float4(0.f, 0.f, 0.f, 0.f);
            if (more && wreg && uint32_t(tid) < wcount) wnext = pack_weight(g0 + kPack, uint32_t(tid));
            auto one = [&](int j) {
                v2f cxy[VPT];
                float cz[VPT];
#pragma unroll
                for (int k = 0; k < VPT; ++k) {
                    cxy[k] = sl[k].pxy + dxy[k][j]; cz[k] = sl[k].pz + dz[k][j];
                }
                run_instance(g0 + j, cxy, cz);
            };
#pragma unroll
            for (int j = 0; j + 1 < kPack; ++j)
                if (g0 + j < gcount) one(j);
            if (!more) {
                if (g0 + kPack - 1 < gcount) one(kPack - 1);
                break;
            }
            one(kPack - 1);
            {
                // every wave has left this pack's walk (it passed the barriers of the pack's instances): the weights can
                // be replaced; one barrier before the next walk reads them.  Tile-order outputs have no per-instance barrier
                // (skin_instance returns before it), so there a wave with short morph rows could get here while another is
                // still reading this pack's weights: one barrier per pack closes the walk explicitly.
                if constexpr (TILE) __syncthreads();
                if (wreg) {
                    if (uint32_t(tid) < wcount) wq[tid] = wnext;
                } else {
                    for (uint32_t i = tid; i < wcount; i += THREADS) wq[i] = pack_weight(g0 + kPack, i);
                }
                __syncthreads();
            }
            g0 += kPack;
        }
    }
    };   // instances
    // (the one-set-of-rates kernel keeps ONE instantiation: two cost it 30 VGPRs -- 98 -> 130 -- and with them its second
    // workgroup per CU: config 5, one frame, 14.9 -> 19.7 us)
    if constexpr (MORPH == kMorphFused1) {
        instances(std::false_type{});
    } else {
        if (all_fast) instances(std::true_type{});
        else instances(std::false_type{});
    }
}

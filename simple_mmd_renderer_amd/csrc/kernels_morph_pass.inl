// kernels_morph_pass.inl -- the shared morph pass (morph_apply_kernel: the morphed positions of a crowd with one facial state, once
// per call) and the group-morph flattening (flatten_kernel and its select form: rates -> slot weights).
// A piece of kernels.hip (included inside namespace mmdx { namespace {): the pass is compiled plain and fast-math, the flatten
// kernels in the bit-exact build only.

// ---- shared morph pass: morphed[gs] = base[gs] + sum(offset*rate), once per call ------------------
// FUSED_FLATTEN: every workgroup first evaluates the group-morph chains of all slots into LDS
// (UpdateMorphTransform's recursion; NS is a few hundred), saving the separate flatten launch.
template <bool F16, bool FUSED_FLATTEN>
__global__ __launch_bounds__(kThreads) void morph_apply_kernel(const DeformParams p,
                                                               const FlattenParams f) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ uint32_t last_block;
    const float *wsl = p.wslot;
    bool walk = true;
    if constexpr (FUSED_FLATTEN) {
        // vertex_images_ depends on morph_rates_ only (poser_impl.inl:362-386): when this call's rates are, bit for bit, the ones
        // `morphed` was last computed from (f.seen, written by the last workgroup of that launch), there is nothing to do.
        if (f.seen) {
            bool same = f.seen[kSeenValid] == 1u;
            for (uint32_t m = threadIdx.x; m < f.nm; m += kThreads) same = same && __float_as_uint(f.rates[m]) == f.seen[kSeenRates + m];
            walk = __syncthreads_and(same) == 0;
        }
        if (walk) {
            float *wl = reinterpret_cast<float *>(smem);
            for (uint32_t s = threadIdx.x; s <= f.ns; s += kThreads)     // slot ns = padding, weight 0
                wl[s] = s < f.ns ? slot_weight(f.rates, f.slot_top, f.chain_off, f.chain_rate, s) : 0.f;
            __syncthreads();
            wsl = wl;
        }
    }
    const size_t gs = size_t(blockIdx.x) * kThreads + threadIdx.x;
    if (walk && gs < p.nv) {
        float bx, by, bz;
        if constexpr (F16) {
            const uint2 r = reinterpret_cast<const uint2 *>(p.spos)[gs];
            bx = h2f(r.x & 0xffffu); by = h2f(r.x >> 16); bz = h2f(r.y & 0xffffu);
        } else {
            const float *sp = reinterpret_cast<const float *>(p.spos) + gs * 3;
            bx = sp[0]; by = sp[1]; bz = sp[2];
        }
        v2f dxy = v2f{0.f, 0.f};
        float dz = 0.f;
        const uint2 sl2 = p.ell[gs >> 6];
        // a thread of this pass has nothing else in its registers: 16 entries in flight cover most rows in one round trip
        for_row<F16, 16>(p.entries, sl2.x + uint32_t(gs & 63), sl2.y, [&](float ox, float oy, float oz, uint32_t slot) {
            const float w = wsl[slot];
            if (!(w < kMorphEps)) { dxy = dxy + v2f{ox, oy} * w; dz = dz + oz * w; }
        });
        p.morphed[gs * 3] = bx + dxy.x;
        p.morphed[gs * 3 + 1] = by + dxy.y;
        p.morphed[gs * 3 + 2] = bz + dz;
    }
    if constexpr (FUSED_FLATTEN) {
        // The workgroup that finishes LAST records the rates (every other one has compared by then: its ticket comes after its
        // reads), so no workgroup ever compares against a half-written record; the next launch on the stream sees it whole.
        if (f.seen) {
            if (threadIdx.x == 0) last_block = atomicAdd(&f.seen[kSeenTicket], 1u) == gridDim.x - 1 ? 1u : 0u;
            __syncthreads();
            if (last_block) {
                for (uint32_t m = threadIdx.x; m < f.nm; m += kThreads) f.seen[kSeenRates + m] = __float_as_uint(f.rates[m]);
                if (threadIdx.x == 0) {
                    f.seen[kSeenValid] = 1u;
                    f.seen[kSeenTicket] = 0u;
                    f.seen[walk ? kSeenWalks : kSeenSkips] += 1u;
                }
            }
        }
    }
}

#ifndef MMDX_FAST_MATH
// ---- group-morph flattening on the device (UpdateMorphTransform's recursion, per slot) ------------
// One thread per (output row, slot); output rows have ns+1 columns: column ns is the padding slot of the morph table, always 0.
// Row j holds the slot weights of the instance at position j (instance_list.hpp); padding rows of a quad, positions behind a list's
// count and ids that are no row of the rates are zeros (their instances are never written).
template <class Instances>
__device__ __forceinline__ void flatten_body(const FlattenParams &f, const Instances &sel) {
    const size_t idx = size_t(blockIdx.x) * kThreads + threadIdx.x;
    const uint32_t rows = f.quad ? ((f.niw + 3) / 4) * 4 : f.niw, cols = f.ns + 1;
    if (idx >= size_t(rows) * cols) return;
    const uint32_t j = uint32_t(idx / cols), s = uint32_t(idx - size_t(j) * cols);
    const Lane ln = sel.lane(j, sel.used(f.niw));
    float out = 0.f;
    if (ln.live && s < f.ns) out = slot_weight(f.rates + size_t(ln.row) * f.nm, f.slot_top, f.chain_off, f.chain_rate, s);
    if (f.quad) f.out[(size_t(j / 4) * cols + s) * 4 + (j & 3)] = out;
    else f.out[idx] = out;
}

__global__ __launch_bounds__(kThreads) void flatten_kernel(const FlattenParams f) { flatten_body(f, AllInstances{}); }

// a select launch (mmdx_deform_batched_select): niw = the list's capacity
__global__ __launch_bounds__(kThreads) void flatten_select_kernel(const FlattenParams f) { flatten_body(f, ListedInstances{f.list}); }
#endif  // !MMDX_FAST_MATH

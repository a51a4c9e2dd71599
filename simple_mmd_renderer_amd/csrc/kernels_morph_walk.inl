// kernels_morph_walk.inl -- walks over a lane's row of the sliced-ELL morph table: the batched walk (row_prefetch / row_consume /
// for_row), the rolling window (walk_rolling), the walk of the per-instance-morph mode (fused4_walk), and the slot weight.
// A piece of kernels.hip (included inside namespace mmdx { namespace {), compiled with it, plain and fast-math.

constexpr float kMorphEps = 1e-7f;                // rate < 1e-7 (double) <=> rate < 1e-7f

// One row of the sliced-ELL morph table (plan.cpp): entry j of this lane's row sits at
// base + j*64 (base already includes the lane), `len` is the slice's padded row length and is
// wave-uniform.  Four independent, fully coalesced loads are issued before the first entry is
// consumed; the body still sees the entries one by one, in order, so the rounding sequence is the
// reference's.  Padding entries carry the dummy slot NS whose weight is always 0.
template <bool F16>
struct RawEntry { using type = float4; };
template <>
struct RawEntry<true> { using type = uint2; };

constexpr uint32_t kRowAhead = 4;   // entries in flight per lane in the deform kernels; deeper (8) costs the fused kernels a wave per
                                    // SIMD and loses: measured.  The stand-alone morph pass has the registers for 16.

template <bool F16, uint32_t B = kRowAhead>
struct RowHead {                    // the first B entries of a row, loaded ahead of their use
    typename RawEntry<F16>::type e[B];
};
// Entry j of a row sits at byte (base + j*64) * sizeof(entry) of the table: a wave-uniform 64-bit base plus a 32-bit
// per-lane offset (plan.cpp keeps the table under 4 GiB), so a lane carries one address register, not a pointer pair.
template <bool F16>
__device__ __forceinline__ typename RawEntry<F16>::type row_entry(const void *entries, uint32_t base, uint32_t j) {
    using Raw = typename RawEntry<F16>::type;
    const uint32_t off = (base + j * 64u) * uint32_t(sizeof(Raw));
    return *reinterpret_cast<const Raw *>(static_cast<const unsigned char *>(entries) + off);
}
template <bool F16, uint32_t B = kRowAhead>
__device__ __forceinline__ void row_prefetch(const void *entries, uint32_t base, uint32_t len, RowHead<F16, B> &h) {
    using Raw = typename RawEntry<F16>::type;
    const uint32_t last = len ? len - 1 : 0u;
    // every element is (re)defined on every path, so that a head requested for the next pack is not kept alive
    // across the code in front of the request
#pragma unroll
    for (uint32_t i = 0; i < B; ++i) {
        Raw v = Raw{};
        if (len) v = row_entry<F16>(entries, base, min(i, last));
        h.e[i] = v;
    }
}
template <bool F16, uint32_t B = kRowAhead, typename Body>
__device__ __forceinline__ void row_consume(const void *entries, uint32_t base, uint32_t len, const RowHead<F16, B> &h,
                                            Body body) {
    using Raw = typename RawEntry<F16>::type;
    auto apply = [&](const Raw r) {
        if constexpr (F16) {
            body(h2f(r.x & 0xffffu), h2f(r.x >> 16), h2f(r.y & 0xffffu), uint32_t(r.y >> 16));
        } else {
            body(r.x, r.y, r.z, __float_as_uint(r.w));
        }
    };
    // software-pipelined: the next B entries are in flight while the current B are consumed (the
    // gather is a chain of L2 round trips; with ~3 resident waves per SIMD nothing else hides them)
    if (len == 0) return;
    const uint32_t last = len - 1;
    Raw cur[B], nxt[B];
#pragma unroll
    for (uint32_t i = 0; i < B; ++i) cur[i] = h.e[i];
    for (uint32_t j = 0; j < len; j += B) {
#pragma unroll
        for (uint32_t i = 0; i < B; ++i) nxt[i] = cur[i];
        if (j + B < len) {
#pragma unroll
            for (uint32_t i = 0; i < B; ++i) nxt[i] = row_entry<F16>(entries, base, min(j + B + i, last));
        }
#pragma unroll
        for (uint32_t i = 0; i < B; ++i)
            if (i == 0 || j + i < len) apply(cur[i]);
#pragma unroll
        for (uint32_t i = 0; i < B; ++i) cur[i] = nxt[i];
    }
}
template <bool F16, uint32_t B = kRowAhead, typename Body>
__device__ __forceinline__ void for_row(const void *entries, uint32_t base, uint32_t len, Body body) {
    RowHead<F16, B> h;
    row_prefetch<F16, B>(entries, base, len, h);
    row_consume<F16, B>(entries, base, len, h, body);
}

// The same walk through a ROLLING window (round 4): entry j+D is requested as soon as entry j has been consumed -- D loads in
// flight in ONE register set (row_consume keeps a current and a next batch, 2 x 4 entries, and copies one into the other), and the
// steady-state loop has no branch in its body (a refill past the row's end re-reads the last entry, which is never applied
// twice), so the compiler counts the loads in flight and waits for exactly the oldest one instead of draining the queue at
// every batch.  `len` must be wave-uniform (a scalar: the slice's padded length).
constexpr uint32_t kWalkDepth32 = 4;        // entries in flight per lane, f32 table (16-byte entries: 4 registers each)
constexpr uint32_t kWalkDepth16 = 4;        // ... f16 table (8-byte entries: 2 registers each)
// (Head and walk stay two functions: written as one, with one `last` for both, the 48 per-instance-morph kernels that walk this way
// compile to other instructions -- profiles/kernels_split/README.md.)
template <bool F16>
struct WalkHead {                   // the first D entries of a row, requested ahead of the walk that consumes them
    static constexpr uint32_t D = F16 ? kWalkDepth16 : kWalkDepth32;
    typename RawEntry<F16>::type e[D];
};
template <bool F16>
__device__ __forceinline__ void walk_head(const void *entries, uint32_t base, uint32_t len, WalkHead<F16> &h) {
    using Raw = typename RawEntry<F16>::type;
    const uint32_t last = len ? len - 1 : 0u;
#pragma unroll
    for (uint32_t i = 0; i < WalkHead<F16>::D; ++i) h.e[i] = len ? row_entry<F16>(entries, base, min(i, last)) : Raw{};
}
template <bool F16, typename Body>
__device__ __forceinline__ void walk_from_head(const void *entries, uint32_t base, uint32_t len, WalkHead<F16> &h, Body body) {
    using Raw = typename RawEntry<F16>::type;
    constexpr uint32_t D = WalkHead<F16>::D;
    if (len == 0) return;
    auto apply = [&](const Raw r) {
        if constexpr (F16) body(h2f(r.x & 0xffffu), h2f(r.x >> 16), h2f(r.y & 0xffffu), uint32_t(r.y >> 16));
        else body(r.x, r.y, r.z, __float_as_uint(r.w));
    };
    const uint32_t last = len - 1;
    uint32_t j = 0;
    for (; j + D < len; j += D) {
#pragma unroll
        for (uint32_t i = 0; i < D; ++i) {
            apply(h.e[i]);
            h.e[i] = row_entry<F16>(entries, base, min(j + D + i, last));
        }
    }
#pragma unroll
    for (uint32_t i = 0; i < D; ++i)
        if (i == 0 || j + i < len) apply(h.e[i]);
}
template <bool F16, typename Body>
__device__ __forceinline__ void walk_rolling(const void *entries, uint32_t base, uint32_t len, Body body) {
    WalkHead<F16> h;
    walk_head<F16>(entries, base, len, h);
    walk_from_head<F16>(entries, base, len, h, body);
}

// Group-morph recursion of one slot (UpdateMorphTransform, poser_impl.inl:328-339): rate[top] times the
// nested groups' sub-rates, with the `< 1e-7` skip after every factor; a skipped slot weighs 0.
__device__ __forceinline__ float slot_weight(const float *rates, const uint32_t *slot_top,
                                             const uint32_t *chain_off, const float *chain_rate,
                                             uint32_t s) {
    float r = rates[slot_top[s]];
    bool skip = r < kMorphEps;
    for (uint32_t c = chain_off[s]; !skip && c < chain_off[s + 1]; ++c) {
        r = chain_rate[c] * r;
        skip = r < kMorphEps;
    }
    return skip ? 0.f : r;
}

// The walk of the per-instance-morph mode: the rolling window (LAB_NOTES R4.2), or the batched walk for tile-order outputs
// (ROLLING = false).  A sorted slot's row length is the same for the 64 lanes of its wave (one slice), lanes past the tile's end
// included or all of them 0.
template <bool F16, bool ROLLING, typename Body>
__device__ __forceinline__ void fused4_walk(const void *entries, uint32_t rb, uint32_t rlen, Body body) {
    if constexpr (ROLLING) walk_rolling<F16>(entries, rb, __builtin_amdgcn_readfirstlane(rlen), body);
    else for_row<F16>(entries, rb, rlen, body);
}

// kernels_store.inl -- the output stores of the deform kernels and the cooperative copy of an LDS image to global memory.
// A piece of kernels.hip (included inside namespace mmdx { namespace {), compiled with it, plain and fast-math.

// ---- cache policy of the OUTPUT stores ------------------------------------------------------------------------------------------
// 98.7 % of the crowd kernel's HBM bytes are write-once stores, and they carry the `nt` (non-temporal) hint: measured interleaved on
// the same arrays against plain stores, whose lines stay in the XCD's L2 until evicted (profiles/r03/store_policy_*.txt; LAB_NOTES
// R3.1), nt takes the crowd kernel from 218.7 to 206.2 us (fast placement; 264 -> 253 on a slow one), the 32-byte-vertex crowd
// from 271 to 246, config 3' from 382 to 341, config 5 x 64 from 144 to 136.  Compiler-visible stores, bit-identical results.
// The write-through flavour (`sc1 nt`) exists ONLY as the buffer-store builtin of CopyFast below: round 3's inline-asm `sc1`
// flavours were invisible to the hazard recogniser and corrupted results -- removed.
typedef float v4f __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void store16(float4 *dst, const float4 v) {
    __builtin_nontemporal_store(v4f{v.x, v.y, v.z, v.w}, reinterpret_cast<v4f *>(dst));
}
// three consecutive floats (tile-order direct stores: 12-byte vertices, so no 16-byte alignment to promise)
__device__ __forceinline__ void store3(float *dst, float x, float y, float z) {
    __builtin_nontemporal_store(x, dst); __builtin_nontemporal_store(y, dst + 1); __builtin_nontemporal_store(z, dst + 2);
}
template <typename T>
__device__ __forceinline__ void store_elem(T *dst, const T v) {      // scalar pieces (ragged tiles, direct stores)
    __builtin_nontemporal_store(v, dst);
}

// ---- cooperative copy of LDS images to global, 16-byte stores where whole chunks fit -------------
// An image mirrors global memory from the 16-byte boundary below element `base`:
// LDS element (shift + i) <-> out[base + i], shift = base % (16/sizeof(T)).
template <typename T>
__device__ __forceinline__ void copy_chunk(const unsigned char *img, T *g, uint32_t q, uint32_t shift,
                                           uint32_t n, bool aligned16) {
    constexpr uint32_t EPC = 16 / sizeof(T);
    const uint32_t lo = q * EPC;
    if (aligned16 && lo >= shift && lo + EPC <= shift + n) {
        const float4 v = *reinterpret_cast<const float4 *>(img + size_t(q) * 16);
        store16(reinterpret_cast<float4 *>(g + lo), v);
    } else {
        const T *l = reinterpret_cast<const T *>(img);
#pragma unroll
        for (uint32_t e = 0; e < EPC; ++e) {
            const uint32_t i = lo + e;
            if (i >= shift && i < shift + n) store_elem(g + i, l[i]);
        }
    }
}

// two images (A then B) in one pass over the workgroup's threads
template <int THREADS, typename TA, typename TB>
__device__ __forceinline__ void copy_out2(const unsigned char *imgA, TA *outA, size_t baseA,
                                          uint32_t shA, uint32_t nA, const unsigned char *imgB,
                                          TB *outB, size_t baseB, uint32_t shB, uint32_t nB,
                                          bool aligned16, int tid) {
    const uint32_t ncA = (shA + nA + 16 / sizeof(TA) - 1) / (16 / sizeof(TA));
    const uint32_t ncB = (shB + nB + 16 / sizeof(TB) - 1) / (16 / sizeof(TB));
    TA *gA = outA + baseA - shA;
    TB *gB = outB + baseB - shB;
    for (uint32_t q = tid; q < ncA + ncB; q += THREADS) {
        if (q < ncA) copy_chunk<TA>(imgA, gA, q, shA, nA, aligned16);
        else copy_chunk<TB>(imgB, gB, q - ncA, shB, nB, aligned16);
    }
}


// Fast path for a FULL tile whose output range starts on a 16-byte boundary (every tile but the last
// when NV % 4 == 0): all LDS reads are issued first, then all stores -- one LDS round trip per
// instance instead of one per chunk, no per-chunk branching.  CA / CB = 16-byte chunks of image A / B;
// image B sits `gapB` bytes after image A in LDS.
// WT (write-through): the 16-byte stores carry `sc1 nt` instead of `nt` -- the line is written through to memory and dropped from
// the XCD's L2.  On output arrays whose physical backing is in the slow store mode (six plain allocations in
// seven) the SoA crowd kernel runs 4.6-5.0 % faster with it (251.6 -> 240.0 us), in the fast mode 2 % slower (207.0 -> 211.4):
// profiles/r03/store_policy_buffer_builtin_ab*.txt -- so the host picks per launch (api.cpp).  Issued through the buffer-store
// builtin: the compiler sees the instruction and keeps its data hazards (round 3's inline-asm flavours did not, and corrupted
// results: removed); descriptor = this instance's piece of the array (wave-uniform), lane offset in bytes.
template <int THREADS, int CA, int CB, int I, bool WT = false>
struct CopyFast {
    // step I of ceil((CA+CB)/THREADS): load chunk q = tid + I*THREADS, recurse (so every LDS read is
    // issued before the first store), then store it.  Scalars only -- an indexed float4 array here
    // ends up in scratch memory with a vmcnt(0) in front of every store.
    static __device__ __forceinline__ void run(const unsigned char *img, uint32_t gapB, float4 *outA,
                                               float4 *outB, int tid) {
        constexpr int TOTAL = CA + CB;
        if constexpr (I * THREADS < TOTAL) {
            constexpr bool full = (I + 1) * THREADS <= TOTAL;
            const int q = tid + I * THREADS;
            const bool inA = (I + 1) * THREADS <= CA ? true : (I * THREADS >= CA ? false : q < CA);
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (full || q < TOTAL)
                v = *reinterpret_cast<const float4 *>(img + (inA ? 0u : gapB - uint32_t(CA) * 16u) +
                                                      size_t(q) * 16);
            CopyFast<THREADS, CA, CB, I + 1, WT>::run(img, gapB, outA, outB, tid);
            if (full || q < TOTAL) {
                if constexpr (WT) {
                    typedef unsigned int v4u __attribute__((ext_vector_type(4)));
                    constexpr int kSc1Nt = 2 | 16;                      // cache-policy bits of the buffer intrinsics: nt, sc1
                    const v4u d = {__float_as_uint(v.x), __float_as_uint(v.y), __float_as_uint(v.z), __float_as_uint(v.w)};
                    if (inA) {
                        const __amdgpu_buffer_rsrc_t r = __builtin_amdgcn_make_buffer_rsrc(outA, 0, uint32_t(CA) * 16u, 0x00027000);
                        __builtin_amdgcn_raw_buffer_store_b128(d, r, uint32_t(q) * 16u, 0, kSc1Nt);
                    } else {
                        const __amdgpu_buffer_rsrc_t r = __builtin_amdgcn_make_buffer_rsrc(outB, 0, uint32_t(CB) * 16u, 0x00027000);
                        __builtin_amdgcn_raw_buffer_store_b128(d, r, uint32_t(q - CA) * 16u, 0, kSc1Nt);
                    }
                } else {
                    float4 *dst = inA ? outA + q : outB + (q - CA);
                    store16(dst, v);
                }
            }
        }
    }
};
template <int THREADS, int CA, int CB, bool WT = false>
__device__ __forceinline__ void copy_out_fast(const unsigned char *img, uint32_t gapB, float4 *outA,
                                              float4 *outB, int tid) {
    CopyFast<THREADS, CA, CB, 0, WT>::run(img, gapB, outA, outB, tid);
}

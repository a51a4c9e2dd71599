// kernels_bounds.inl -- per-instance bounds (mmdx_deform_batched_bounds): the NaN-skipping min / max, its reduction over a wave,
// and where deform_kernel<..., BOUNDS> puts an instance's partials.  The kernels that fold the partials: kernels_bounds_reduce.inl
// (they stand behind the other kernels of the bit-exact build, where the code object has always had them).
// A piece of kernels.hip (included inside namespace mmdx { namespace {), compiled with it, plain and fast-math.

// min / max with IEEE minNum / maxNum (v_min_f32 / v_max_f32, IEEE mode): a NaN operand is skipped, so NaN is the identity and a
// component that is NaN everywhere stays NaN; the result is always one of the operands (bit for bit, up to NaN payloads).
template <bool MAX>
__device__ __forceinline__ float bound_op(float a, float b) { return MAX ? fmaxf(a, b) : fminf(a, b); }
// Across lanes the comparison runs on ordered integer keys (signed order of the keys = numeric order of the floats, -0 just below
// +0; key2f(f2key(x)) == x bit for bit): an integer min / max takes its DPP operand directly, where the float one would first have
// to quiet the moved value (a v_max_f32 x, x per step) -- a third of the instructions.
__device__ __forceinline__ int f2key(float x) { const int b = __float_as_int(x); return b ^ ((b >> 31) & 0x7fffffff); }
__device__ __forceinline__ float key2f(int k) { return __int_as_float(k ^ ((k >> 31) & 0x7fffffff)); }
template <bool MAX>
__device__ __forceinline__ int key_op(int a, int b) { return MAX ? max(a, b) : min(a, b); }
template <int CTRL>
__device__ __forceinline__ int dpp_i(int v) { return __builtin_amdgcn_mov_dpp(v, CTRL, 0xf, 0xf, false); }
// one DPP step of the six keys at once (independent chains: they fill each other's DPP wait states)
template <int CTRL>
__device__ __forceinline__ void dpp_step6(int (&k)[6]) {
#pragma unroll
    for (int c = 0; c < 6; ++c) k[c] = c < 3 ? key_op<false>(k[c], dpp_i<CTRL>(k[c])) : key_op<true>(k[c], dpp_i<CTRL>(k[c]));
}
// Lane c < 6 of the calling wave gets component c of {min x, min y, min z, max x, max y, max z} over the wave's lanes, NaN lanes
// skipped (NaN when every lane holds NaN): four DPP steps inside each row of 16 lanes (none of them reads outside its row), then
// the four row results through readlane.
__device__ __forceinline__ float wave_bounds6(const float (&mn)[3], const float (&mx)[3], uint32_t lane) {
    int k[6];
#pragma unroll
    for (int c = 0; c < 3; ++c) {                           // a NaN lane's key loses against every value
        k[c] = mn[c] != mn[c] ? INT_MAX : f2key(mn[c]);
        k[3 + c] = mx[c] != mx[c] ? INT_MIN : f2key(mx[c]);
    }
    dpp_step6<0xb1>(k);        // quad_perm [1,0,3,2]
    dpp_step6<0x4e>(k);        // quad_perm [2,3,0,1]
    dpp_step6<0x141>(k);       // row_half_mirror
    dpp_step6<0x140>(k);       // row_mirror: every lane of a row holds the row's result
    int r[6];
#pragma unroll
    for (int c = 0; c < 6; ++c) {
        const int a = __builtin_amdgcn_readlane(k[c], 0), b = __builtin_amdgcn_readlane(k[c], 16);
        const int d = __builtin_amdgcn_readlane(k[c], 32), e = __builtin_amdgcn_readlane(k[c], 48);
        r[c] = c < 3 ? key_op<false>(key_op<false>(a, b), key_op<false>(d, e)) : key_op<true>(key_op<true>(a, b), key_op<true>(d, e));
    }
    const int s = lane == 0 ? r[0] : lane == 1 ? r[1] : lane == 2 ? r[2] : lane == 3 ? r[3] : lane == 4 ? r[4] : r[5];
    return s == (lane < 3 ? INT_MAX : INT_MIN) ? __builtin_nanf("") : key2f(s);
}

// Where one instance's bounds go in a bounds launch: `lds` = the combine words of the instance's image parity (image path: one
// group of 6 per wave), `out` = its partial(s) in p.bounds -- one group of 6 per tile, or per wave of a tile for tile-order outputs.
struct BoundsOut {
    float *lds;
    float *out;
};

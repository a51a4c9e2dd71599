// pbounds_kernels.hip -- mmdx_palette_bounds on gfx950: a conservative box per instance from the palette and the model's bone-box
// table (include/mmdx.h states the arithmetic; pbounds_math.hpp holds it, shared with the CPU driver of the tests; this file is built
// with -ffp-contract=off like the rest, and models created with MMDX_CREATE_FAST_MATH run this same kernel).
//
// one lane per (instance, table row)   a lane loads its table row (three 16-byte loads from a table of a few KB that every instance
//                           reads: it stays in L2) and columns 0..2 of its bone's matrix (four 16-byte loads, the only HBM traffic:
//                           the palette is read once), transforms the row's box and pads it.  Tables longer than the instance's lanes
//                           are folded in registers, on ordered integer keys.
// WPI = 4 (one instance per workgroup)  tables of more than 64 rows.  The wave reduces its six keys with four DPP steps inside each
//                           row of 16 lanes and readlane across the four rows (the pattern of the deform kernels' bounds flavour);
//                           the four waves meet in 128 bytes of LDS behind ONE barrier; lane 0 stores the row.
// WPI = 1 (four instances per workgroup) tables of at most 64 rows.  A 256-lane workgroup would idle three waves in four and still
//                           pay the barrier; here a wave is an instance, nothing is shared, no LDS, no barrier, and a workgroup
//                           keeps the 256 lanes the CU schedules best.  Between 65 and 255 rows the WPI = 4 form idles lanes too, but
//                           idle lanes request no memory, and the kernel's time is its palette read.
// No atomics, no initialisation launch, no workgroup waits for another: the result is the integer min / max of the keys, whatever
// the reduction tree.
#include <hip/hip_runtime.h>

#include "pbounds_kernels.hpp"
#include "pbounds_math.hpp"

namespace mmdx {

namespace {

template <int CTRL>
__device__ __forceinline__ int dpp_i(int v) { return __builtin_amdgcn_mov_dpp(v, CTRL, 0xf, 0xf, false); }
// one DPP step of the six keys at once (independent chains: they fill each other's DPP wait states)
template <int CTRL>
__device__ __forceinline__ void dpp_step6(int (&k)[6]) {
#pragma unroll
    for (int c = 0; c < 6; ++c) k[c] = c < 3 ? min(k[c], dpp_i<CTRL>(k[c])) : max(k[c], dpp_i<CTRL>(k[c]));
}
// The wave's fold of the six keys, in every lane (wave-uniform values).  Every lane of the wave is active here.
__device__ __forceinline__ void wave_fold6(int (&k)[6]) {
    dpp_step6<0xb1>(k);        // quad_perm [1,0,3,2]
    dpp_step6<0x4e>(k);        // quad_perm [2,3,0,1]
    dpp_step6<0x141>(k);       // row_half_mirror
    dpp_step6<0x140>(k);       // row_mirror: every lane of a row of 16 holds the row's result
#pragma unroll
    for (int c = 0; c < 6; ++c) {
        const int a = __builtin_amdgcn_readlane(k[c], 0), b = __builtin_amdgcn_readlane(k[c], 16);
        const int d = __builtin_amdgcn_readlane(k[c], 32), e = __builtin_amdgcn_readlane(k[c], 48);
        k[c] = c < 3 ? min(min(a, b), min(d, e)) : max(max(a, b), max(d, e));
    }
}

__device__ __forceinline__ void store_row(float *__restrict__ out, uint32_t i, const int (&k)[6], bool nan_or_empty, float pos_scale) {
    float o[6];
    pbounds_finish(k, k + 3, nan_or_empty, pos_scale, o);
    float *row = out + size_t(i) * 6;
#pragma unroll
    for (int c = 0; c < 6; ++c) row[c] = o[c];
}

template <int WPI>
__global__ __launch_bounds__(kPBoundsThreads) void palette_bounds_kernel(const float4 *__restrict__ palettes, const float4 *__restrict__ table,
                                                                         float *__restrict__ out, uint32_t ni, uint32_t nb, uint32_t n_boxes,
                                                                         float eps, float morph_scale, float pos_scale) {
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t i = WPI == 1 ? blockIdx.x * 4 + wave : blockIdx.x;
    if (WPI == 1 && i >= ni) return;                    // wave-uniform; this form has no barrier
    const float4 *P = palettes + size_t(i) * nb * 4;
    PBoundsAcc acc;
    pbounds_init(acc);
    for (uint32_t r = WPI == 1 ? lane : tid; r < n_boxes; r += WPI * 64) {
        const float4 *t = table + size_t(r) * 3;
        const float4 t0 = t[0], t1 = t[1], t2 = t[2];
        const float4 *M = P + size_t(__float_as_uint(t0.w)) * 4;
        const float4 r0 = M[0], r1 = M[1], r2 = M[2], r3 = M[3];
        const float lo[3] = {t0.x, t0.y, t0.z}, hi[3] = {t1.x, t1.y, t1.z}, reach[3] = {t2.x, t2.y, t2.z};
        const float m[16] = {r0.x, r0.y, r0.z, 0.0f, r1.x, r1.y, r1.z, 0.0f, r2.x, r2.y, r2.z, 0.0f, r3.x, r3.y, r3.z, 0.0f};
        float blo[3], bhi[3];
        pbounds_row(lo, hi, reach, morph_scale, m, eps, blo, bhi);
        pbounds_fold(acc, blo, bhi);
    }
    int k[6] = {acc.kmin[0], acc.kmin[1], acc.kmin[2], acc.kmax[0], acc.kmax[1], acc.kmax[2]};
    wave_fold6(k);
    const bool nan = __ballot(acc.nan) != 0ull;
    if constexpr (WPI == 1) {
        if (lane == 0) store_row(out, i, k, nan || n_boxes == 0, pos_scale);
    } else {
        __shared__ int part[WPI][8];
        if (lane == 0) {
#pragma unroll
            for (int c = 0; c < 6; ++c) part[wave][c] = k[c];
            part[wave][6] = nan ? 1 : 0;
        }
        __syncthreads();
        if (tid == 0) {
            bool any = false;
#pragma unroll
            for (int w = 0; w < WPI; ++w) {
#pragma unroll
                for (int c = 0; c < 6; ++c) k[c] = c < 3 ? min(k[c], part[w][c]) : max(k[c], part[w][c]);
                any = any || part[w][6] != 0;
            }
            store_row(out, i, k, any, pos_scale);
        }
    }
}

}  // namespace

hipError_t launch_palette_bounds(const PBoundsLaunch &p, hipStream_t stream) {
    const dim3 grid(pbounds_workgroups(p.ni, p.n_boxes)), block(kPBoundsThreads);
    const float4 *pal = reinterpret_cast<const float4 *>(p.palettes), *tab = reinterpret_cast<const float4 *>(p.table);
    if (pbounds_waves_per_instance(p.n_boxes) == 1)
        hipLaunchKernelGGL(palette_bounds_kernel<1>, grid, block, 0, stream, pal, tab, p.out, p.ni, p.nb, p.n_boxes, p.eps, p.morph_scale,
                           p.pos_scale);
    else
        hipLaunchKernelGGL(palette_bounds_kernel<4>, grid, block, 0, stream, pal, tab, p.out, p.ni, p.nb, p.n_boxes, p.eps, p.morph_scale,
                           p.pos_scale);
    return hipGetLastError();
}

}  // namespace mmdx

// spring_kernels.hip -- mmdx_spring_step on gfx950 (include/mmdx.h states the arithmetic; spring_math.hpp holds it, shared with the
// CPU driver of the tests; this file is built with -ffp-contract=off like the rest).
//
// the lane        (list position, chain): blockIdx.y = chain, 64 consecutive instances (select form: list positions) to a wave, so
//                 the chain, its joints and the colliders are wave-uniform and arrive through scalar loads, and a lane owns every
//                 joint of its chain for its instance: the joints are a dependent loop of at most 32 in registers, the parent's
//                 row handed from one joint to the next.  No barrier, no LDS, no atomics; vector stores only.
// the state       [joint][6][max_instances], instance fastest: the six loads and six stores of a joint are coalesced (256 bytes
//                 per wave each).  It is indexed by the INSTANCE, so a list only permutes lanes.
// the palette     rows move as four 16-byte accesses: the anchor's row once per lane, each collider bone's row once per lane (its
//                 centre is kept in registers, 16 x 3 floats, for every joint of the chain), each joint's row stored once.  Rows of
//                 one instance are NB * 64 bytes from the next instance's, as in every kernel that reads palettes.
// Anchor and collider bones are no joints of any chain (spring_table.hpp refuses that), so no lane reads a row another lane writes;
// the palette pointer is nevertheless not __restrict__: it is read and written.
#include <hip/hip_runtime.h>

#include "spring_kernels.hpp"

namespace mmdx {

namespace {

__device__ __forceinline__ void load_row(const float4 *src, float *r) {
    const float4 a = src[0], b = src[1], c = src[2], d = src[3];
    r[0] = a.x; r[1] = a.y; r[2] = a.z; r[3] = a.w; r[4] = b.x; r[5] = b.y; r[6] = b.z; r[7] = b.w;
    r[8] = c.x; r[9] = c.y; r[10] = c.z; r[11] = c.w; r[12] = d.x; r[13] = d.y; r[14] = d.z; r[15] = d.w;
}

template <bool kSelect>
__global__ __launch_bounds__(kSpringThreads) void spring_step_kernel(const SpringLaunch p, float dt, const float *dt_dev,
                                                                     const InstanceList list, uint32_t cells) {
    if (dt_dev) dt = *dt_dev;
    const uint32_t k = blockIdx.x * kSpringThreads + threadIdx.x;      // < 2^24 + 64
    uint32_t i = k;
    if (kSelect) {
        const ListedInstances li{list};
        const Lane ln = li.lane(k, li.used(cells));
        if (!ln.live) return;
        i = ln.row;
    } else if (k >= p.ni) {
        return;
    }
    if (i >= p.max_instances) return;                                  // (ni <= max_instances: never; the state is not overrun)
    const SpringChain &ch = p.chains[blockIdx.y];
    float4 *pal = reinterpret_cast<float4 *>(p.palettes) + size_t(i) * p.nb * 4;
    float centres[kSpringMaxColliders][4];
#pragma unroll
    for (uint32_t j = 0; j < kSpringMaxColliders; ++j) {
        centres[j][0] = centres[j][1] = centres[j][2] = centres[j][3] = 0.0f;
        if (j < p.nc) {
            const SpringCollider &col = p.colliders[j];
            float s[16];
            load_row(pal + size_t(col.bone) * 4, s);
            const float x[3] = {col.centre[0], col.centre[1], col.centre[2]};
            spring_pt(x, s, centres[j]);
            centres[j][3] = col.r;
        }
    }
    float row[16];
    load_row(pal + size_t(ch.anchor) * 4, row);
    const float g[3] = {p.gravity[0], p.gravity[1], p.gravity[2]};
    const size_t stride = p.max_instances;
    // (Measured: requesting the state of joint j + 1 before joint j is computed and stored changed nothing, 24.8 us against 24.7 at
    // 1 024 instances; a lone wave's time here is the arithmetic it issues, not its loads.  Not kept.)
    for (uint32_t j = 0; j < ch.count; ++j) {
        const SpringJoint &e = p.joints[ch.first + j];
        float *s = p.state + size_t(ch.first + j) * kSpringStateFloats * stride + i;
        float c[3] = {s[0], s[stride], s[2 * stride]}, q[3] = {s[3 * stride], s[4 * stride], s[5 * stride]};
        const float h[3] = {e.h[0], e.h[1], e.h[2]}, t[3] = {e.t[0], e.t[1], e.t[2]};
        spring_joint(row, h, t, c, q, ch.stiffness, ch.drag, ch.gravity_scale, ch.radius, g, dt, p.reset != 0, centres, p.nc);
        s[0] = c[0]; s[stride] = c[1]; s[2 * stride] = c[2];
        s[3 * stride] = q[0]; s[4 * stride] = q[1]; s[5 * stride] = q[2];
        float4 *dst = pal + size_t(e.bone) * 4;
        dst[0] = make_float4(row[0], row[1], row[2], row[3]);
        dst[1] = make_float4(row[4], row[5], row[6], row[7]);
        dst[2] = make_float4(row[8], row[9], row[10], row[11]);
        dst[3] = make_float4(row[12], row[13], row[14], row[15]);
    }
}

}  // namespace

hipError_t launch_spring_step(const SpringLaunch &p, const InstanceList *list, uint32_t cells, float dt, const float *dt_dev,
                              hipStream_t stream) {
    const uint32_t n = list ? cells : p.ni;
    if (!n || !p.n_chains) return hipSuccess;
    const dim3 grid((n + kSpringThreads - 1) / kSpringThreads, p.n_chains), block(kSpringThreads);
    if (list)
        hipLaunchKernelGGL(spring_step_kernel<true>, grid, block, 0, stream, p, dt, dt_dev, *list, cells);
    else
        hipLaunchKernelGGL(spring_step_kernel<false>, grid, block, 0, stream, p, dt, dt_dev, InstanceList{nullptr, nullptr, p.ni}, n);
    return hipGetLastError();
}

}  // namespace mmdx

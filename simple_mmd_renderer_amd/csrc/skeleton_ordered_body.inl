// skeleton_ordered_body.inl -- the ordered solver's workgroup program behind the point where a lane has learnt its instance; included
// by skeleton_ordered_kernel and skeleton_ordered_select_kernel (rig_kernels.hip), which define, each in ONE place:
//   slot        threadIdx.x / kSolveInstances
//   inst        the lane's state cell (solver scratch and bone-morph state, p.ni cells): the instance, or the list position
//   row         its row of the caller's arrays (poses, palettes): the instance, or ids[inst]
//   live        false: the lane skips the work but reaches every barrier
// Text, not a function, and tried: as a __forceinline__ function template this body compiles (gfx950, the project's flags) to
// different code in all six skeleton_ordered*_kernel instantiations, 5-17 of ~11 800 instructions each, and bone_morph_body.inl as a
// function adds one instruction to both bone-morph kernels.  The solver is register-bound (256 VGPRs dense, spills plain) and takes
// milliseconds, so a tidy-up would mean re-measuring it; as text the plain kernel stays the kernel it was before there was a select
// form (tools/disassembly_diff.py) and the select form cannot drift from it.  The track and FK kernels, which are not register-bound,
// do share their bodies as functions (clip_source.hpp, instance_list.hpp).
    const State st = {p.state + (live ? inst : 0), p.ni};
    extern __shared__ float chain_lds[];   // (windows x instances) lanes x window_floats of state, then the
                                           // windows' link constants
    // Which event of a round this slot runs: the events are dealt over the WAVES first (slot 4w + k runs event 4k + w), so that
    // a round's IK solves -- the first events of the round -- sit in different waves as far as possible: lanes of one wave that
    // solve DIFFERENT chains take turns through every divergent piece of the CCD loop (two chains per wave instead of four on the
    // bench rig: measured).  The LDS windows belong to the round's first p.windows events, whichever slot runs them.
    constexpr uint32_t kSlotsPerWave = 64 / kSolveInstances, kSolveWaves = kSolveSlots / kSlotsPerWave;
    const uint32_t ev = (slot % kSlotsPerWave) * kSolveWaves + slot / kSlotsPerWave;
    const uint32_t wf = window_floats(p.fast_slots);
    auto *lds_lane = (__attribute__((address_space(3))) float *)chain_lds + (ev * kSolveInstances + threadIdx.x % kSolveInstances) * wf;
    auto *lds_consts = (__attribute__((address_space(3))) float *)chain_lds +
                       size_t(p.windows) * kSolveInstances * wf + ev * (kMaxFastLinks * kLinkConstFloats);
    const float4 *pose = reinterpret_cast<const float4 *>(p.poses) + size_t(live ? row : 0) * p.nb * 2;
    if (live && (p.passes & 1u) && (p.seg_flags & 1u)) {
        for (uint32_t b = slot; b < p.nb; b += kSolveSlots) {   // PrePhysicsPosing's reset, poser_impl.inl:366-377
            st.set_quat(b, kStTotalRot, q_identity());
            st.set_quat(b, kStIkRot, q_identity());
            st.set_quat(b, kStPreIkRot, q_identity());
            st.at(b, kStTotalTr + 0) = 0.f; st.at(b, kStTotalTr + 1) = 0.f; st.at(b, kStTotalTr + 2) = 0.f;
#pragma unroll
            for (int k = 0; k < 16; ++k) st.at(b, kStLocal + k) = (k % 5 == 0) ? 1.f : 0.f;
        }
    }
    __syncthreads();
    float4 *out = reinterpret_cast<float4 *>(p.out) + size_t(live ? row : 0) * p.nb * 4;
    for (uint32_t pass = 0; pass < 2; ++pass) {
        if (!(p.passes >> pass & 1u)) continue;              // the physics seam runs the two lists as two launches
        const uint32_t r0 = max(pass ? p.n_rounds_pre : 0u, p.seg_r0), r1 = min(pass ? p.n_rounds : p.n_rounds_pre, p.seg_r1);
        for (uint32_t r = r0; r < r1; ++r) {
            const RoundRec rr = p.rounds[r];
            if (live && ev < rr.count) {
                const uint32_t b = p.events[rr.first + ev];
                transform_bone(st, p, pose, inst, b);
                if (p.bones[b].bits & kBoneHasIk) solve_ik<NESTED>(st, p, pose, inst, b, lds_lane, lds_consts);
            }
            __syncthreads();
        }
        const uint32_t s0 = pass ? p.n_pre : 0, s1 = pass ? p.nb : p.n_pre;
        if (live && (p.seg_flags >> (1 + pass) & 1u)) {
            for (uint32_t s = s0 + slot; s < s1; s += kSolveSlots) {   // UpdateBoneSkinningMatrix of this list
                const uint32_t b = p.order[s];
                const BoneRec rec = p.bones[b];
                Mat4 G;
#pragma unroll
                for (int y = 0; y < 4; ++y)
#pragma unroll
                    for (int x = 0; x < 4; ++x) G.m[y][x] = x == y ? 1.f : 0.f;
                G.m[3][0] = rec.neg_rest[0]; G.m[3][1] = rec.neg_rest[1]; G.m[3][2] = rec.neg_rest[2];
                const Mat4 S = mul(G, st.local(b));
#pragma unroll
                for (int y = 0; y < 4; ++y) out[4 * size_t(b) + y] = make_float4(S.m[y][0], S.m[y][1], S.m[y][2], S.m[y][3]);
            }
        }
        __syncthreads();                                     // the second list's IK may rewrite these bones
    }

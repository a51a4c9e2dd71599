// ik_coop_body.inl -- one sixteen-lane CCD-IK solve behind the point where the group has learnt its instance; included by ik_coop_kernel
// and ik_coop_select_kernel (rig_kernels.hip), which define, each in ONE place: rr, ev (the round and which IK bone of it), solve, sub
// (the group of the block, the lane of the group), `inst` (the group's state cell: the instance, or the list position) and `row` (its
// pose row: the instance, or ids[inst]); dead groups have left.  Text, not a function, for the reason skeleton_ordered_body.inl gives.
    const State st = {p.state + inst, p.ni};
    const float4 *pose = reinterpret_cast<const float4 *>(p.poses) + size_t(row) * p.nb * 2;
    auto *win = (__attribute__((address_space(3))) float *)coop_lds + solve * kCoopWindow;
    const ChainState cs = {win, 0};
    const uint32_t b = p.events[rr.first + ev];
    const IkRec ik = p.iks[p.bones[b].ik];
    const LinkRec *links = p.links + ik.link0;
    const uint32_t n = ik.nlinks, tidx = n;
    const int32_t outside = ik.outside_parent;
    const WindowChain ch = {win + kCoopConsts, n, outside >= 0 ? int32_t(n + 1) : -1};
    auto group_sync = [] { __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront"); __builtin_amdgcn_wave_barrier(); };

    // the event's own bone first, as the ordered kernel does (UpdateBoneTransform up to the solve), then the chain into the window
    if (sub == 0) {
        transform_bone(st, p, pose, inst, b);
        win[kCoopMisc + 0] = st.at(b, kStLocal + 12); win[kCoopMisc + 1] = st.at(b, kStLocal + 13); win[kCoopMisc + 2] = st.at(b, kStLocal + 14);
    }
    auto copy = [&](uint32_t slot, uint32_t bone, bool in) {
        for (uint32_t f = sub; f < kSerialStateFloats; f += kCoopLanes) {
            if (in) cs.at(slot, f) = st.at(bone, f); else st.at(bone, f) = cs.at(slot, f);
        }
    };
    for (uint32_t j = 0; j < n; ++j) copy(j, links[j].bone, true);
    copy(n, ik.target, true);
    if (outside >= 0) copy(n + 1, uint32_t(outside), true);
    if (sub < n) {                                             // link constants, as solve_ik lays them out
        const LinkRec lk = links[sub];
        const float *off = p.bones[lk.bone].local_offset;
        auto *c = win + kCoopConsts + sub * kLinkConstFloats;
        c[0] = off[0]; c[1] = off[1]; c[2] = off[2];
        c[3] = __uint_as_float(lk.limited | lk.order << 8 | lk.fix << 16);
        c[4] = lk.lo[0]; c[5] = lk.lo[1]; c[6] = lk.lo[2];
        c[7] = lk.hi[0]; c[8] = lk.hi[1]; c[9] = lk.hi[2];
    }
    group_sync();
    const V3 ik_pos = {win[kCoopMisc + 0], win[kCoopMisc + 1], win[kCoopMisc + 2]};
    const BoneRec trec = p.bones[ik.target];

    // ccd()'s preamble on the window, one lane: the links root-first, the target, the convergence test; then what the loop keeps
    if (sub == 0) {
        for (uint32_t i = 0; i < n; ++i) cs.set_quat(ch.idx(i), kStIkRot, q_identity());
        for (uint32_t i = 0; i < n; ++i) {
            const uint32_t j = n - i - 1, lb = links[j].bone;
            const BoneRec rec = p.bones[lb];
            transform_at(cs, rec, morph_of(p, lb, inst), pose[2 * size_t(lb)], pose[2 * size_t(lb) + 1], ch.idx(j), ch.par(j),
                         uint32_t(rec.append_parent));
        }
        transform_at(cs, trec, morph_of(p, ik.target, inst), pose[2 * size_t(ik.target)], pose[2 * size_t(ik.target) + 1], tidx, 0,
                     uint32_t(trec.append_parent));
        const V3 t0 = {cs.at(tidx, kStLocal + 12), cs.at(tidx, kStLocal + 13), cs.at(tidx, kStLocal + 14)};
        const V3 e0 = {ik_pos.x - t0.x, ik_pos.y - t0.y, ik_pos.z - t0.z};
        win[kCoopMisc + 3] = v_dot(e0, e0) < 1e-7f ? 0.f : 1.f;
        auto pre_parent = [&](uint32_t idx, const float *off, uint32_t at) {       // a bone's local matrix before its parent product
            Mat4 L = q_to_matrix(cs.quat(idx, kStTotalRot));
            L.m[3][0] = cs.at(idx, kStTotalTr + 0) + off[0];
            L.m[3][1] = cs.at(idx, kStTotalTr + 1) + off[1];
            L.m[3][2] = cs.at(idx, kStTotalTr + 2) + off[2];
#pragma unroll
            for (int k = 0; k < 16; ++k) win[at + k] = L.m[k / 4][k % 4];
        };
        for (uint32_t j = 0; j < n; ++j) {
            const V3 off = ch.offset(j);
            const float o[3] = {off.x, off.y, off.z};
            pre_parent(j, o, kCoopLpre + j * 16);
        }
        pre_parent(tidx, trec.local_offset, kCoopTpre);
    }
    group_sync();
    const bool run = win[kCoopMisc + 3] != 0.f;
    if (run) {
        const float tpre = win[kCoopTpre + sub];
        V3 tgt = {cs.at(tidx, kStLocal + 12), cs.at(tidx, kStLocal + 13), cs.at(tidx, kStLocal + 14)};
        const uint32_t ikt = ik.loop / 2;
        for (uint32_t i = 0; i < ik.loop; ++i) {
            bool changed = false;
            for (uint32_t j = 0; j < n; ++j) {
                const LinkInfo lk = ch.link(j);
                if (lk.fix == kFixAll) continue;
                const uint32_t ls = j;
                const int32_t lp = ch.par(j);
                const V3 lpos = {cs.at(ls, kStLocal + 12), cs.at(ls, kStLocal + 13), cs.at(ls, kStLocal + 14)};
                const V3 tdir = v_normalize({lpos.x - tgt.x, lpos.y - tgt.y, lpos.z - tgt.z});
                const V3 idir = v_normalize({lpos.x - ik_pos.x, lpos.y - ik_pos.y, lpos.z - ik_pos.z});
                V3 axis = {tdir.y * idir.z - tdir.z * idir.y, tdir.z * idir.x - tdir.x * idir.z,
                           tdir.x * idir.y - tdir.y * idir.x};
                if (fabsf(axis.x) < 1e-7f) axis.x = 1e-7f;
                if (fabsf(axis.y) < 1e-7f) axis.y = 1e-7f;
                if (fabsf(axis.z) < 1e-7f) axis.z = 1e-7f;
                // the parent's matrix: this lane's element for the product below, the rotation part whole for the axis
                const float loc = lp >= 0 ? cs.at(uint32_t(lp), kStLocal + sub) : (sub % 5u == 0u ? 1.f : 0.f);
                auto L = [&](uint32_t y, uint32_t x) { return lp >= 0 ? cs.at(uint32_t(lp), kStLocal + 4 * y + x) : (x == y ? 1.f : 0.f); };
                if (lk.limited && lk.fix != kFixNone && i < ikt) {
                    const uint32_t row = lk.fix - kFixX;
                    const float d = axis.x * L(row, 0) + axis.y * L(row, 1) + axis.z * L(row, 2);
                    const float sgn = d >= 0.0f ? 1.0f : -1.0f;
                    axis = {row == 0 ? sgn : 0.f, row == 1 ? sgn : 0.f, row == 2 ? sgn : 0.f};
                } else {                                       // rotate(axis, loc.Transpose()).Normalize()
                    const V3 r = {axis.x * L(0, 0) + axis.y * L(0, 1) + axis.z * L(0, 2),
                                  axis.x * L(1, 0) + axis.y * L(1, 1) + axis.z * L(1, 2),
                                  axis.x * L(2, 0) + axis.y * L(2, 1) + axis.z * L(2, 2)};
                    axis = v_normalize(r);
                }
                float dot = v_dot(tdir, idir);
                dot = dot < -1.0f ? -1.0f : dot;
                dot = 1.0f < dot ? 1.0f : dot;
                const float ac = d_acos(dot), cap = ik.angle_limit * float(j + 1);
                const float angle = cap < ac ? cap : ac;
                const Quat ikr_old = cs.quat(ls, kStIkRot);
                Quat ikr = q_mul(axis_to_quat(axis, angle), ikr_old);
                const Quat pre = cs.quat(ls, kStPreIkRot);
                if (lk.limited) {
                    Quat lr = q_mul(ikr, pre);
                    float e[3];
                    quat_to_euler_coop(lk.order, lr, e, sub);
                    limit_euler(e, lk.lo, lk.hi, i < ikt);
                    lr = euler_to_quat_coop(lk.order, e, sub);
                    ikr = q_mul(lr, q_inverse(pre));
                }
                changed = changed || __float_as_uint(ikr.i) != __float_as_uint(ikr_old.i) || __float_as_uint(ikr.j) != __float_as_uint(ikr_old.j) ||
                          __float_as_uint(ikr.k) != __float_as_uint(ikr_old.k) || __float_as_uint(ikr.e) != __float_as_uint(ikr_old.e);
                // the link just turned: ik_rotation * pre-IK rotation, as the reference; its matrix before the parent product
                const Quat total = q_mul(ikr, pre);
                Mat4 M = q_to_matrix(total);
                const V3 off = ch.offset(j);
                M.m[3][0] = cs.at(ls, kStTotalTr + 0) + off.x;
                M.m[3][1] = cs.at(ls, kStTotalTr + 1) + off.y;
                M.m[3][2] = cs.at(ls, kStTotalTr + 2) + off.z;
                const float mine = pick16(M, sub);
                group_sync();                                  // every lane has read what the stores below replace
                if (sub == 0) { cs.set_quat(ls, kStIkRot, ikr); cs.set_quat(ls, kStTotalRot, total); }
                win[kCoopLpre + ls * 16 + sub] = mine;
                float prev = lp >= 0 ? coop_mul(mine, loc) : mine;
                cs.at(ls, kStLocal + sub) = prev;
                for (uint32_t k = 1; k <= j; ++k) {            // below it nothing changed: the cached matrix IS the recomputed one
                    const uint32_t jj = j - k;
                    prev = coop_mul(win[kCoopLpre + jj * 16 + sub], prev);
                    cs.at(jj, kStLocal + sub) = prev;
                }
                const float T = coop_mul(tpre, prev);          // the target hangs off link 0, the last one placed
                cs.at(tidx, kStLocal + sub) = T;
                tgt = {lane_of_group<12>(T), lane_of_group<13>(T), lane_of_group<14>(T)};
                group_sync();                                  // the next link step reads the matrices just stored
            }
            const V3 err = {ik_pos.x - tgt.x, ik_pos.y - tgt.y, ik_pos.z - tgt.z};
            if (v_dot(err, err) < 1e-7f) break;
            // ccd()'s shortcut: a sweep that reproduced every link's IK rotation bit for bit (bit patterns, so a NaN that keeps its bits
            // counts as reproduced and -0 for +0 as a change; exact because a sweep is a function of the chain's bits alone) skips the
            // rest of its half.  All sixteen lanes hold the same rotations, so the group takes the same way out.
            if (!changed) {
                if (i >= ikt) break;
                i = ikt - 1;
            }
        }
    }
    group_sync();
    for (uint32_t j = 0; j < n; ++j) copy(j, links[j].bone, false);
    copy(n, ik.target, false);

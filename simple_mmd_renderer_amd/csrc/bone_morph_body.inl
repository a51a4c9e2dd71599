// bone_morph_body.inl -- one thread's walk over the bone-morph applications; included by bone_morph_kernel and bone_morph_select_kernel
// (rig_kernels.hip), which define `inst` (the thread's state cell, p.ni cells: the instance, or the list position) and `row` (its row
// of per-instance rates: the instance, or ids[inst]).  Text, not a function, for the reason skeleton_ordered_body.inl gives.
    float *out = p.out + inst;
    const size_t n = p.ni;
    for (uint32_t b = 0; b < p.nb; ++b) {
        float *o = out + size_t(b) * kMorphStateFloats * n;
        o[0] = 0.f; o[n] = 0.f; o[2 * n] = 0.f;
        o[3 * n] = 0.f; o[4 * n] = 0.f; o[5 * n] = 0.f; o[6 * n] = 1.f;
    }
    const float *rates = p.rates + (p.shared ? 0 : size_t(row) * p.nm);
    for (uint32_t a = 0; a < p.napps; ++a) {
        const BoneMorphApp app = p.apps[a];
        float r = rates[app.top];
        bool skip = r < 1e-7f;
        for (uint32_t c = 0; !skip && c < app.chain_len; ++c) {
            r = p.chain[app.chain_off + c] * r;
            skip = r < 1e-7f;
        }
        if (skip) continue;
        float *o = out + size_t(app.bone) * kMorphStateFloats * n;
        o[0] = o[0] + app.tr[0] * r; o[n] = o[n] + app.tr[1] * r; o[2 * n] = o[2 * n] + app.tr[2] * r;
        const Quat cur = {o[3 * n], o[4 * n], o[5 * n], o[6 * n]};
        const Quat q = q_mul(cur, q_slerp_from_identity({app.rot[0], app.rot[1], app.rot[2], app.rot[3]}, r));
        o[3 * n] = q.i; o[4 * n] = q.j; o[5 * n] = q.k; o[6 * n] = q.e;
    }

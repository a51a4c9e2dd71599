// launch_shape.cpp -- see launch_shape.hpp.  This is where the project's measured knowledge about launch shapes lives: every constant
// below carries a number from LAB_NOTES.md or profiles/.
#include "launch_shape.hpp"

#include <algorithm>
#include <cstring>

namespace mmdx {

namespace {
constexpr size_t kLdsPerCu = 160 * 1024;

// Store flavour of a crowd launch (kernels.hip CopyFast), decided from the CALL alone -- no table of addresses, no state behind the
// boundary: the caller's hint first (mmdx_placement_info.store_flags hands it the probe's verdict for arrays from
// mmdx_crowd_output_alloc), then MMDX_STORE_WT=0 / 1 (A/B runs), then the default for arrays nothing is known about: outputs large
// enough to stream through the caches (>= 512 MB per call) are written through, because six plain allocations in seven are not in
// the fast store mode (expected cost of the wrong guess: 2 % on a fast pair against 4.6-5 % on the others).
bool write_through_for(size_t out_bytes, uint32_t flags, int store_wt) {
    if (flags & MMDX_OUT_STORES_WRITE_THROUGH) return true;
    if (flags & MMDX_OUT_STORES_CACHED) return false;
    if (store_wt == 0 || store_wt == 1) return store_wt == 1;
    return out_bytes >= (size_t(512) << 20);
}
}  // namespace

mmdx_status plan_deform_launch(const Plan &p, const DeformCall &c, const LaunchOverrides &ov, LaunchShape &s, std::string &err) {
    const uint32_t layout = c.layout, ni = c.ni, nwork = c.nwork;
    const int morph = c.morph;
    const bool tile_order = (p.flags & MMDX_CREATE_TILE_ORDER) != 0;
    s = LaunchShape{};
    // The bounds and the select flavours exist of deform_kernel only, and with nt stores only: such calls never take the write-through
    // store flavour (they store cached whatever the hint says), the pack kernel (an archived A/B) or the frame kernel.
    const bool plain = !c.bounds && !c.select;

    // ---- workgroup shape ------------------------------------------------------------------------------
    // 256 threads / two vertex slots per lane everywhere except the per-instance-morph path: there one slot
    // per lane (512 threads) leaves the registers to serve 8 instances per walk over a morph row.
    // A single frame (one instance) is latency-bound: one slot per lane and twice the waves per tile finish sooner
    // (config 2: 8.4 -> 6.9 us, config 5: 16.9 -> 14.9 us).
    const bool one_frame = ni == 1 && nwork <= 1 && (morph == kMorphNone || morph == kMorphFused1);
    // (tile-order outputs: no LDS image, 80 VGPRs with one slot per lane -- 512 threads measured 215.5 vs 219.1 us on the crowd)
    int threads = (ov.threads ? ov.threads : (morph == kMorphFused4 || one_frame || tile_order ? 512 : 256)) == 512 ? 512 : 256;
    if (morph == kMorphFused4 && threads == 512) {   // tiles with hundreds of bones: 8 palettes do not fit, 4 may
        uint32_t so, wo;
        if (deform_lds_bytes(512, layout, morph, 8, p.max_tile_bones, p.ns, &so, &wo) > kLdsPerCu) threads = 256;
    }
    s.threads = threads;
    // ---- store flavour: only where the launch shape has the write-through flavour, and only for outputs in device memory (stores
    // into mapped host memory cross PCIe whatever their cache bits say) ------------------------------------------------------------
    s.write_through = plain && c.out_dev && deform_has_write_through(threads, int(layout), morph, p.f16, tile_order) &&
                      write_through_for(c.out_bytes, c.flags, ov.store_wt);
    // ---- group size (instances per workgroup) from the LDS budget ---------------------------------
    const uint32_t gmin = morph == kMorphFused4 ? (threads == 512 ? 8u : 4u) : 1u;
    uint32_t group = gmin;
    if (morph != kMorphFused1 || ni > 1) {
        const uint32_t target = uint32_t(ov.lds_target ? ov.lds_target : (morph == kMorphFused4 ? 64 : 42) * 1024);
        uint32_t so, wo;
        const size_t fixed = deform_lds_bytes(threads, layout, morph, 0, p.max_tile_bones, p.ns, &so, &wo, tile_order);
        const size_t per = size_t(p.max_tile_bones) * 48;
        uint32_t g = target > fixed ? uint32_t((target - fixed) / per) : 0u;
        g = std::min(g, (morph == kMorphFused4 || tile_order) ? 16u : 32u);   // tile order: 16 219 us, 32 229 us, 8 244 us
        if (g >= 8) g &= ~3u;   // measured: 16 beats 17 (even split of 1024 instances, aligned strides)
        // write-through stores go to arrays that are not in the fast store mode; there 8 instances per workgroup (four workgroups
        // per CU, half the open output streams each) beat 16 by 3-8 % -- 218-224 vs 225-241 us on four such pairs, while on a fast
        // pair 16 wins (204 vs 211): profiles/r03/shape_sweep_write_through*.txt
        if (s.write_through) g = std::min(g, 8u);
        g = std::max(g / gmin * gmin, gmin);
        const uint32_t ni_up = (std::max(nwork, 1u) + gmin - 1) / gmin * gmin;
        g = std::min(g, ni_up);
        // keep the grid large enough to fill 256 CUs several times over
        while (g > gmin && uint64_t(p.ntiles) * ((nwork + g - 1) / g) < 2048) {
            const uint32_t half = std::max((g / 2) / gmin * gmin, gmin);
            if (half == g) break;
            g = half;
        }
        group = std::max(g, gmin);
        const int forced = ov.group;
        if (forced > 0) group = std::max(uint32_t(forced) / gmin * gmin, gmin);
    }
    s.group = group;
    // Per-instance morph weights, second shape (kernels.hip pack_kernel), OPT-IN (MMDX_FUSED_PACK=1): packs of 4 instances, 80 registers,
    // three 8-wave workgroups per CU while a workgroup's LDS stays under a third of the CU's.  It runs at 5.7 waves per SIMD where
    // deform_kernel<512, ., kMorphFused4> runs at 3.8 -- and loses (config 3' 372-382 us against 335-348; profiles/r04/fused_pack_*):
    // the walk and the skinning of one CU do not overlap in either kernel (walk alone 132 us + skinning alone 254 us), and packs of 4
    // walk the table twice as often as packs of 8.  Kept for the A/B, not the default.  Two-array layouts in original vertex order.
    // The group: as many instances (multiple of 4, up to 16) as keep three workgroups on a CU, else as fit two.
    bool pack = plain && morph == kMorphFused4 && ov.fused_pack != 0 && kTileVerts == 512 && !tile_order && layout != MMDX_OUT_VERTEX32 &&
                !ov.threads;
    size_t lds = 0;
    if (pack) {
        uint32_t so, wo, mo;
        const size_t third = kLdsPerCu / 3 - 64, half = 80 * 1024 - 64;
        uint32_t g = 0;
        for (uint32_t k = 16; k >= 4 && !g; k -= 4)
            if (pack_lds_bytes(k, p.max_tile_bones, p.ns, &so, &wo, &mo) <= third) g = k;
        for (uint32_t k = 16; k >= 4 && !g; k -= 4)
            if (pack_lds_bytes(k, p.max_tile_bones, p.ns, &so, &wo, &mo) <= half) g = k;
        if (!g && pack_lds_bytes(4, p.max_tile_bones, p.ns, &so, &wo, &mo) <= kLdsPerCu) g = 4;
        if (g) {
            g = std::min(g, (ni + 3) / 4 * 4);
            while (g > 4 && uint64_t(p.ntiles) * ((ni + g - 1) / g) < 1536) g -= 4;     // keep 256 CUs x 3 workgroups busy twice over
        }
        // (forced last, as for the tile kernel above: a forced group is not shrunk to fill the chip)
        if (ov.group > 0) g = std::max(uint32_t(ov.group) / 4 * 4, 4u);
        if (g) {
            s.group = g;
            lds = pack_lds_bytes(g, p.max_tile_bones, p.ns, &s.stage_off, &s.w_off, &s.mp_off);
            if (lds > kLdsPerCu) pack = false;
        } else {
            pack = false;
        }
    }
    if (!pack) {
        s.group = group;
        lds = deform_lds_bytes(threads, layout, morph, group, p.max_tile_bones, p.ns, &s.stage_off, &s.w_off, tile_order);
        if (c.bounds && !tile_order) {
            s.bounds_off = uint32_t(lds);
            lds += kBoundsLdsBytes;
        }
    }
    s.bounds_units = c.bounds ? deform_bounds_units(threads, p.ntiles, tile_order) : 0u;
    s.lds = lds;
    if (lds > kLdsPerCu) {
        err = "tile needs " + std::to_string(lds) + " bytes of LDS (> 160 KiB): "
              "too many distinct bones in one vertex tile / too many morph slots";
        return MMDX_ERR_UNSUPPORTED;
    }

    if (morph == kMorphFused4) {
        s.stagger = uint32_t(std::max(ov.stagger, 0));
        s.slots_per_cu = std::max<uint32_t>(1u, std::min<uint32_t>(uint32_t(kLdsPerCu / std::max<size_t>(lds, 1)), pack ? 3u : 2u));
    }
    // One frame of one model into device memory: the latency-ordered kernel (parts of tiles on every CU, direct stores).
    // Outputs in mapped host memory keep the tile kernel: its 16-byte coalesced stores are what crosses PCIe well.
    // Models with fewer tiles than the chip has CUs only (config 2: 6.3 us against the tile kernel's 6.9); a large model fills the
    // chip with whole tiles and is better off with their coalesced stores (config 5: 14.9 us against 15.2).
    const bool frame = plain && one_frame && !c.out_host_mapped && (ov.frame_kernel == 2 || (ov.frame_kernel == 1 && p.ntiles < 256));
    if (frame) {
        s.kernel = LaunchShape::kFrame;
        s.lds = frame_lds_bytes(morph, p.max_tile_bones, p.ns, &s.w_off);
        if (s.lds > kLdsPerCu) {
            err = "tile needs " + std::to_string(s.lds) + " bytes of LDS (> 160 KiB)";
            return MMDX_ERR_UNSUPPORTED;
        }
    } else if (pack) {
        s.kernel = LaunchShape::kPack;
    } else if (c.select && nwork == 0) {
        // an empty list: no instance to write (the shared morph pass has run as in the plain call)
        s.kernel = LaunchShape::kNone;
    } else {
        s.kernel = LaunchShape::kDeform;
    }
    return MMDX_OK;
}

mmdx_status plan_morph_pass(const MorphCall &c, const MorphRecord &rec, MorphPlan &pl, std::string &err) {
    pl = MorphPlan{};
    pl.morphed_valid = rec.morphed_valid;
    const uint32_t ni = c.ni;
    const bool shared = (c.flags & MMDX_WEIGHTS_SHARED) != 0 || ni == 1;      // one set of rates for the call
    const bool promised = shared && ni > 1 && (c.flags & MMDX_MORPH_UNCHANGED);
    if (promised && !rec.morphed_valid) {
        err = "MMDX_MORPH_UNCHANGED without an earlier MMDX_WEIGHTS_SHARED crowd call on this model";
        return MMDX_ERR_INVALID_ARGUMENT;
    }
    if (!c.ns) return MMDX_OK;                                  // kMorphNone: nothing to upload, launch or remember
    pl.upload = !(c.flags & MMDX_WEIGHTS_ON_DEVICE) && !promised;
    pl.niw = pl.wslot_rows = 1;
    if (!shared) {
        pl.morph = kMorphFused4;
        pl.pass = MorphPlan::kFlatten;
        pl.quad = true;
        pl.select_rows = c.select;
        pl.niw = c.select ? c.n_ids : ni;                       // (select: one row per list position)
        pl.wslot_rows = (pl.niw + 3) / 4 * 4;
        return MMDX_OK;
    }
    if (ni == 1) {
        // A single frame leaves the model's kept positions alone: they belong to the last SHARED CROWD call (MMDX_MORPH_UNCHANGED
        // is documented against that one), whichever kernel the frame takes.
        pl.morph = kMorphFused1;
        pl.pass = MorphPlan::kGather;
        pl.withhold_morphed = true;
        return MMDX_OK;
    }
    // A crowd with one facial state.  SMALL crowds gather the morphs inside the deform kernel like a single frame (every workgroup
    // repeats its tile's walk; no separate launch: 8.8 vs 10.1 us for 2 instances of the 50k model, break-even at 8,
    // tools/archive/probes/shared_ab.py); larger crowds run the morph pass once, in front (257 vs 269 us for 1024 instances) -- or
    // not at all when the caller declares the rates unchanged since the last such call.
    // shared_fused: 0 never for crowds, 1 small crowds (default), 2 always.
    const bool small = c.ns <= kMaxFusedSlots && (c.shared_fused == 2 || (c.shared_fused == 1 && ni <= 8));
    pl.morphed_valid = true;                                    // kept by either path
    // (a select call with an empty list launches no deform kernel: its shared rates take the morph pass, so that the positions
    // later MMDX_MORPH_UNCHANGED calls rely on are there)
    if (small && !promised && !(c.select && c.n_ids == 0)) {
        pl.morph = kMorphFused1;
        pl.pass = MorphPlan::kGather;
        pl.seen = MorphPlan::kSeenClearedByDeform;              // it overwrites `morphed`: neither record describes it afterwards
        pl.host_rates = MorphPlan::kRatesVoid;
        return MMDX_OK;
    }
    pl.morph = kMorphShared;
    // The same as the caller's promise, without it: vertex_images_ depends on morph_rates_ only (poser_impl.inl:362-386), so a crowd
    // call whose shared rates are, bit for bit, those of the morph pass whose result this handle still holds needs no morph pass.
    // Rates in HOST memory are compared here (with the copy kept of the last pass's), the launch and the upload are skipped; rates
    // in DEVICE memory are compared by morph_apply_kernel itself, which then skips its walk (RatesSeen, kernels.hpp).
    // Only crowds past the small size keep and consult the host's copy (a small crowd gets here with a promise or an empty list).
    const bool host_rates_call = !small && !promised && !(c.flags & MMDX_WEIGHTS_ON_DEVICE);
    pl.host_skip = host_rates_call && c.morph_autoskip != 0 && rec.morphed_valid && rec.host_rates_valid && rec.n_host_rates == c.nm &&
                   std::memcmp(rec.host_rates, c.rates, size_t(c.nm) * 4) == 0;
    if (promised || pl.host_skip) {                             // nothing to launch: `morphed` holds the positions
        pl.upload = false;
        return MMDX_OK;
    }
    if (c.ns <= kMaxFusedSlots) {
        pl.pass = MorphPlan::kFusedApply;
        pl.seen = c.morph_autoskip != 0 ? MorphPlan::kSeenCompared : MorphPlan::kSeenUntouched;
    } else {
        pl.pass = MorphPlan::kFlattenApply;
        pl.seen = MorphPlan::kSeenClearedByMemset;              // this (rare: > 8192 slots) pass keeps no record of its rates
    }
    // the host's own record: the rates of the pass `morphed` now holds, when they were host memory
    pl.host_rates = host_rates_call ? MorphPlan::kRatesStored : MorphPlan::kRatesVoid;
    return MMDX_OK;
}

}  // namespace mmdx

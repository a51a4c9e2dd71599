// CPU driver of the morph planner (plan_morph_pass, simple_mmd_renderer_amd/csrc/launch_shape.cpp), built by tests/test_morph_plan.py
// with g++ under ASan + UBSan from this file and launch_shape.cpp alone.
//   morph_plan_driver sweep       the planner over a cross product of models, calls, overrides and handle records; every plan is checked
//                                 against the rules in launch_shape.hpp, restated here as properties; prints the row count
//   morph_plan_driver sequences L every sequence of up to L events, for every (slot class, shared_fused, autoskip) setting, against a
//                                 model of the truth: the kept positions are never read for rates they were not computed from
//   morph_plan_driver eval        scripted sequences on stdin, per step the morph mode, the kernel kind and the pass counters
// The handle and the device are simulated: Sim holds the handle's record as api.cpp keeps it, the device record as morph_apply_kernel
// and deform_kernel treat it (kernels.hip), and `truth` -- the rates `morphed` was really computed from.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../simple_mmd_renderer_amd/csrc/launch_shape.hpp"

using namespace mmdx;

namespace {

constexpr uint32_t kNm = 2;
const char kRefusal[] = "MMDX_MORPH_UNCHANGED without an earlier MMDX_WEIGHTS_SHARED crowd call on this model";

struct Setting { uint32_t ns; int shared_fused, autoskip; };

// One deform call.  rates: an id (> 0) standing for nm floats; a per-instance call has its own
struct Call {
    uint32_t ni;
    int rates;
    bool host, shared, unchanged;
    int sel;                    // -1: no list, else n_ids
};

void rates_of(int id, float out[kNm]) { out[0] = float(id); out[1] = 0.5f; }

uint32_t flags_of(const Call &c) {
    return (c.shared ? uint32_t(MMDX_WEIGHTS_SHARED) : 0u) | (c.unchanged ? uint32_t(MMDX_MORPH_UNCHANGED) : 0u) |
           (c.host ? 0u : uint32_t(MMDX_WEIGHTS_ON_DEVICE));
}

struct Sim {
    // the handle (api_internal.hpp)
    bool morphed_valid = false, host_rates_valid = false, replayed = false;
    float host_rates[kNm] = {0, 0};
    size_t n_host_rates = 0;
    uint32_t host_skips = 0;
    // the device record (kernels.hpp, RatesSeen)
    bool seen_valid = false;
    int seen_rates = 0;
    uint32_t walks = 0, skips = 0;
    // the truth: which rates `morphed` holds; 0 = none yet
    int truth = 0;
};

// The launches of a plan, on the device.  false: a comparison on the device skipped a walk that was needed
bool run_on_device(const MorphPlan &pl, int rates, Sim &s) {
    switch (pl.pass) {
    case MorphPlan::kFusedApply:            // morph_apply_kernel<., true>: compares and skips, or walks; records either way
        if (pl.seen == MorphPlan::kSeenCompared) {
            if (s.seen_valid && s.seen_rates == rates) {
                ++s.skips;
                if (s.truth != rates) return false;
            } else {
                ++s.walks;
                s.truth = rates;
            }
            s.seen_valid = true;
            s.seen_rates = rates;
        } else {
            s.truth = rates;
        }
        break;
    case MorphPlan::kFlattenApply:          // morph_apply_kernel<., false>, then the memset
        s.truth = rates;
        s.seen_valid = false;
        break;
    case MorphPlan::kGather:                // deform_kernel, kMorphFused1: workgroup 0 of every tile keeps its positions
        if (!pl.withhold_morphed) s.truth = rates;
        if (pl.seen == MorphPlan::kSeenClearedByDeform) s.seen_valid = false;
        break;
    case MorphPlan::kFlatten:
    case MorphPlan::kNoPass:
        break;
    }
    return true;
}

mmdx_status plan_call(const Setting &set, const Call &c, const Sim &s, const float *rates, MorphPlan &pl, std::string &err) {
    const MorphCall mc{set.ns, kNm, c.ni, flags_of(c), c.sel >= 0, c.sel >= 0 ? uint32_t(c.sel) : 0u, set.shared_fused, set.autoskip,
                       c.host ? rates : nullptr};
    return plan_morph_pass(mc, {s.morphed_valid, s.host_rates_valid, s.host_rates, s.n_host_rates}, pl, err);
}

// run_morph_pass (api.cpp) on the simulated handle.  `recording`: the launches go into a graph instead of running (the caller keeps
// the plan and replays it).  Returns false when the record proved unsound; `refused` says the call was refused (and changed nothing
// but `replayed`).
bool do_call(const Setting &set, const Call &c, Sim &s, MorphPlan &pl, bool &refused, bool recording = false) {
    if (s.replayed) { s.replayed = false; s.host_rates_valid = false; }
    float rates[kNm];
    rates_of(c.rates, rates);
    std::string err;
    const bool promised = c.shared && c.ni > 1 && c.unchanged;
    const mmdx_status st = plan_call(set, c, s, rates, pl, err);
    refused = st != MMDX_OK;
    // the caller's flag: refused exactly when the handle holds no positions
    if (refused != (promised && !s.morphed_valid)) return false;
    if (refused) return st == MMDX_ERR_INVALID_ARGUMENT && err == kRefusal;
    if (pl.host_skip) ++s.host_skips;
    if (!recording && !run_on_device(pl, c.rates, s)) return false;
    s.morphed_valid = pl.morphed_valid;
    if (pl.host_rates == MorphPlan::kRatesStored) { std::memcpy(s.host_rates, rates, sizeof(rates)); s.n_host_rates = kNm; }
    if (pl.host_rates != MorphPlan::kRatesKept) s.host_rates_valid = pl.host_rates == MorphPlan::kRatesStored;
    // the deform kernel reads `morphed` without the caller's word for it: it must hold this call's rates
    if (!recording && pl.morph == kMorphShared && !promised && s.truth != c.rates) return false;
    return true;
}

// A replay of a recorded call: its launches run again, behind the host's back
bool do_replay(const MorphPlan &graph, int rates, Sim &s) {
    const bool ok = run_on_device(graph, rates, s);
    s.replayed = true;
    return ok && (graph.morph != kMorphShared || graph.pass == MorphPlan::kNoPass || s.truth == rates);
}

uint64_t g_failures = 0;

// ---- (a) the rule sweep --------------------------------------------------------------------------------------------------------
struct Row {
    Setting set;
    Call c;
    bool morphed_valid, host_rates_valid;
    int kept;                   // the handle's copy of the host rates: 0 none, 1 = the call's, 2 others
};

void print_row(const Row &r) {
    std::fprintf(stderr, "ns=%u shared_fused=%d autoskip=%d ni=%u host=%d shared=%d unchanged=%d sel=%d morphed_valid=%d host_rates_valid=%d "
                         "kept=%d\n", r.set.ns, r.set.shared_fused, r.set.autoskip, r.c.ni, r.c.host, r.c.shared, r.c.unchanged, r.c.sel,
                 r.morphed_valid, r.host_rates_valid, r.kept);
}

#define CHECK(cond)                                                                                    \
    do {                                                                                               \
        if (!(cond)) {                                                                                 \
            if (g_failures++ < 20) { std::fprintf(stderr, "FAILED %s\n  ", #cond); print_row(r); }    \
            return;                                                                                    \
        }                                                                                              \
    } while (0)

void check_row(const Row &r, uint64_t &refusals) {
    const Call &c = r.c;
    const uint32_t ns = r.set.ns, ni = c.ni;
    Sim s;
    s.morphed_valid = r.morphed_valid; s.host_rates_valid = r.host_rates_valid;
    if (r.kept) { rates_of(r.kept == 1 ? c.rates : c.rates + 1, s.host_rates); s.n_host_rates = kNm; }
    float rates[kNm];
    rates_of(c.rates, rates);
    MorphPlan pl;
    std::string err;
    const mmdx_status st = plan_call(r.set, c, s, rates, pl, err);
    const bool one = c.shared || ni == 1, crowd = one && ni > 1, promised = crowd && c.unchanged;
    if (st != MMDX_OK) {
        CHECK(st == MMDX_ERR_INVALID_ARGUMENT && err == kRefusal && promised && !r.morphed_valid);
        ++refusals;
        return;
    }
    CHECK(!(promised && !r.morphed_valid) && err.empty());
    const bool apply = pl.pass == MorphPlan::kFusedApply || pl.pass == MorphPlan::kFlattenApply;
    const bool small = ns <= 8192 && (r.set.shared_fused == 2 || (r.set.shared_fused == 1 && ni <= 8));
    CHECK((pl.morph == kMorphNone) == (ns == 0));
    CHECK(pl.withhold_morphed == (ns != 0 && ni == 1));                                     // a single frame never keeps `morphed`
    CHECK((pl.morph == kMorphFused4) == (ns != 0 && !one));
    CHECK((pl.morph == kMorphFused1) == (ns != 0 && (ni == 1 || (crowd && small && !promised && c.sel != 0))));
    CHECK((pl.morph == kMorphShared) == (ns != 0 && crowd && pl.morph != kMorphFused1));
    // every mode has its pass form
    CHECK(pl.morph != kMorphNone || pl.pass == MorphPlan::kNoPass);
    CHECK((pl.morph == kMorphFused4) == (pl.pass == MorphPlan::kFlatten));
    CHECK((pl.morph == kMorphFused1) == (pl.pass == MorphPlan::kGather));
    CHECK(!apply || pl.morph == kMorphShared);
    CHECK(pl.morph != kMorphShared || (pl.pass == MorphPlan::kNoPass) == (promised || pl.host_skip));
    CHECK(pl.pass != MorphPlan::kFusedApply || ns <= 8192);
    CHECK(pl.pass != MorphPlan::kFlattenApply || ns > 8192);
    // the host's comparison: trusted only with everything that makes it true, and only by a call that would have stored its rates
    CHECK(pl.host_skip == (pl.morph == kMorphShared && !small && !promised && c.host && r.set.autoskip != 0 && r.morphed_valid &&
                           r.host_rates_valid && r.kept == 1));
    // a plan that uploads has host rates and a reader for them
    CHECK(pl.upload == (ns != 0 && c.host && !(pl.morph == kMorphShared && pl.pass == MorphPlan::kNoPass)));
    // rows
    const uint32_t niw = pl.morph == kMorphFused4 ? (c.sel >= 0 ? uint32_t(c.sel) : ni) : (ns ? 1u : 0u);
    CHECK(pl.niw == niw && pl.wslot_rows == (pl.morph == kMorphFused4 ? (niw + 3) / 4 * 4 : niw));
    CHECK(pl.quad == (pl.morph == kMorphFused4) && pl.select_rows == (pl.morph == kMorphFused4 && c.sel >= 0));
    // the device record
    CHECK((pl.seen == MorphPlan::kSeenCompared) == (pl.pass == MorphPlan::kFusedApply && r.set.autoskip != 0));
    CHECK((pl.seen == MorphPlan::kSeenClearedByMemset) == (pl.pass == MorphPlan::kFlattenApply));
    CHECK((pl.seen == MorphPlan::kSeenClearedByDeform) == (pl.pass == MorphPlan::kGather && ni > 1));
    // the handle's record afterwards
    const bool writes = apply || (pl.pass == MorphPlan::kGather && ni > 1);                 // `morphed` is overwritten
    CHECK(pl.morphed_valid == (r.morphed_valid || writes || pl.morph == kMorphShared));
    CHECK((pl.host_rates == MorphPlan::kRatesKept) == !writes);
    CHECK((pl.host_rates == MorphPlan::kRatesStored) == (apply && c.host && !small));
    // pinned, odd as it looks: a small crowd that promises unchanged rates reads `morphed`, launches nothing and records nothing
    if (ns != 0 && small && promised)
        CHECK(pl.morph == kMorphShared && pl.pass == MorphPlan::kNoPass && !pl.host_skip && pl.host_rates == MorphPlan::kRatesKept && !pl.upload);
    // ... and a small crowd's select call with an empty list takes the apply launch, and stores no host rates
    if (ns != 0 && small && crowd && !promised && c.sel == 0)
        CHECK(pl.pass == MorphPlan::kFusedApply && pl.host_rates == MorphPlan::kRatesVoid);
}

int sweep() {
    uint64_t rows = 0, refusals = 0;
    Row r{};
    r.c.rates = 1;
    for (uint32_t ns : {0u, 1u, 8192u, 8193u})
    for (uint32_t ni : {1u, 2u, 8u, 9u, 12u})
    for (int shared = 0; shared < 2; ++shared)
    for (int unchanged = 0; unchanged < 2; ++unchanged)
    for (int host = 0; host < 2; ++host)
    for (int sel : {-1, 0, 1, 9})
    for (int sf = 0; sf < 3; ++sf)
    for (int autoskip = 0; autoskip < 2; ++autoskip)
    for (int mv = 0; mv < 2; ++mv)
    for (int hv = 0; hv < 2; ++hv)
    for (int kept = 0; kept < 3; ++kept) {
        r.set = {ns, sf, autoskip};
        r.c.ni = ni; r.c.shared = shared; r.c.unchanged = unchanged; r.c.host = host; r.c.sel = sel;
        r.morphed_valid = mv; r.host_rates_valid = hv; r.kept = kept;
        ++rows;
        check_row(r, refusals);
    }
    std::printf("rows=%" PRIu64 " refusals=%" PRIu64 " failures=%" PRIu64 "\n", rows, refusals, g_failures);
    return g_failures ? 1 : 0;
}

// ---- (b) every short sequence ---------------------------------------------------------------------------------------------------
enum { kRatesA = 1, kRatesB = 2, kRatesOther = 3 };
struct Event { const char *name; bool replay; Call c; };
const Event kEvents[] = {
    {"host A", false, {12, kRatesA, true, true, false, -1}},
    {"host B", false, {12, kRatesB, true, true, false, -1}},
    {"device A", false, {12, kRatesA, false, true, false, -1}},
    {"device B", false, {12, kRatesB, false, true, false, -1}},
    {"host A unchanged", false, {12, kRatesA, true, true, true, -1}},
    {"host B unchanged", false, {12, kRatesB, true, true, true, -1}},
    {"device A unchanged", false, {12, kRatesA, false, true, true, -1}},
    {"device B unchanged", false, {12, kRatesB, false, true, true, -1}},
    {"small crowd", false, {4, kRatesOther, true, true, false, -1}},
    {"single frame", false, {1, kRatesOther, true, false, false, -1}},
    {"per-instance rates", false, {12, kRatesOther, true, false, false, -1}},
    {"select, empty list", false, {12, kRatesA, false, true, false, 0}},
    {"select, 9 ids", false, {12, kRatesB, false, true, false, 9}},
    {"replay A", true, {12, kRatesA, false, true, false, -1}},       // a replay of a recorded "device A" / "device B"
    {"replay B", true, {12, kRatesB, false, true, false, -1}},
};
constexpr int kNEvents = int(sizeof(kEvents) / sizeof(kEvents[0]));

struct Walker {
    Setting set;
    int max_len;
    int path[16];
    uint64_t sequences = 0, refusals = 0, reads = 0;

    void fail(int len) {
        if (g_failures++ >= 20) return;
        std::fprintf(stderr, "UNSOUND ns=%u shared_fused=%d autoskip=%d:", set.ns, set.shared_fused, set.autoskip);
        for (int i = 0; i < len; ++i) std::fprintf(stderr, " [%s]", kEvents[path[i]].name);
        std::fprintf(stderr, "\n");
    }
    void walk(const Sim &s, int len) {
        if (len == max_len) return;
        for (int e = 0; e < kNEvents; ++e) {
            const Event &ev = kEvents[e];
            Sim t = s;
            path[len] = e;
            bool ok;
            if (ev.replay) {
                // what the recorded call planned: a device-rates crowd call plans the same against any record
                MorphPlan graph;
                std::string err;
                ok = plan_call(set, ev.c, Sim{}, nullptr, graph, err) == MMDX_OK && do_replay(graph, ev.c.rates, t);
            } else {
                MorphPlan pl;
                bool refused;
                ok = do_call(set, ev.c, t, pl, refused);
                refusals += refused;
                reads += !refused && pl.morph == kMorphShared;
            }
            ++sequences;
            if (!ok) { fail(len + 1); continue; }
            walk(t, len + 1);
        }
    }
};

int sequences(int max_len) {
    uint64_t total = 0, refusals = 0, reads = 0;
    for (uint32_t ns : {0u, 40u, 8193u})
    for (int sf = 0; sf < 3; ++sf)
    for (int autoskip = 0; autoskip < 2; ++autoskip) {
        Walker w{};
        w.set = {ns, sf, autoskip};
        w.max_len = max_len;
        w.walk(Sim{}, 0);
        total += w.sequences; refusals += w.refusals; reads += w.reads;
    }
    std::printf("sequences=%" PRIu64 " events=%d settings=18 refusals=%" PRIu64 " reads=%" PRIu64 " failures=%" PRIu64 "\n", total, kNEvents,
                refusals, reads, g_failures);
    return g_failures ? 1 : 0;
}

// ---- (c) scripted sequences -------------------------------------------------------------------------------------------------------
//   seq <ns> <ntiles> <max_tile_bones> <shared_fused> <autoskip>      a fresh handle
//   call | record <ni> <rates> <host> <shared> <unchanged> <sel>      a deform call (device outputs); record: into a graph
//   replay                                                            of the last recorded call
int eval() {
    char word[32];
    Setting set{};
    Plan p;
    Sim s;
    MorphPlan graph{};
    int graph_rates = 0;
    int morph = 0, kernel = 0;
    while (std::scanf("%31s", word) == 1) {
        if (!std::strcmp(word, "seq")) {
            if (std::scanf("%u %u %u %d %d", &set.ns, &p.ntiles, &p.max_tile_bones, &set.shared_fused, &set.autoskip) != 5) return 2;
            p.ns = set.ns;
            s = Sim{};
            morph = kernel = 0;
            continue;
        }
        if (!std::strcmp(word, "replay")) {
            if (!do_replay(graph, graph_rates, s)) { std::printf("unsound\n"); continue; }
        } else {
            const bool recording = !std::strcmp(word, "record");
            Call c{};
            int host, shared, unchanged;
            if (std::scanf("%u %d %d %d %d %d", &c.ni, &c.rates, &host, &shared, &unchanged, &c.sel) != 6) return 2;
            c.host = host; c.shared = shared; c.unchanged = unchanged;
            MorphPlan pl;
            bool refused;
            if (!do_call(set, c, s, pl, refused, recording)) { std::printf("unsound\n"); continue; }
            if (refused) { std::printf("refused\n"); continue; }
            if (recording) { graph = pl; graph_rates = c.rates; }
            // the launch the plan's morph mode goes into (outputs in device memory, original vertex order, f32)
            const DeformCall dc{MMDX_OUT_SOA, c.ni, c.sel >= 0 ? uint32_t(c.sel) : c.ni, flags_of(c), pl.morph, false, c.sel >= 0, true, false,
                                size_t(c.ni) * p.ntiles * kTileVerts * 24};
            const LaunchOverrides ov{1, 0, 0, 0, 0, 0, 1, 256, set.shared_fused, -1, set.autoskip, 0, 0, 1};
            LaunchShape shape;
            std::string err;
            if (plan_deform_launch(p, dc, ov, shape, err) != MMDX_OK) { std::printf("error %s\n", err.c_str()); continue; }
            morph = pl.morph; kernel = int(shape.kernel);
        }
        std::printf("morph=%d kernel=%d walks=%u device_skips=%u host_skips=%u\n", morph, kernel, s.walks, s.skips, s.host_skips);
    }
    return 0;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc == 2 && !std::strcmp(argv[1], "sweep")) return sweep();
    if (argc == 3 && !std::strcmp(argv[1], "sequences")) return sequences(std::atoi(argv[2]));
    if (argc == 2 && !std::strcmp(argv[1], "eval")) return eval();
    std::fprintf(stderr, "usage: %s sweep | sequences <length> | eval\n", argv[0]);
    return 2;
}

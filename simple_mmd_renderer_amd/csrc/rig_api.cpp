// rig_api.cpp -- C ABI of the bone-track and skeleton entry points (include/mmdx.h) over the HIP runtime.
// Static tables (keys, curve tables, chains) are uploaded on first use per device; per-call operands may
// live on the host (copied through handle-owned scratch) or in HBM.  No CPU fallback.
//
// Every device call is the same sequence, and every step of it is one function, defined ahead of the entry points here or -- the
// steps other files share: refuse_recording, stage_in, clock_in, route_out, finish, the list checks -- in host_runtime.hpp:
//   check the arguments (nothing here needs the device) -> resolve_stream -> refuse what a recording cannot hold (refuse_recording)
//   -> *_to_device -> graph_note_handle -> stage host operands (*_in) -> the parameter block (*_params) -> route_out -> launch ->
//   finish.  A track + solve call on a skeleton that needs two launches (two_launches) sizes a pose scratch and makes two such calls.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <initializer_list>
#include <memory>
#include <new>
#include <string>
#include <vector>

#include "../../include/mmdx.h"
#include "../../include/mmdx_bench.h"
#include "anim_kernels.hpp"
#include "api_internal.hpp"
#include "bone_mask.hpp"
#include "error.hpp"
#include "graph_pin.hpp"
#include "host_runtime.hpp"
#include "kernels.hpp"
#include "motion_blend.hpp"
#include "rig.hpp"
#include "rig_kernels.hpp"
#include "solve_shape.hpp"
#include "vmd.hpp"

using namespace mmdx;

namespace {

void release(const std::vector<DevBuf *> &bufs) {
    for (DevBuf *b : bufs) b->release();
}

// The key and curve tables of bone tracks in device memory: one motion's, or a set's clips laid end to end (rig.hpp).
struct BoneTables {
    DevBuf key_off, key_frame, key_tr, key_rot, key_curve, lut;
    mmdx_status upload(const BoneMotionHost &h) {
        HIP_TRY(key_off.upload(h.key_off));
        HIP_TRY(key_frame.upload(h.key_frame));
        HIP_TRY(key_tr.upload(h.key_tr));
        HIP_TRY(key_rot.upload(h.key_rot));
        HIP_TRY(key_curve.upload(h.key_curve));
        HIP_TRY(lut.upload(h.lut));
        return MMDX_OK;
    }
    // `ni`: instances, or the list positions of a select call; clock and output are the call's to fill in
    BoneTrackParams params(uint32_t nb, uint32_t ni) const {
        BoneTrackParams p;
        p.key_off = static_cast<const uint32_t *>(key_off.ptr);
        p.key_frame = static_cast<const uint32_t *>(key_frame.ptr);
        p.key_tr = static_cast<const float *>(key_tr.ptr);
        p.key_rot = static_cast<const float *>(key_rot.ptr);
        p.key_curve = static_cast<const uint32_t *>(key_curve.ptr);
        p.lut = static_cast<const float *>(lut.ptr);
        p.frames = nullptr; p.out = nullptr; p.times = nullptr;
        p.nb = nb; p.ni = ni;
        return p;
    }
};

}  // namespace

struct mmdx_bone_motion_s {
    BoneMotionHost host;
    int device = -1;
    BoneTables t;
    DevBuf frames_in, out;
    GraphPin pin;                                         // recorded graphs that hold these buffers' addresses
    std::vector<DevBuf *> all() { return {&t.key_off, &t.key_frame, &t.key_tr, &t.key_rot, &t.key_curve, &t.lut, &frames_in, &out}; }
    mmdx_bone_motion_s() {
        for (DevBuf *b : all()) { b->pin = &pin; b->floor = 16; }    // (the floor: host_runtime.hpp)
    }
};

struct mmdx_skeleton_s {
    SkeletonPlan plan;
    int device = -1;
    DevBuf local_offset, neg_rest, chain_off, chain, poses_in, out;
    DevBuf order, bones, iks, links, events, rounds, state;  // ordered solver
    DevBuf apps, app_chain, rates_in, morph_state;           // bone morphs
    DevBuf over_bone, over_strict, over_skin;                // physics seam: the reactor's writes of one frame
    DevBuf sel_in;                                           // mmdx_skeleton_solve_select with a host list: {live count, ids[live]}
    std::vector<uint32_t> sel_host;                       // ... its source, alive until the copy has left it
    uint32_t pre_instances = 0;                           // instances of the last mmdx_skeleton_solve_pre (0: none pending)
    const float *pre_poses = nullptr;                     // the poses that call solved (device address)
    const float *pre_morph = nullptr;
    SolveShape last_solve;                                // what the last successful solve launched (mmdx_debug_last_solve_shape)
    GraphPin pin;                                         // recorded graphs that hold these buffers' addresses
    std::vector<DevBuf *> all() {
        return {&local_offset, &neg_rest, &chain_off, &chain, &poses_in, &out, &order, &bones, &iks, &links, &events, &rounds, &state,
                &apps, &app_chain, &rates_in, &morph_state, &over_bone, &over_strict, &over_skin, &sel_in};
    }
    mmdx_skeleton_s() {
        for (DevBuf *b : all()) { b->pin = &pin; b->floor = 16; }    // (the floor: host_runtime.hpp)
    }
};

// A bank of clips bound to one model (rig.hpp MotionSetHost): the concatenated tables of both sides, uploaded on first use.
struct mmdx_motion_set_s {
    MotionSetHost host;
    std::vector<uint32_t> clip_frames;                              // [n_clips] largest key frame of each clip (mmdx_motion_set_clip_frames)
    int device = -1;
    BoneTables t;                                                   // bone side
    DevBuf m_key_off, m_frames, m_weights;                             // morph side
    DevBuf clips_in, clock_in;                                         // host operands: 4 + 8 bytes per instance
    DevBuf blend_in;                                                   // host operands of a blend call: 28 bytes per instance
    DevBuf poses, out;                                                 // the two-launch palette path's poses; results bound for the host
    DevBuf sel_in;                                                     // a *_blend_*_time_select call with a host list: {live count, ids[live]}
    std::vector<uint32_t> sel_host;                                 // ... its source, alive until the copy has left it
    GraphPin pin;                                                   // recorded graphs that hold these buffers' addresses
    std::vector<DevBuf *> all() {
        return {&t.key_off, &t.key_frame, &t.key_tr, &t.key_rot, &t.key_curve, &t.lut, &m_key_off, &m_frames, &m_weights, &clips_in,
                &clock_in, &blend_in, &poses, &out, &sel_in};
    }
    mmdx_motion_set_s() {
        for (DevBuf *b : all()) { b->pin = &pin; b->floor = 16; }    // (the floor: host_runtime.hpp)
    }
};

SkeletonRest mmdx::skeleton_rest(const mmdx_skeleton_s *s) { return {s->plan.nb, s->plan.parent.data(), s->plan.neg_rest.data()}; }

const std::vector<uint32_t> &mmdx::motion_set_clip_frames(const mmdx_motion_set_s *set) { return set->clip_frames; }

// ---- static tables of a motion / a skeleton / a set -> the device they are about to run on (once per device) --------------------
static mmdx_status motion_to_device(mmdx_bone_motion_t m, int device) {
    if (m->device == device) return MMDX_OK;
    if (graph_pinned(&m->pin)) return hip_fail(hipErrorIllegalState, "moving a bone motion to another device");
    release(m->all());
    if (mmdx_status r = m->t.upload(m->host)) return r;
    m->device = device;
    return MMDX_OK;
}

static mmdx_status skeleton_to_device(mmdx_skeleton_t s, int device) {
    if (s->device == device) return MMDX_OK;
    if (graph_pinned(&s->pin)) return hip_fail(hipErrorIllegalState, "moving a skeleton to another device");
    const SkeletonPlan &pl = s->plan;
    release(s->all());
    HIP_TRY(s->apps.upload(pl.apps));
    HIP_TRY(s->app_chain.upload(pl.app_chain));
    if (pl.serial) {
        HIP_TRY(s->order.upload(pl.order));
        HIP_TRY(s->bones.upload(pl.bones));
        HIP_TRY(s->iks.upload(pl.iks));
        HIP_TRY(s->links.upload(pl.links));
        HIP_TRY(s->events.upload(pl.events));
        HIP_TRY(s->rounds.upload(pl.rounds));
    } else {
        HIP_TRY(s->local_offset.upload(pl.local_offset));
        HIP_TRY(s->neg_rest.upload(pl.neg_rest));
        HIP_TRY(s->chain_off.upload(pl.chain_off));
        HIP_TRY(s->chain.upload(pl.chain));
    }
    s->device = device;
    return MMDX_OK;
}

static mmdx_status set_to_device(mmdx_motion_set_t set, int device) {
    if (set->device == device) return MMDX_OK;
    if (graph_pinned(&set->pin)) return hip_fail(hipErrorIllegalState, "moving a motion set to another device");
    const MotionSetHost &h = set->host;
    release(set->all());
    if (h.has_bones)
        if (mmdx_status r = set->t.upload(h.bones)) return r;
    if (h.has_morphs) {
        HIP_TRY(set->m_key_off.upload(h.morph_key_off));
        HIP_TRY(set->m_frames.upload(h.morph_frames));
        HIP_TRY(set->m_weights.upload(h.morph_weights));
    }
    set->device = device;
    return MMDX_OK;
}

SetBoneSide mmdx::motion_set_bone_side(const mmdx_motion_set_s *set) {
    return {set->host.has_bones, set->host.n_clips, set->host.has_bones ? set->host.bones.nb : 0u, set->device};
}

mmdx_status mmdx::motion_set_bone_tables(mmdx_motion_set_s *set, mmdx_model_t model, int device, BoneTrackParams *p) {
    if (mmdx_status r = set_to_device(set, device)) return r;
    graph_note_handle(model, &set->pin);
    *p = set->t.params(set->host.bones.nb, 0);
    return MMDX_OK;
}

// ---- what a recording cannot hold (refuse_recording: host_runtime.hpp) ------------------------------------------------------------
static const uint32_t kClockAndOut = MMDX_FRAMES_ON_DEVICE | MMDX_OUT_ON_DEVICE;      // (MMDX_TIMES_ON_DEVICE is the same bit)
static const char *const kSkeletonRecording = "while a graph is being recorded every operand must be in device memory, the "
                                              "skeleton must have run on this device before, and physics overrides "
                                              "(host lists) are not recordable";
static const char *const kSetRecording = "while a graph is being recorded every operand must be in device memory and the motion set "
                                         "must have run on this device before";
static const char *const kSetSkeletonRecording = "while a graph is being recorded every operand must be in device memory and the "
                                                 "motion set and the skeleton must have run on this device before";

// Append bones / IK (the ordered solver), or a skeleton too large for the LDS pose table of the one-launch kernels: a track + solve
// call takes two launches -- the track call into a pose scratch of the motion (its `out`) or the set (its `poses`), then the solve.
static bool two_launches(const SkeletonPlan &pl) { return pl.serial || size_t(pl.nb) * 32 > kMotionFkMaxLds; }

// ... and growing that scratch is an allocation: a recording refuses, anything else moves the tables and sizes it.  (The one call
// on a single motion, skeleton_solve_motion, spells the same three steps out on m->out; it never asked for the device.)
static mmdx_status set_pose_scratch(mmdx_motion_set_t set, int device, size_t bytes, float **poses) {
    if (graph_recording() && (set->poses.bytes < bytes || set->device != device))
        return fail(MMDX_ERR_INVALID_ARGUMENT, "run the call once before recording: it sizes the motion set's pose buffer");
    if (mmdx_status r = set_to_device(set, device)) return r;
    HIP_TRY(set->poses.ensure(bytes));
    *poses = static_cast<float *>(set->poses.ptr);
    return MMDX_OK;
}

static size_t pose_bytes(uint32_t ni, uint32_t nb) { return size_t(ni) * nb * MMDX_POSE_FLOATS * sizeof(float); }
static size_t palette_bytes(uint32_t ni, uint32_t nb) { return size_t(ni) * nb * 16 * sizeof(float); }

// ---- host operands -> device addresses, through handle-owned scratch in stream order --------------------------------------------
// (one operand: stage_in; the clock of one motion: clock_in -- both in host_runtime.hpp)
// clip ids and the instant of every instance -> device addresses: the clips, and the clock in `*frames` or, with `time`, `*times`
// (the two clock fields of a parameter block).  MMDX_FRAMES_ON_DEVICE covers both operands; host operands go through the set's
// scratch (4 + 8 bytes per instance, room for frames or times).
static mmdx_status set_operands_in(mmdx_motion_set_t set, const uint32_t *clips, const void *clock, bool time, uint32_t n_instances,
                                   uint32_t flags, hipStream_t st, const uint32_t **dev_clips, const uint32_t **frames,
                                   const double **times) {
    *dev_clips = clips;
    if (!(flags & MMDX_FRAMES_ON_DEVICE)) {
        HIP_TRY(set->clips_in.ensure(size_t(n_instances) * 4));
        HIP_TRY(set->clock_in.ensure(size_t(n_instances) * 8));
        HIP_TRY(hipMemcpyAsync(set->clips_in.ptr, clips, size_t(n_instances) * 4, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(set->clock_in.ptr, clock, size_t(n_instances) * (time ? 8 : 4), hipMemcpyHostToDevice, st));
        *dev_clips = static_cast<const uint32_t *>(set->clips_in.ptr);
        clock = set->clock_in.ptr;
    }
    if (time) *times = static_cast<const double *>(clock);
    else *frames = static_cast<const uint32_t *>(clock);
    return MMDX_OK;
}

// the five operand arrays of a blend call that are in device memory already (all a select form takes) ...
static BlendOperands blend_operands_device(mmdx_motion_set_t set, const mmdx_motion_blend_args *a) {
    BlendOperands o;
    o.clips_a = a->clips_a; o.clips_b = a->clips_b;
    o.times_a = a->times_a; o.times_b = a->times_b;
    o.weights = a->weights;
    o.n_clips = set->host.n_clips;
    return o;
}

// ... and wherever they are: MMDX_TIMES_ON_DEVICE covers all five; host operands go through the set's scratch (times_a, times_b,
// clips_a, clips_b, weights laid end to end: 28 bytes per instance).
static mmdx_status blend_operands_in(mmdx_motion_set_t set, const mmdx_motion_blend_args *a, hipStream_t st, BlendOperands *o) {
    *o = blend_operands_device(set, a);
    if (a->flags & MMDX_TIMES_ON_DEVICE) return MMDX_OK;
    const size_t n = a->n_instances;
    HIP_TRY(set->blend_in.ensure(n * 28));
    char *base = static_cast<char *>(set->blend_in.ptr);
    const struct { const void *src; size_t off, bytes; } parts[5] = {{a->times_a, 0, n * 8},       {a->times_b, n * 8, n * 8},
                                                                     {a->clips_a, n * 16, n * 4}, {a->clips_b, n * 20, n * 4},
                                                                     {a->weights, n * 24, n * 4}};
    for (const auto &p : parts) HIP_TRY(hipMemcpyAsync(base + p.off, p.src, p.bytes, hipMemcpyHostToDevice, st));
    o->times_a = reinterpret_cast<const double *>(base);
    o->times_b = reinterpret_cast<const double *>(base + n * 8);
    o->clips_a = reinterpret_cast<const uint32_t *>(base + n * 16);
    o->clips_b = reinterpret_cast<const uint32_t *>(base + n * 20);
    o->weights = reinterpret_cast<const float *>(base + n * 24);
    return MMDX_OK;
}

// the list of a select call -> device addresses: a device list as it is; a host list through the handle's scratch (`sel_in`, its
// source `sel_host` alive until the copy has left it), count word first.  `cells` = list positions the launch is sized from -- state
// and bone-morph cells are per LIST POSITION --: the capacity of a device list, the ids in use of a host list.
static mmdx_status list_in(DevBuf &sel_in, std::vector<uint32_t> &sel_host, const mmdx_instance_select *sel, uint32_t n_instances,
                           uint32_t live_host, hipStream_t st, InstanceList *list, uint32_t *cells) {
    *list = InstanceList{sel->ids, sel->count, n_instances};
    if (sel->flags & MMDX_SELECT_ON_DEVICE) {
        *cells = sel->n_ids;
        return MMDX_OK;
    }
    *cells = live_host;
    if (live_host == 0) return MMDX_OK;
    return stage_list(sel_in, sel_host, sel->ids, live_host, live_host, st, &list->count, &list->ids);
}

// ---- parameter blocks from a handle ----------------------------------------------------------------------------------------------
static SkeletonParams fk_params(mmdx_skeleton_t s, uint32_t ni, const float *poses, const float *morph, float *out) {
    SkeletonParams fp;
    fp.morph = morph;
    fp.poses = poses; fp.out = out;
    fp.local_offset = static_cast<const float *>(s->local_offset.ptr);
    fp.neg_rest = static_cast<const float *>(s->neg_rest.ptr);
    fp.chain_off = static_cast<const uint32_t *>(s->chain_off.ptr);
    fp.chain = static_cast<const uint32_t *>(s->chain.ptr);
    fp.nb = s->plan.nb; fp.ni = ni;
    return fp;
}

static MorphTrackParams set_morph_params(mmdx_motion_set_t set, uint32_t ni) {
    MorphTrackParams t;
    t.key_off = static_cast<const uint32_t *>(set->m_key_off.ptr);
    t.key_frames = static_cast<const uint32_t *>(set->m_frames.ptr);
    t.key_weights = static_cast<const float *>(set->m_weights.ptr);
    t.nm = set->host.nm; t.ni = ni;
    t.frames = nullptr; t.times = nullptr; t.out = nullptr;
    return t;
}

static void note_fk_solve(mmdx_skeleton_t s) {
    s->last_solve = SolveShape{};
    s->last_solve.solver = 2;
}

// ---- the solve -------------------------------------------------------------------------------------------------------------------
// From "the poses are at a device address" on: the bone-morph pass (`rates`: device rates, or null for none), then the ordered solver
// or parallel FK, for all `cells` instances (`list` null) or for the `cells` positions of `list`.
// passes: bit 0 = reset + bone morphs + pre-physics list, bit 1 = (physics overrides +) post-physics list
static mmdx_status solve_on_device(mmdx_skeleton_t s, uint32_t cells, const InstanceList *list, const float *poses, const float *rates,
                                   bool shared_rates, float *out, uint32_t passes, hipStream_t st) {
    const SkeletonPlan &pl = s->plan;
    // bone morphs first: per-bone morph_translation_ / morph_rotation_ of every instance
    const float *morph_state = (passes & 1u) ? nullptr : s->pre_morph;
    if (rates) {
        HIP_TRY(s->morph_state.ensure(size_t(cells) * pl.nb * kMorphStateFloats * sizeof(float)));
        BoneMorphParams mp;
        mp.rates = rates;
        mp.apps = static_cast<const BoneMorphApp *>(s->apps.ptr);
        mp.chain = static_cast<const float *>(s->app_chain.ptr);
        mp.out = static_cast<float *>(s->morph_state.ptr);
        mp.napps = uint32_t(pl.apps.size()); mp.nb = pl.nb; mp.ni = cells; mp.nm = pl.nm; mp.shared = shared_rates ? 1u : 0u;
        HIP_TRY(list ? launch_bone_morph_select(mp, *list, st) : launch_bone_morph(mp, st));
        morph_state = mp.out;
    }
    if (!pl.serial) {
        const SkeletonParams fp = fk_params(s, cells, poses, morph_state, out);
        HIP_TRY(list ? launch_skeleton_fk_select(fp, *list, st) : launch_skeleton_fk(fp, st));
        note_fk_solve(s);
        return MMDX_OK;
    }
    HIP_TRY(s->state.ensure(size_t(cells) * pl.nb * kSerialStateFloats * sizeof(float)));
    SerialParams sp;
    sp.morph = morph_state;
    sp.poses = poses; sp.out = out;
    sp.state = static_cast<float *>(s->state.ptr);
    sp.order = static_cast<const uint32_t *>(s->order.ptr);
    sp.bones = static_cast<const BoneRec *>(s->bones.ptr);
    sp.iks = static_cast<const IkRec *>(s->iks.ptr);
    sp.links = static_cast<const LinkRec *>(s->links.ptr);
    sp.events = static_cast<const uint32_t *>(s->events.ptr);
    sp.rounds = static_cast<const RoundRec *>(s->rounds.ptr);
    sp.nb = pl.nb; sp.ni = cells; sp.n_pre = pl.n_pre;
    sp.n_rounds_pre = pl.n_rounds_pre; sp.n_rounds = uint32_t(pl.rounds.size());
    sp.fast_slots = pl.fast_slots;
    sp.windows = pl.windows;
    sp.passes = passes;
    sp.nested = pl.nested_ik ? 1u : 0u;
    const uint8_t *coop = pl.round_coop.empty() ? nullptr : pl.round_coop.data();
    HIP_TRY(list ? launch_skeleton_ordered_select(sp, coop, *list, st, &s->last_solve) : launch_skeleton_ordered(sp, coop, st, &s->last_solve));
    // a pre step leaves what its post step re-reads; after any other solve the scratch a pending pre step left is gone
    if (passes == 1u) { s->pre_instances = cells; s->pre_poses = poses; s->pre_morph = morph_state; }
    else s->pre_instances = 0;
    return MMDX_OK;
}

// mmdx_skeleton_solve / _morphed / _pre / _post (passes: as above)
static mmdx_status skeleton_solve(mmdx_skeleton_t s, mmdx_model_t model, uint32_t n_instances, const float *poses,
                                  const float *morph_weights, uint32_t flags, float *out_palettes, uint32_t passes,
                                  const mmdx_physics_overrides *ov) {
    if (!s || (!poses && (passes & 1u)) || !out_palettes || !n_instances)
        return fail(MMDX_ERR_INVALID_ARGUMENT, "NULL argument or n_instances == 0");
    int device;
    hipStream_t st;
    if (mmdx_status r = resolve_stream(model, &device, &st)) return r;
    const SkeletonPlan &pl = s->plan;
    const bool morphs = (passes & 1u) && morph_weights && !pl.apps.empty();
    const bool overrides = (passes & 2u) && ov && ov->n_bones;
    const uint32_t need = MMDX_OUT_ON_DEVICE | ((passes & 1u) ? uint32_t(MMDX_POSES_ON_DEVICE) : 0u) |
                          (morphs ? uint32_t(MMDX_WEIGHTS_ON_DEVICE) : 0u);
    if (graph_recording() && ov && ov->n_bones) return fail(MMDX_ERR_INVALID_ARGUMENT, kSkeletonRecording);
    if (mmdx_status r = refuse_recording(flags, need, device, {s->device}, kSkeletonRecording)) return r;
    if (mmdx_status r = skeleton_to_device(s, device)) return r;
    graph_note_handle(model, &s->pin);
    const float *dev_poses = poses;
    if (!(passes & 1u)) {
        dev_poses = s->pre_poses;                    // the post-physics list re-reads the poses the pre step solved:
                                                     // they must still be there (device poses are the caller's to keep)
    } else if (!(flags & MMDX_POSES_ON_DEVICE)) {
        if (mmdx_status r = stage_in(s->poses_in, poses, pose_bytes(n_instances, pl.nb), st)) return r;
        dev_poses = static_cast<const float *>(s->poses_in.ptr);
    }
    OutRoute o;
    if (mmdx_status r = route_out(flags, out_palettes, palette_bytes(n_instances, pl.nb), s->out, &o)) return r;
    const bool shared = (flags & MMDX_WEIGHTS_SHARED) != 0;
    const float *rates = morphs ? morph_weights : nullptr;
    const bool borrowed_rates = morphs && !(flags & MMDX_WEIGHTS_ON_DEVICE);
    if (borrowed_rates) {
        if (mmdx_status r = stage_in(s->rates_in, morph_weights, size_t(shared ? 1 : n_instances) * pl.nm * sizeof(float), st)) return r;
        rates = static_cast<const float *>(s->rates_in.ptr);
    }
    if (overrides) {                                  // the reactor's writes, between the two lists
        HIP_TRY(s->state.ensure(size_t(n_instances) * pl.nb * kSerialStateFloats * sizeof(float)));
        PhysicsParams pp;
        std::vector<uint32_t> ob(ov->bone, ov->bone + ov->n_bones);
        std::vector<uint8_t> os(ov->n_bones, 0);
        for (uint32_t k = 0; ov->strict && k < ov->n_bones; ++k) os[k] = ov->strict[k] ? 1 : 0;
        HIP_TRY(s->over_bone.ensure(ob.size() * 4));
        HIP_TRY(s->over_strict.ensure(os.size()));
        HIP_TRY(hipMemcpyAsync(s->over_bone.ptr, ob.data(), ob.size() * 4, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(s->over_strict.ptr, os.data(), os.size(), hipMemcpyHostToDevice, st));
        const size_t xf_bytes = size_t(n_instances) * ov->n_bones * 64;
        if (flags & MMDX_OVERRIDES_ON_DEVICE) {
            pp.skinning = ov->skinning;
        } else {
            if (mmdx_status r = stage_in(s->over_skin, ov->skinning, xf_bytes, st)) return r;
            pp.skinning = static_cast<const float *>(s->over_skin.ptr);
        }
        HIP_TRY(hipStreamSynchronize(st));        // ob / os are locals: the copies above must have read them
        pp.bone = static_cast<const uint32_t *>(s->over_bone.ptr);
        pp.strict = static_cast<const uint8_t *>(s->over_strict.ptr);
        pp.out = o.dev;
        pp.state = static_cast<float *>(s->state.ptr);
        pp.bones = static_cast<const BoneRec *>(s->bones.ptr);
        pp.k = ov->n_bones; pp.nb = pl.nb; pp.ni = n_instances;
        HIP_TRY(launch_physics_override(pp, st));
    }
    if (mmdx_status r = solve_on_device(s, n_instances, nullptr, dev_poses, rates, shared, o.dev, passes, st)) return r;
    return finish(flags, !(flags & MMDX_POSES_ON_DEVICE) || borrowed_rates, st, o);
}

// The list of a select call (mmdx_skeleton_solve_select, the *_blend_*_time_select calls), decided without the device: `plain` names
// the calls that take every instance; `live_host` = the ids of a host list that are in use.
static mmdx_status check_instance_list(const mmdx_instance_select *sel, uint32_t n_instances, const char *plain, uint32_t &live_host) {
    if (!sel) return fail(MMDX_ERR_INVALID_ARGUMENT, std::string("select is NULL (") + plain + ")");
    if (mmdx_status r = list_header_check(sel)) return r;
    if (mmdx_status r = list_placement_check(sel, graph_recording())) return r;      // this THREAD records: these calls may have no model
    return host_list_check(sel, n_instances, live_host);
}

// mmdx_skeleton_solve_select: mmdx_skeleton_solve_morphed for the listed instances (include/mmdx.h, rules 1-10).  Everything that can
// be decided without the device comes first, in the header's order.
static mmdx_status check_select_args(mmdx_skeleton_t s, uint32_t n_instances, const float *poses, const float *morph_weights,
                                     uint32_t flags, const mmdx_instance_select *sel, const float *out_palettes, uint32_t &live_host) {
    if (!s || !poses || !out_palettes || !n_instances) return fail(MMDX_ERR_INVALID_ARGUMENT, "NULL argument or n_instances == 0");
    const uint32_t need = MMDX_POSES_ON_DEVICE | MMDX_OUT_ON_DEVICE | (morph_weights ? uint32_t(MMDX_WEIGHTS_ON_DEVICE) : 0u);
    if ((flags & need) != need)
        return fail(MMDX_ERR_INVALID_ARGUMENT, "mmdx_skeleton_solve_select takes device operands only: pass MMDX_POSES_ON_DEVICE | "
                                               "MMDX_OUT_ON_DEVICE, and MMDX_WEIGHTS_ON_DEVICE with morph_weights");
    if (flags & ~uint32_t(MMDX_POSES_ON_DEVICE | MMDX_OUT_ON_DEVICE | MMDX_WEIGHTS_ON_DEVICE | MMDX_WEIGHTS_SHARED))
        return fail(MMDX_ERR_INVALID_ARGUMENT, "unknown flag bits");
    return check_instance_list(sel, n_instances, "mmdx_skeleton_solve / _morphed solve every instance", live_host);
}

// ---- one motion ------------------------------------------------------------------------------------------------------------------
// mmdx_bone_motion_eval / _eval_time: frames (uint32_t) or, with `time`, seconds (double)
static mmdx_status bone_motion_eval(mmdx_bone_motion_t m, mmdx_model_t model, uint32_t n_instances, const void *clock, bool time,
                                    uint32_t flags, float *out_poses) {
    if (!m || !clock || !out_poses || !n_instances)
        return fail(MMDX_ERR_INVALID_ARGUMENT, "NULL argument or n_instances == 0");
    int device;
    hipStream_t st;
    if (mmdx_status r = resolve_stream(model, &device, &st)) return r;
    if (mmdx_status r = refuse_recording(flags, kClockAndOut, device, {m->device},
                                         "while a graph is being recorded every operand must be in device memory and the "
                                         "motion must have run on this device before"))
        return r;
    if (mmdx_status r = motion_to_device(m, device)) return r;
    graph_note_handle(model, &m->pin);
    BoneTrackParams p = m->t.params(m->host.nb, n_instances);
    if (mmdx_status r = clock_in(m->frames_in, "bone motion clock scratch", clock, time, n_instances, flags, st, &p.frames, &p.times)) return r;
    OutRoute o;
    if (mmdx_status r = route_out(flags, out_poses, pose_bytes(n_instances, p.nb), m->out, &o)) return r;
    p.out = o.dev;
    HIP_TRY(launch_bone_track_eval(p, st));
    return finish(flags, !(flags & MMDX_FRAMES_ON_DEVICE), st, o);
}

// mmdx_skeleton_solve_motion / _time: frames (uint32_t) or, with `time`, seconds (double)
static mmdx_status skeleton_solve_motion(mmdx_skeleton_t s, mmdx_bone_motion_t m, mmdx_model_t model, uint32_t n_instances,
                                         const void *clock, bool time, uint32_t flags, float *out_palettes) {
    if (!s || !m || !clock || !out_palettes || !n_instances)
        return fail(MMDX_ERR_INVALID_ARGUMENT, "NULL argument or n_instances == 0");
    if (m->host.nb != s->plan.nb)
        return fail(MMDX_ERR_INVALID_ARGUMENT, "the motion was bound to " + std::to_string(m->host.nb) + " bones, the skeleton has " +
                                               std::to_string(s->plan.nb));
    int device;
    hipStream_t st;
    if (mmdx_status r = resolve_stream(model, &device, &st)) return r;
    const SkeletonPlan &pl = s->plan;
    if (two_launches(pl)) {
        const size_t bytes = pose_bytes(n_instances, pl.nb);
        if (graph_recording() && m->out.bytes < bytes)
            return fail(MMDX_ERR_INVALID_ARGUMENT, "run the call once before recording: it sizes the motion's pose buffer");
        if (mmdx_status r = motion_to_device(m, device)) return r;
        HIP_TRY(m->out.ensure(bytes));
        float *poses = static_cast<float *>(m->out.ptr);
        if (mmdx_status r = bone_motion_eval(m, model, n_instances, clock, time, (flags & MMDX_FRAMES_ON_DEVICE) | MMDX_OUT_ON_DEVICE, poses))
            return r;
        return mmdx_skeleton_solve(s, model, n_instances, poses, MMDX_POSES_ON_DEVICE | (flags & MMDX_OUT_ON_DEVICE), out_palettes);
    }
    if (mmdx_status r = refuse_recording(flags, kClockAndOut, device, {m->device, s->device},
                                         "while a graph is being recorded every operand must be in device memory and the motion "
                                         "and the skeleton must have run on this device before"))
        return r;
    if (mmdx_status r = motion_to_device(m, device)) return r;
    if (mmdx_status r = skeleton_to_device(s, device)) return r;
    graph_note_handle(model, &m->pin);
    graph_note_handle(model, &s->pin);
    BoneTrackParams tp = m->t.params(pl.nb, n_instances);
    if (mmdx_status r = clock_in(m->frames_in, "bone motion clock scratch", clock, time, n_instances, flags, st, &tp.frames, &tp.times)) return r;
    OutRoute o;
    if (mmdx_status r = route_out(flags, out_palettes, palette_bytes(n_instances, pl.nb), s->out, &o)) return r;
    HIP_TRY(launch_motion_fk(tp, fk_params(s, n_instances, nullptr, nullptr, o.dev), st));
    note_fk_solve(s);
    return finish(flags, !(flags & MMDX_FRAMES_ON_DEVICE), st, o);
}

// ---- motion sets -----------------------------------------------------------------------------------------------------------------
// Everything about a set call that can be decided without the device, in one place and before the first HIP call: NULLs, the
// instance count, flag bits, NaN in host times (check_time_args), the side the set was created without, host clip ids.
static mmdx_status set_check_args(mmdx_motion_set_t set, bool bone_side, uint32_t n_instances, const uint32_t *clips, const void *clock,
                                  bool time, uint32_t flags, const float *out) {
    if (!set || !clips || !clock || !out || !n_instances) return fail(MMDX_ERR_INVALID_ARGUMENT, "NULL argument or n_instances == 0");
    const uint32_t allowed = MMDX_FRAMES_ON_DEVICE | MMDX_OUT_ON_DEVICE;
    if (time) {
        if (mmdx_status r = check_time_args(static_cast<const double *>(clock), n_instances, flags, allowed)) return r;
    } else if (flags & ~allowed) {
        return fail(MMDX_ERR_INVALID_ARGUMENT, "unknown flag bits");
    }
    if (bone_side ? !set->host.has_bones : !set->host.has_morphs)
        return fail(MMDX_ERR_INVALID_ARGUMENT, std::string("this motion set was created without ") + (bone_side ? "bone" : "morph") + " motions");
    if (!(flags & MMDX_FRAMES_ON_DEVICE))
        for (uint32_t i = 0; i < n_instances; ++i)
            if (clips[i] >= set->host.n_clips && clips[i] != MMDX_CLIP_NONE)
                return fail(MMDX_ERR_BAD_INDEX, "clips[" + std::to_string(i) + "] = " + std::to_string(clips[i]) + ": the set has " +
                                                std::to_string(set->host.n_clips) + " clips");
    return MMDX_OK;
}

static mmdx_status skeleton_matches_set(mmdx_skeleton_t s, mmdx_motion_set_t set) {
    if (set->host.bones.nb != s->plan.nb)
        return fail(MMDX_ERR_INVALID_ARGUMENT, "the motion set was bound to " + std::to_string(set->host.bones.nb) +
                                               " bones, the skeleton has " + std::to_string(s->plan.nb));
    return MMDX_OK;
}

// mmdx_motion_set_eval_bones / _time: frames (uint32_t) or, with `time`, seconds (double)
static mmdx_status set_eval_bones(mmdx_motion_set_t set, mmdx_model_t model, uint32_t n_instances, const uint32_t *clips,
                                  const void *clock, bool time, uint32_t flags, float *out_poses) {
    if (mmdx_status r = set_check_args(set, true, n_instances, clips, clock, time, flags, out_poses)) return r;
    int device;
    hipStream_t st;
    if (mmdx_status r = resolve_stream(model, &device, &st)) return r;
    if (mmdx_status r = refuse_recording(flags, kClockAndOut, device, {set->device}, kSetRecording)) return r;
    if (mmdx_status r = set_to_device(set, device)) return r;
    graph_note_handle(model, &set->pin);
    BoneTrackParams p = set->t.params(set->host.bones.nb, n_instances);
    const uint32_t *dev_clips;
    if (mmdx_status r = set_operands_in(set, clips, clock, time, n_instances, flags, st, &dev_clips, &p.frames, &p.times)) return r;
    OutRoute o;
    if (mmdx_status r = route_out(flags, out_poses, pose_bytes(n_instances, p.nb), set->out, &o)) return r;
    p.out = o.dev;
    HIP_TRY(launch_bone_track_eval_set(p, dev_clips, set->host.n_clips, st));
    return finish(flags, !(flags & MMDX_FRAMES_ON_DEVICE), st, o);
}

// mmdx_motion_set_eval_morphs / _time
static mmdx_status set_eval_morphs(mmdx_motion_set_t set, mmdx_model_t model, uint32_t n_instances, const uint32_t *clips,
                                   const void *clock, bool time, uint32_t flags, float *out_weights) {
    if (mmdx_status r = set_check_args(set, false, n_instances, clips, clock, time, flags, out_weights)) return r;
    int device;
    hipStream_t st;
    if (mmdx_status r = resolve_stream(model, &device, &st)) return r;
    if (mmdx_status r = refuse_recording(flags, kClockAndOut, device, {set->device}, kSetRecording)) return r;
    if (mmdx_status r = set_to_device(set, device)) return r;
    graph_note_handle(model, &set->pin);
    MorphTrackParams t = set_morph_params(set, n_instances);
    const uint32_t *dev_clips;
    if (mmdx_status r = set_operands_in(set, clips, clock, time, n_instances, flags, st, &dev_clips, &t.frames, &t.times)) return r;
    OutRoute o;
    if (mmdx_status r = route_out(flags, out_weights, size_t(n_instances) * t.nm * sizeof(float), set->out, &o)) return r;
    t.out = o.dev;
    HIP_TRY(launch_morph_track_eval_set(t, dev_clips, set->host.n_clips, st));
    return finish(flags, !(flags & MMDX_FRAMES_ON_DEVICE), st, o);
}

// mmdx_skeleton_solve_motion_set / _time
static mmdx_status skeleton_solve_motion_set(mmdx_skeleton_t s, mmdx_motion_set_t set, mmdx_model_t model, uint32_t n_instances,
                                             const uint32_t *clips, const void *clock, bool time, uint32_t flags, float *out_palettes) {
    if (!s) return fail(MMDX_ERR_INVALID_ARGUMENT, "NULL argument or n_instances == 0");
    if (mmdx_status r = set_check_args(set, true, n_instances, clips, clock, time, flags, out_palettes)) return r;
    if (mmdx_status r = skeleton_matches_set(s, set)) return r;
    int device;
    hipStream_t st;
    if (mmdx_status r = resolve_stream(model, &device, &st)) return r;
    const SkeletonPlan &pl = s->plan;
    if (two_launches(pl)) {
        float *poses;
        if (mmdx_status r = set_pose_scratch(set, device, pose_bytes(n_instances, pl.nb), &poses)) return r;
        if (mmdx_status r = set_eval_bones(set, model, n_instances, clips, clock, time, (flags & MMDX_FRAMES_ON_DEVICE) | MMDX_OUT_ON_DEVICE,
                                           poses))
            return r;
        return mmdx_skeleton_solve(s, model, n_instances, poses, MMDX_POSES_ON_DEVICE | (flags & MMDX_OUT_ON_DEVICE), out_palettes);
    }
    if (mmdx_status r = refuse_recording(flags, kClockAndOut, device, {set->device, s->device}, kSetSkeletonRecording)) return r;
    if (mmdx_status r = set_to_device(set, device)) return r;
    if (mmdx_status r = skeleton_to_device(s, device)) return r;
    graph_note_handle(model, &set->pin);
    graph_note_handle(model, &s->pin);
    BoneTrackParams tp = set->t.params(pl.nb, n_instances);
    const uint32_t *dev_clips;
    if (mmdx_status r = set_operands_in(set, clips, clock, time, n_instances, flags, st, &dev_clips, &tp.frames, &tp.times)) return r;
    OutRoute o;
    if (mmdx_status r = route_out(flags, out_palettes, palette_bytes(n_instances, pl.nb), s->out, &o)) return r;
    HIP_TRY(launch_motion_fk_set(tp, fk_params(s, n_instances, nullptr, nullptr, o.dev), dev_clips, set->host.n_clips, st));
    note_fk_solve(s);
    return finish(flags, !(flags & MMDX_FRAMES_ON_DEVICE), st, o);
}

// ---- cross-fade between two clips of a set (mmdx_motion_set_blend_*_time, mmdx_skeleton_solve_motion_set_blend_time) ---------------
// Everything about a blend call that can be decided without the device, before the first HIP call, in two parts: the header (NULLs,
// struct_size) ...
static mmdx_status blend_check_header(mmdx_motion_set_t set, const mmdx_motion_blend_args *a, const float *out) {
    if (!set || !a || !out) return fail(MMDX_ERR_INVALID_ARGUMENT, "NULL argument");
    if (a->struct_size != sizeof(mmdx_motion_blend_args)) return fail(MMDX_ERR_INVALID_ARGUMENT, "mmdx_motion_blend_args.struct_size mismatch");
    return MMDX_OK;
}

// ... and the operands: their NULLs, the instance count, flag bits, the side the set was created without, and -- for host operands --
// clip ids of both arrays, NaN times and NaN weights.
static mmdx_status blend_check_operands(mmdx_motion_set_t set, bool bone_side, const mmdx_motion_blend_args *a) {
    if (!a->clips_a || !a->clips_b || !a->times_a || !a->times_b || !a->weights || !a->n_instances)
        return fail(MMDX_ERR_INVALID_ARGUMENT, "NULL argument or n_instances == 0");
    if (a->flags & ~uint32_t(MMDX_TIMES_ON_DEVICE | MMDX_OUT_ON_DEVICE)) return fail(MMDX_ERR_INVALID_ARGUMENT, "unknown flag bits");
    if (bone_side ? !set->host.has_bones : !set->host.has_morphs)
        return fail(MMDX_ERR_INVALID_ARGUMENT, std::string("this motion set was created without ") + (bone_side ? "bone" : "morph") + " motions");
    if (a->flags & MMDX_TIMES_ON_DEVICE) return MMDX_OK;
    const struct { const char *name; const uint32_t *clips; const double *times; } sides[2] = {{"a", a->clips_a, a->times_a},
                                                                                                 {"b", a->clips_b, a->times_b}};
    for (const auto &s : sides)
        for (uint32_t i = 0; i < a->n_instances; ++i)
            if (s.clips[i] >= set->host.n_clips && s.clips[i] != MMDX_CLIP_NONE)
                return fail(MMDX_ERR_BAD_INDEX, std::string("clips_") + s.name + "[" + std::to_string(i) + "] = " + std::to_string(s.clips[i]) +
                                                ": the set has " + std::to_string(set->host.n_clips) + " clips");
    for (const auto &s : sides)
        for (uint32_t i = 0; i < a->n_instances; ++i)
            if (s.times[i] != s.times[i])
                return fail(MMDX_ERR_INVALID_ARGUMENT, std::string("times_") + s.name + "[" + std::to_string(i) + "] is NaN");
    for (uint32_t i = 0; i < a->n_instances; ++i)
        if (a->weights[i] != a->weights[i]) return fail(MMDX_ERR_INVALID_ARGUMENT, "weights[" + std::to_string(i) + "] is NaN");
    return MMDX_OK;
}

static mmdx_status blend_check_args(mmdx_motion_set_t set, bool bone_side, const mmdx_motion_blend_args *a, const float *out) {
    if (mmdx_status r = blend_check_header(set, a, out)) return r;
    return blend_check_operands(set, bone_side, a);
}

// The select forms (mmdx_motion_set_blend_*_time_select, mmdx_skeleton_solve_motion_set_blend_time_select; include/mmdx.h, rules
// 1-10) take device operands only, and say so ahead of the operand part, which reads host operands when MMDX_TIMES_ON_DEVICE is
// absent; unknown flag bits are reported ahead of that.
static mmdx_status blend_select_check(mmdx_motion_set_t set, bool bone_side, const mmdx_motion_blend_args *a,
                                      const mmdx_instance_select *sel, const float *out, uint32_t &live_host) {
    if (mmdx_status r = blend_check_header(set, a, out)) return r;
    if (a->flags & ~uint32_t(MMDX_TIMES_ON_DEVICE | MMDX_OUT_ON_DEVICE)) return fail(MMDX_ERR_INVALID_ARGUMENT, "unknown flag bits");
    const uint32_t need = MMDX_TIMES_ON_DEVICE | MMDX_OUT_ON_DEVICE;
    if ((a->flags & need) != need)
        return fail(MMDX_ERR_INVALID_ARGUMENT, "the select form of a blend call takes device operands only: pass MMDX_TIMES_ON_DEVICE | "
                                               "MMDX_OUT_ON_DEVICE");
    if (mmdx_status r = blend_check_operands(set, bone_side, a)) return r;
    return check_instance_list(sel, a->n_instances, "the calls without _select evaluate every instance", live_host);
}

// mmdx_bone_motion_in_place and _in_place_turn: the copy, with the translations of `bone` zeroed on `axes` and, for the turn form,
// its rotations replaced by {+0,+0,+0,1}
static mmdx_status bone_motion_in_place(mmdx_bone_motion_t src, uint32_t bone, uint32_t axes, bool turn, mmdx_bone_motion_t *out) {
    if (!out) return fail(MMDX_ERR_INVALID_ARGUMENT, "out_motion is NULL");
    *out = nullptr;
    if (!src) return fail(MMDX_ERR_INVALID_ARGUMENT, "motion is NULL");
    if (axes & ~uint32_t(MMDX_ROOT_X | MMDX_ROOT_Y | MMDX_ROOT_Z)) return fail(MMDX_ERR_INVALID_ARGUMENT, "unknown axes bits");
    if (bone >= src->host.nb)
        return fail(MMDX_ERR_BAD_INDEX, "bone = " + std::to_string(bone) + ": the motion is bound to " + std::to_string(src->host.nb) + " bones");
    try {
        std::unique_ptr<mmdx_bone_motion_s> m(new mmdx_bone_motion_s);
        m->host = src->host;                                 // the tables only: the copy uploads its own on first use
        for (uint32_t k = m->host.key_off[bone]; k < m->host.key_off[bone + 1]; ++k)
            for (uint32_t c = 0; c < 3; ++c)
                if (axes & (1u << c)) m->host.key_tr[size_t(k) * 4 + c] = 0.0f;
        if (turn)
            for (uint32_t k = m->host.key_off[bone]; k < m->host.key_off[bone + 1]; ++k)
                for (uint32_t c = 0; c < 4; ++c) m->host.key_rot[size_t(k) * 4 + c] = c == 3 ? 1.0f : 0.0f;
        *out = m.release();
    } catch (const std::bad_alloc &) {
        return fail(MMDX_ERR_OUT_OF_MEMORY, "host allocation failed");
    }
    return MMDX_OK;
}

extern "C" {

mmdx_status mmdx_vmd_bind_bones(mmdx_vmd_t vmd, uint32_t n_bones, const char *const *bone_names,
                                mmdx_bone_motion_t *out) {
    if (!vmd || !out || (n_bones && !bone_names)) return fail(MMDX_ERR_INVALID_ARGUMENT, "NULL argument");
    *out = nullptr;
    try {
        std::unique_ptr<mmdx_bone_motion_s> m(new mmdx_bone_motion_s);
        const VmdBoneTracks t = vmd_bone_tracks(vmd);
        build_bone_motion(*t.names, *t.off, t.keys, n_bones, bone_names, m->host);
        *out = m.release();
    } catch (const std::bad_alloc &) {
        return fail(MMDX_ERR_OUT_OF_MEMORY, "host allocation failed");
    }
    return MMDX_OK;
}

mmdx_status mmdx_bone_motion_get_info(mmdx_bone_motion_t m, uint32_t *n_bones, uint32_t *n_mapped,
                                      uint32_t *n_keys, uint32_t *n_curves) {
    if (!m) return fail(MMDX_ERR_INVALID_ARGUMENT, "NULL argument");
    if (n_bones) *n_bones = m->host.nb;
    if (n_mapped) *n_mapped = m->host.n_mapped;
    if (n_keys) *n_keys = uint32_t(m->host.key_frame.size());
    if (n_curves) *n_curves = uint32_t(m->host.lut.size() / kCurveSamples);
    return MMDX_OK;
}

mmdx_status mmdx_bone_motion_eval(mmdx_bone_motion_t m, mmdx_model_t model, uint32_t n_instances,
                                  const uint32_t *frames, uint32_t flags, float *out_poses) {
    return bone_motion_eval(m, model, n_instances, frames, false, flags, out_poses);
}

mmdx_status mmdx_bone_motion_eval_time(mmdx_bone_motion_t m, mmdx_model_t model, uint32_t n_instances,
                                       const double *times, uint32_t flags, float *out_poses) {
    if (!m || !times || !out_poses || !n_instances)              // ahead of check_time_args, which reads `times`
        return fail(MMDX_ERR_INVALID_ARGUMENT, "NULL argument or n_instances == 0");
    if (mmdx_status r = check_time_args(times, n_instances, flags, MMDX_TIMES_ON_DEVICE | MMDX_OUT_ON_DEVICE)) return r;
    return bone_motion_eval(m, model, n_instances, times, true, flags, out_poses);
}

mmdx_status mmdx_bone_motion_in_place(mmdx_bone_motion_t src, uint32_t bone, uint32_t axes, mmdx_bone_motion_t *out) {
    return bone_motion_in_place(src, bone, axes, false, out);
}

mmdx_status mmdx_bone_motion_in_place_turn(mmdx_bone_motion_t src, uint32_t bone, uint32_t axes, mmdx_bone_motion_t *out) {
    return bone_motion_in_place(src, bone, axes, true, out);
}

mmdx_status mmdx_bone_motion_get_keys(mmdx_bone_motion_t m, mmdx_bone_motion_keys *out) {
    if (!m || !out || out->struct_size != sizeof(mmdx_bone_motion_keys))
        return fail(MMDX_ERR_INVALID_ARGUMENT, "NULL argument or mmdx_bone_motion_keys.struct_size mismatch");
    const BoneMotionHost &h = m->host;
    out->n_bones = h.nb;
    out->n_keys = uint32_t(h.key_frame.size());
    out->n_curves = uint32_t(h.lut.size() / kCurveSamples);
    out->key_off = h.key_off.data();
    out->key_frame = h.key_frame.data();
    out->key_tr = h.key_tr.data();
    out->key_rot = h.key_rot.data();
    out->key_curve = h.key_curve.data();
    out->lut = h.lut.data();
    return MMDX_OK;
}

void mmdx_bone_motion_destroy(mmdx_bone_motion_t m) {
    if (!m) return;
    graph_drop_handle(&m->pin);
    if (m->device >= 0) (void)hipSetDevice(m->device);
    release(m->all());
    delete m;
}

mmdx_status mmdx_skeleton_create(const mmdx_skeleton_desc *desc, mmdx_skeleton_t *out) {
    if (!desc || !out || desc->struct_size != sizeof(mmdx_skeleton_desc))
        return fail(MMDX_ERR_INVALID_ARGUMENT, "NULL argument or mmdx_skeleton_desc.struct_size mismatch");
    *out = nullptr;
    if (desc->create_flags & ~uint32_t(MMDX_SKELETON_PHYSICS_SEAM))
        return fail(MMDX_ERR_INVALID_ARGUMENT, "unknown bits in mmdx_skeleton_desc.create_flags");
    try {
        std::unique_ptr<mmdx_skeleton_s> s(new mmdx_skeleton_s);
        std::string err;
        if (mmdx_status st = build_skeleton(*desc, s->plan, err)) return fail(st, "skeleton: " + err);
        *out = s.release();
    } catch (const std::bad_alloc &) {
        return fail(MMDX_ERR_OUT_OF_MEMORY, "host allocation failed");
    }
    return MMDX_OK;
}

mmdx_status mmdx_skeleton_get_info(mmdx_skeleton_t s, mmdx_skeleton_info *info) {
    if (!s || !info || info->struct_size != sizeof(mmdx_skeleton_info))
        return fail(MMDX_ERR_INVALID_ARGUMENT, "NULL argument or mmdx_skeleton_info.struct_size mismatch");
    info->n_bones = s->plan.nb;
    info->n_pre_physics = s->plan.n_pre;
    info->n_post_physics = s->plan.n_post;
    info->max_chain = s->plan.max_chain;
    info->solver = s->plan.serial ? MMDX_SOLVER_SERIAL : MMDX_SOLVER_PARALLEL_FK;
    info->n_ik_bones = s->plan.n_ik;
    info->n_ik_links = s->plan.n_links;
    info->n_append_bones = s->plan.n_append;
    info->n_bone_morph_entries = uint32_t(s->plan.apps.size());
    info->n_solve_rounds = uint32_t(s->plan.rounds.size());
    info->n_ik_rounds_16_lanes = 0;
    for (uint8_t c : s->plan.round_coop) info->n_ik_rounds_16_lanes += (c && !s->plan.nested_ik) ? 1u : 0u;
    return MMDX_OK;
}

// a mask row of mmdx_pose_blend from the hierarchy (bone_mask.hpp): host only, no device
mmdx_status mmdx_skeleton_subtree_mask(mmdx_skeleton_t s, uint32_t n_roots, const uint32_t *roots, float inside, float outside,
                                       float *out_mask) {
    if (!s || !out_mask || (n_roots && !roots)) return fail(MMDX_ERR_INVALID_ARGUMENT, "skeleton / out_mask / roots is NULL");
    const int64_t bad = subtree_mask(s->plan.parent.data(), s->plan.nb, roots, n_roots, inside, outside, out_mask);
    if (bad >= 0)
        return fail(MMDX_ERR_BAD_INDEX, "roots[" + std::to_string(bad) + "] = " + std::to_string(roots[bad]) + " is not a bone of the skeleton (" +
                                        std::to_string(s->plan.nb) + " bones)");
    return MMDX_OK;
}

mmdx_status mmdx_debug_last_solve_shape(mmdx_skeleton_t s, mmdx_debug_solve_shape *out) {
    if (!s || !out) return fail(MMDX_ERR_INVALID_ARGUMENT, "NULL argument");
    if (out->struct_size != sizeof(mmdx_debug_solve_shape))
        return fail(MMDX_ERR_INVALID_ARGUMENT, "mmdx_debug_solve_shape.struct_size mismatch");
    const SolveShape &l = s->last_solve;
    *out = mmdx_debug_solve_shape{sizeof(mmdx_debug_solve_shape), l.solver, l.nested, l.dense, l.select, l.workgroups, l.lds,
                                  l.segments, l.coop_launches, 0u};
    return MMDX_OK;
}

void mmdx_skeleton_destroy(mmdx_skeleton_t s) {
    if (!s) return;
    graph_drop_handle(&s->pin);
    if (s->device >= 0) (void)hipSetDevice(s->device);
    release(s->all());
    delete s;
}

mmdx_status mmdx_skeleton_solve_motion(mmdx_skeleton_t s, mmdx_bone_motion_t m, mmdx_model_t model, uint32_t n_instances,
                                       const uint32_t *frames, uint32_t flags, float *out_palettes) {
    return skeleton_solve_motion(s, m, model, n_instances, frames, false, flags, out_palettes);
}

mmdx_status mmdx_skeleton_solve_motion_time(mmdx_skeleton_t s, mmdx_bone_motion_t m, mmdx_model_t model, uint32_t n_instances,
                                            const double *times, uint32_t flags, float *out_palettes) {
    if (!s || !m || !times || !out_palettes || !n_instances)     // ahead of check_time_args, which reads `times`
        return fail(MMDX_ERR_INVALID_ARGUMENT, "NULL argument or n_instances == 0");
    if (mmdx_status r = check_time_args(times, n_instances, flags, MMDX_TIMES_ON_DEVICE | MMDX_OUT_ON_DEVICE)) return r;
    return skeleton_solve_motion(s, m, model, n_instances, times, true, flags, out_palettes);
}

mmdx_status mmdx_skeleton_solve(mmdx_skeleton_t s, mmdx_model_t model, uint32_t n_instances, const float *poses,
                                uint32_t flags, float *out_palettes) {
    return mmdx_skeleton_solve_morphed(s, model, n_instances, poses, nullptr, flags, out_palettes);
}

mmdx_status mmdx_skeleton_solve_morphed(mmdx_skeleton_t s, mmdx_model_t model, uint32_t n_instances,
                                        const float *poses, const float *morph_weights, uint32_t flags,
                                        float *out_palettes) {
    return skeleton_solve(s, model, n_instances, poses, morph_weights, flags, out_palettes, 3u, nullptr);
}

mmdx_status mmdx_skeleton_solve_select(mmdx_skeleton_t s, mmdx_model_t model, uint32_t n_instances, const float *poses,
                                       const float *morph_weights, uint32_t flags, const mmdx_instance_select *select,
                                       float *out_palettes) {
    uint32_t live_host = 0;
    if (mmdx_status r = check_select_args(s, n_instances, poses, morph_weights, flags, select, out_palettes, live_host)) return r;
    int device;
    hipStream_t st;
    if (mmdx_status r = resolve_stream(model, &device, &st)) return r;
    if (mmdx_status r = refuse_recording(0, 0, device, {s->device},
                                         "while a graph is being recorded the skeleton must have run on this device before"))
        return r;
    if (mmdx_status r = skeleton_to_device(s, device)) return r;
    graph_note_handle(model, &s->pin);
    InstanceList list;
    uint32_t cells;
    if (mmdx_status r = list_in(s->sel_in, s->sel_host, select, n_instances, live_host, st, &list, &cells)) return r;
    if (cells == 0) return MMDX_OK;                                 // an empty list writes nothing
    const float *rates = s->plan.apps.empty() ? nullptr : morph_weights;
    if (mmdx_status r = solve_on_device(s, cells, &list, poses, rates, (flags & MMDX_WEIGHTS_SHARED) != 0, out_palettes, 3u, st)) return r;
    // results on the device: waits when the list was borrowed -- it is consumed then, and the results are there
    return finish(flags, !(select->flags & MMDX_SELECT_ON_DEVICE), st, OutRoute{});
}

mmdx_status mmdx_skeleton_solve_pre(mmdx_skeleton_t s, mmdx_model_t model, uint32_t n_instances, const float *poses,
                                    const float *morph_weights, uint32_t flags, float *out_palettes) {
    if (s && !s->plan.serial)
        return fail(MMDX_ERR_INVALID_ARGUMENT, "mmdx_skeleton_solve_pre needs a skeleton created with MMDX_SKELETON_PHYSICS_SEAM");
    return skeleton_solve(s, model, n_instances, poses, morph_weights, flags, out_palettes, 1u, nullptr);
}

mmdx_status mmdx_skeleton_solve_post(mmdx_skeleton_t s, mmdx_model_t model, uint32_t n_instances,
                                     const mmdx_physics_overrides *ov, uint32_t flags, float *out_palettes) {
    if (s && !s->plan.serial)
        return fail(MMDX_ERR_INVALID_ARGUMENT, "mmdx_skeleton_solve_post needs a skeleton created with MMDX_SKELETON_PHYSICS_SEAM");
    if (s && (!s->pre_instances || s->pre_instances != n_instances))
        return fail(MMDX_ERR_INVALID_ARGUMENT, "mmdx_skeleton_solve_post without a matching mmdx_skeleton_solve_pre");
    if (ov) {
        if (ov->struct_size != sizeof(mmdx_physics_overrides))
            return fail(MMDX_ERR_INVALID_ARGUMENT, "mmdx_physics_overrides.struct_size mismatch");
        if (ov->n_bones && (!ov->bone || !ov->skinning)) return fail(MMDX_ERR_INVALID_ARGUMENT, "overrides: bone / skinning is NULL");
        for (uint32_t k = 0; s && k < ov->n_bones; ++k)
            if (ov->bone[k] < 0 || uint32_t(ov->bone[k]) >= s->plan.nb)
                return fail(MMDX_ERR_BAD_INDEX, "overrides: bone " + std::to_string(ov->bone[k]) + " out of range");
    }
    return skeleton_solve(s, model, n_instances, nullptr, nullptr, flags, out_palettes, 2u, ov);
}

mmdx_status mmdx_motion_set_create(uint32_t n_clips, const mmdx_bone_motion_t *bone_motions, const mmdx_morph_motion_t *morph_motions,
                                   mmdx_motion_set_t *out) {
    if (!out) return fail(MMDX_ERR_INVALID_ARGUMENT, "NULL argument");
    *out = nullptr;
    if (!n_clips || (!bone_motions && !morph_motions))
        return fail(MMDX_ERR_INVALID_ARGUMENT, "a motion set needs at least one clip and at least one of bone_motions / morph_motions");
    for (uint32_t c = 0; c < n_clips; ++c)
        if ((bone_motions && !bone_motions[c]) || (morph_motions && !morph_motions[c]))
            return fail(MMDX_ERR_INVALID_ARGUMENT, "clip " + std::to_string(c) + " is NULL");
    try {
        std::unique_ptr<mmdx_motion_set_s> set(new mmdx_motion_set_s);
        set->host.n_clips = n_clips;
        std::string err;
        if (bone_motions) {
            std::vector<const BoneMotionHost *> clips;
            for (uint32_t c = 0; c < n_clips; ++c) clips.push_back(&bone_motions[c]->host);
            if (mmdx_status st = build_motion_set_bones(clips, set->host, err)) return fail(st, "motion set: " + err);
        }
        if (morph_motions) {
            std::vector<MorphMotionHost> clips;
            for (uint32_t c = 0; c < n_clips; ++c) clips.push_back(morph_motion_host(morph_motions[c]));
            if (mmdx_status st = build_motion_set_morphs(clips, set->host, err)) return fail(st, "motion set: " + err);
        }
        set->clip_frames = motion_set_last_frames(set->host);
        *out = set.release();
    } catch (const std::bad_alloc &) {
        return fail(MMDX_ERR_OUT_OF_MEMORY, "host allocation failed");
    }
    return MMDX_OK;
}

mmdx_status mmdx_motion_set_get_info(mmdx_motion_set_t set, mmdx_motion_set_info *info) {
    if (!set || !info || info->struct_size != sizeof(mmdx_motion_set_info))
        return fail(MMDX_ERR_INVALID_ARGUMENT, "NULL argument or mmdx_motion_set_info.struct_size mismatch");
    const MotionSetHost &h = set->host;
    info->n_clips = h.n_clips;
    info->n_bones = h.has_bones ? h.bones.nb : 0;
    info->n_morphs = h.has_morphs ? h.nm : 0;
    info->n_bone_keys = uint32_t(h.bones.key_frame.size());
    info->n_morph_keys = uint32_t(h.morph_frames.size());
    info->n_curves = uint32_t(h.bones.lut.size() / kCurveSamples);
    return MMDX_OK;
}

void mmdx_motion_set_destroy(mmdx_motion_set_t set) {
    if (!set) return;
    graph_drop_handle(&set->pin);
    if (set->device >= 0) (void)hipSetDevice(set->device);
    release(set->all());
    delete set;
}

mmdx_status mmdx_motion_set_eval_bones(mmdx_motion_set_t set, mmdx_model_t model, uint32_t n_instances, const uint32_t *clips,
                                       const uint32_t *frames, uint32_t flags, float *out_poses) {
    return set_eval_bones(set, model, n_instances, clips, frames, false, flags, out_poses);
}

mmdx_status mmdx_motion_set_eval_bones_time(mmdx_motion_set_t set, mmdx_model_t model, uint32_t n_instances, const uint32_t *clips,
                                            const double *times, uint32_t flags, float *out_poses) {
    return set_eval_bones(set, model, n_instances, clips, times, true, flags, out_poses);
}

mmdx_status mmdx_motion_set_eval_morphs(mmdx_motion_set_t set, mmdx_model_t model, uint32_t n_instances, const uint32_t *clips,
                                        const uint32_t *frames, uint32_t flags, float *out_weights) {
    return set_eval_morphs(set, model, n_instances, clips, frames, false, flags, out_weights);
}

mmdx_status mmdx_motion_set_eval_morphs_time(mmdx_motion_set_t set, mmdx_model_t model, uint32_t n_instances, const uint32_t *clips,
                                             const double *times, uint32_t flags, float *out_weights) {
    return set_eval_morphs(set, model, n_instances, clips, times, true, flags, out_weights);
}

mmdx_status mmdx_skeleton_solve_motion_set(mmdx_skeleton_t s, mmdx_motion_set_t set, mmdx_model_t model, uint32_t n_instances,
                                           const uint32_t *clips, const uint32_t *frames, uint32_t flags, float *out_palettes) {
    return skeleton_solve_motion_set(s, set, model, n_instances, clips, frames, false, flags, out_palettes);
}

mmdx_status mmdx_skeleton_solve_motion_set_time(mmdx_skeleton_t s, mmdx_motion_set_t set, mmdx_model_t model, uint32_t n_instances,
                                                const uint32_t *clips, const double *times, uint32_t flags, float *out_palettes) {
    return skeleton_solve_motion_set(s, set, model, n_instances, clips, times, true, flags, out_palettes);
}

mmdx_status mmdx_motion_set_blend_bones_time(mmdx_motion_set_t set, mmdx_model_t model, const mmdx_motion_blend_args *args,
                                             float *out_poses) {
    if (mmdx_status r = blend_check_args(set, true, args, out_poses)) return r;
    int device;
    hipStream_t st;
    if (mmdx_status r = resolve_stream(model, &device, &st)) return r;
    if (mmdx_status r = refuse_recording(args->flags, kClockAndOut, device, {set->device}, kSetRecording)) return r;
    if (mmdx_status r = set_to_device(set, device)) return r;
    graph_note_handle(model, &set->pin);
    BoneTrackParams p = set->t.params(set->host.bones.nb, args->n_instances);
    BlendOperands ops;
    if (mmdx_status r = blend_operands_in(set, args, st, &ops)) return r;
    OutRoute o;
    if (mmdx_status r = route_out(args->flags, out_poses, pose_bytes(args->n_instances, p.nb), set->out, &o)) return r;
    p.out = o.dev;
    HIP_TRY(launch_bone_track_blend_set(p, ops, st));
    return finish(args->flags, !(args->flags & MMDX_TIMES_ON_DEVICE), st, o);
}

mmdx_status mmdx_motion_set_blend_morphs_time(mmdx_motion_set_t set, mmdx_model_t model, const mmdx_motion_blend_args *args,
                                              float *out_weights) {
    if (mmdx_status r = blend_check_args(set, false, args, out_weights)) return r;
    int device;
    hipStream_t st;
    if (mmdx_status r = resolve_stream(model, &device, &st)) return r;
    if (mmdx_status r = refuse_recording(args->flags, kClockAndOut, device, {set->device}, kSetRecording)) return r;
    if (mmdx_status r = set_to_device(set, device)) return r;
    graph_note_handle(model, &set->pin);
    MorphTrackParams t = set_morph_params(set, args->n_instances);
    BlendOperands ops;
    if (mmdx_status r = blend_operands_in(set, args, st, &ops)) return r;
    OutRoute o;
    if (mmdx_status r = route_out(args->flags, out_weights, size_t(args->n_instances) * t.nm * sizeof(float), set->out, &o)) return r;
    t.out = o.dev;
    HIP_TRY(launch_morph_track_blend_set(t, ops, st));
    return finish(args->flags, !(args->flags & MMDX_TIMES_ON_DEVICE), st, o);
}

mmdx_status mmdx_skeleton_solve_motion_set_blend_time(mmdx_skeleton_t s, mmdx_motion_set_t set, mmdx_model_t model,
                                                      const mmdx_motion_blend_args *args, float *out_palettes) {
    if (!s) return fail(MMDX_ERR_INVALID_ARGUMENT, "NULL argument");
    if (mmdx_status r = blend_check_args(set, true, args, out_palettes)) return r;
    if (mmdx_status r = skeleton_matches_set(s, set)) return r;
    int device;
    hipStream_t st;
    if (mmdx_status r = resolve_stream(model, &device, &st)) return r;
    const SkeletonPlan &pl = s->plan;
    const uint32_t ni = args->n_instances;
    if (two_launches(pl)) {                                         // the blend track call, then the solve
        float *poses;
        if (mmdx_status r = set_pose_scratch(set, device, pose_bytes(ni, pl.nb), &poses)) return r;
        mmdx_motion_blend_args to_scratch = *args;
        to_scratch.flags = (args->flags & MMDX_TIMES_ON_DEVICE) | MMDX_OUT_ON_DEVICE;
        if (mmdx_status r = mmdx_motion_set_blend_bones_time(set, model, &to_scratch, poses)) return r;
        return mmdx_skeleton_solve(s, model, ni, poses, MMDX_POSES_ON_DEVICE | (args->flags & MMDX_OUT_ON_DEVICE), out_palettes);
    }
    if (mmdx_status r = refuse_recording(args->flags, kClockAndOut, device, {set->device, s->device}, kSetSkeletonRecording)) return r;
    if (mmdx_status r = set_to_device(set, device)) return r;
    if (mmdx_status r = skeleton_to_device(s, device)) return r;
    graph_note_handle(model, &set->pin);
    graph_note_handle(model, &s->pin);
    const BoneTrackParams tp = set->t.params(pl.nb, ni);
    BlendOperands ops;
    if (mmdx_status r = blend_operands_in(set, args, st, &ops)) return r;
    OutRoute o;
    if (mmdx_status r = route_out(args->flags, out_palettes, palette_bytes(ni, pl.nb), s->out, &o)) return r;
    HIP_TRY(launch_motion_fk_blend_set(tp, fk_params(s, ni, nullptr, nullptr, o.dev), ops, st));
    note_fk_solve(s);
    return finish(args->flags, !(args->flags & MMDX_TIMES_ON_DEVICE), st, o);
}

// ---- the cross-fade for the listed instances: device operands and output; a borrowed host list is waited for at the end -----------
mmdx_status mmdx_motion_set_blend_bones_time_select(mmdx_motion_set_t set, mmdx_model_t model, const mmdx_motion_blend_args *args,
                                                    const mmdx_instance_select *select, float *out_poses) {
    uint32_t live_host = 0;
    if (mmdx_status r = blend_select_check(set, true, args, select, out_poses, live_host)) return r;
    int device;
    hipStream_t st;
    if (mmdx_status r = resolve_stream(model, &device, &st)) return r;
    if (mmdx_status r = refuse_recording(0, 0, device, {set->device}, kSetRecording)) return r;
    if (mmdx_status r = set_to_device(set, device)) return r;
    graph_note_handle(model, &set->pin);
    InstanceList list;
    uint32_t cells;
    if (mmdx_status r = list_in(set->sel_in, set->sel_host, select, args->n_instances, live_host, st, &list, &cells)) return r;
    if (cells == 0) return MMDX_OK;                                 // an empty list writes nothing
    BoneTrackParams p = set->t.params(set->host.bones.nb, cells);
    p.out = out_poses;
    HIP_TRY(launch_bone_track_blend_set_select(p, blend_operands_device(set, args), list, st));
    return finish(args->flags, !(select->flags & MMDX_SELECT_ON_DEVICE), st, OutRoute{});
}

mmdx_status mmdx_motion_set_blend_morphs_time_select(mmdx_motion_set_t set, mmdx_model_t model, const mmdx_motion_blend_args *args,
                                                     const mmdx_instance_select *select, float *out_weights) {
    uint32_t live_host = 0;
    if (mmdx_status r = blend_select_check(set, false, args, select, out_weights, live_host)) return r;
    int device;
    hipStream_t st;
    if (mmdx_status r = resolve_stream(model, &device, &st)) return r;
    if (mmdx_status r = refuse_recording(0, 0, device, {set->device}, kSetRecording)) return r;
    if (mmdx_status r = set_to_device(set, device)) return r;
    graph_note_handle(model, &set->pin);
    InstanceList list;
    uint32_t cells;
    if (mmdx_status r = list_in(set->sel_in, set->sel_host, select, args->n_instances, live_host, st, &list, &cells)) return r;
    if (cells == 0) return MMDX_OK;
    MorphTrackParams t = set_morph_params(set, cells);
    t.out = out_weights;
    HIP_TRY(launch_morph_track_blend_set_select(t, blend_operands_device(set, args), list, st));
    return finish(args->flags, !(select->flags & MMDX_SELECT_ON_DEVICE), st, OutRoute{});
}

mmdx_status mmdx_skeleton_solve_motion_set_blend_time_select(mmdx_skeleton_t s, mmdx_motion_set_t set, mmdx_model_t model,
                                                             const mmdx_motion_blend_args *args, const mmdx_instance_select *select,
                                                             float *out_palettes) {
    if (!s) return fail(MMDX_ERR_INVALID_ARGUMENT, "NULL argument");
    uint32_t live_host = 0;
    if (mmdx_status r = blend_select_check(set, true, args, select, out_palettes, live_host)) return r;
    if (mmdx_status r = skeleton_matches_set(s, set)) return r;
    int device;
    hipStream_t st;
    if (mmdx_status r = resolve_stream(model, &device, &st)) return r;
    const SkeletonPlan &pl = s->plan;
    const uint32_t ni = args->n_instances;
    if (two_launches(pl)) {
        // the blend select into the set's pose scratch -- [NI] rows, addressed by id -- then the select solve with the same list
        float *poses;
        if (mmdx_status r = set_pose_scratch(set, device, pose_bytes(ni, pl.nb), &poses)) return r;
        if (mmdx_status r = mmdx_motion_set_blend_bones_time_select(set, model, args, select, poses)) return r;
        return mmdx_skeleton_solve_select(s, model, ni, poses, nullptr, MMDX_POSES_ON_DEVICE | MMDX_OUT_ON_DEVICE, select, out_palettes);
    }
    if (mmdx_status r = refuse_recording(0, 0, device, {set->device, s->device}, kSetSkeletonRecording)) return r;
    if (mmdx_status r = set_to_device(set, device)) return r;
    if (mmdx_status r = skeleton_to_device(s, device)) return r;
    graph_note_handle(model, &set->pin);
    graph_note_handle(model, &s->pin);
    InstanceList list;
    uint32_t cells;
    if (mmdx_status r = list_in(set->sel_in, set->sel_host, select, ni, live_host, st, &list, &cells)) return r;
    if (cells == 0) return MMDX_OK;
    const BoneTrackParams tp = set->t.params(pl.nb, cells);
    HIP_TRY(launch_motion_fk_blend_set_select(tp, fk_params(s, cells, nullptr, nullptr, out_palettes), blend_operands_device(set, args), list, st));
    note_fk_solve(s);
    return finish(args->flags, !(select->flags & MMDX_SELECT_ON_DEVICE), st, OutRoute{});
}

}  // extern "C"

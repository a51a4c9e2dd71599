// clip_source.hpp -- what an instance plays: a VMD track evaluated at a clock (eval_bone_pose, eval_morph_rate) and the three sources
// every track and one-launch FK kernel draws from -- one motion, a clip of a motion set, a cross-fade of two clips.  A source is built
// from the call's operands and an instance index i, per lane or once per workgroup alike, and then yields the pose of a bone (rate
// of a morph) of that instance.  A kernel variant is two choices: which instance (instance_list.hpp) and what it plays (here).
// rig_kernels.hip and kernels.hip are both built with -ffp-contract=off: the reference's float operation order, bit for bit.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "motion_blend.hpp"
#include "motion_clock.hpp"
#include "rig.hpp"
#include "vmd.hpp"

namespace mmdx {

// Bezier<float,32>::operator[] (L/util/math_impl.inl:1379-1392): linear lookup in the presampled table.
__device__ __forceinline__ float curve_at(const float *lut, uint32_t id, float x) {
    if (id == kLinearCurve) return x;
    const float *t = lut + size_t(id) * kCurveSamples;
    x = x * float(kCurveSamples - 1);
    const uint32_t ix = uint32_t(x);
    const float r = x - float(ix);
    if (ix < kCurveSamples - 1) return (1.0f - r) * t[ix] + r * t[ix + 1];
    return t[kCurveSamples - 1];
}

// Motion::GetBonePose(name, frame), L/motion/motion_impl.inl:255-319: the local pose (translation, rotation) of one bone at one
// frame; with a TimeClock GetBonePose(name, time), :321-380 (motion_clock.hpp: the clamps, the search key, no exact-hit shortcut,
// bary in double).  The curve lookup and the NLerp are the same code for both.
template <class Clock>
__device__ __forceinline__ void eval_bone_pose(const BoneTrackParams &p, uint32_t bone, const Clock clk, float4 &t_out, float4 &q_out) {
    const uint32_t b = p.key_off[bone], e = p.key_off[bone + 1];
    const float4 *tr = reinterpret_cast<const float4 *>(p.key_tr);
    const float4 *rot = reinterpret_cast<const float4 *>(p.key_rot);
    float4 t = make_float4(0.f, 0.f, 0.f, 0.f), q = make_float4(0.f, 0.f, 0.f, 1.f);   // Poser::ResetPosing
    if (e > b) {
        if (clk.at_or_before_first(p.key_frame[b])) {
            t = tr[b]; q = rot[b];
        } else if (clk.at_or_after_last(p.key_frame[e - 1])) {
            t = tr[e - 1]; q = rot[e - 1];
        } else {
            const uint32_t frame = clk.search();
            uint32_t lo = b, hi = e - 1;                   // key_frame[lo] <= frame < key_frame[hi]
            while (hi - lo > 1) {
                const uint32_t mid = (lo + hi) / 2;
                if (p.key_frame[mid] > frame) hi = mid; else lo = mid;
            }
            const uint32_t lf = p.key_frame[lo], rf = p.key_frame[hi];
            if (clk.exact(lf)) {
                t = tr[lo]; q = rot[lo];
            } else {
                const float bary = clk.bary(lf, rf);
                const uint4 cv = reinterpret_cast<const uint4 *>(p.key_curve)[lo];   // the LEFT key's curves
                const float4 lt = tr[lo], rt = tr[hi], lq = rot[lo], rq = rot[hi];
                float lam = curve_at(p.lut, cv.x, bary);
                t.x = lt.x * (1.0f - lam) + rt.x * lam;
                lam = curve_at(p.lut, cv.y, bary);
                t.y = lt.y * (1.0f - lam) + rt.y * lam;
                lam = curve_at(p.lut, cv.z, bary);
                t.z = lt.z * (1.0f - lam) + rt.z * lam;
                lam = curve_at(p.lut, cv.w, bary);
                // NLerp(l, r)[lam], L/util/math_impl.inl:1260-1282
                if (lam < 1e-7f) {
                    q = lq;
                } else if (lam > 1.0f - 1e-7f) {
                    q = rq;
                } else {
                    const float dot = lq.x * rq.x + lq.y * rq.y + lq.z * rq.z + lq.w * rq.w;
                    const float a = 1.0f - lam;
                    float4 v;
                    if (dot < 0.0f) {
                        v = make_float4(a * lq.x - lam * rq.x, a * lq.y - lam * rq.y, a * lq.z - lam * rq.z,
                                        a * lq.w - lam * rq.w);
                    } else {
                        v = make_float4(a * lq.x + lam * rq.x, a * lq.y + lam * rq.y, a * lq.z + lam * rq.z,
                                        a * lq.w + lam * rq.w);
                    }
                    // Vector4D::Normalize: 1 / float(sqrt(double(sum))), L/util/math_impl.inl:717-728, math.inl:27-29
                    const float s = v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w;
                    const float n = 1.0f / float(sqrt(double(s)));
                    q = make_float4(v.x * n, v.y * n, v.z * n, v.w * n);
                }
            }
        }
    }
    t_out = t;
    q_out = q;
}

// Motion::GetMorphPose(name, frame), motion_impl.inl:382-424: the rate of one model morph at one frame -- clamp to the first / last
// key, exact hit, else the linear blend l*(1-t) + r*t with t = float(frame-left)/float(right-left) (IEEE division: hipcc keeps f32
// division correctly rounded by default).  A morph without a track keeps rate 0, as after ResetPosing.  With a TimeClock:
// GetMorphPose(name, double time), :426-465 (motion_clock.hpp) -- no exact-hit shortcut, so a key hit still goes through the blend
// (an infinite neighbour gives NaN there).
template <class Clock>
__device__ __forceinline__ float eval_morph_rate(const MorphTrackParams &t, uint32_t m, const Clock clk) {
    const uint32_t b = t.key_off[m], e = t.key_off[m + 1];
    float w = 0.f;
    if (e > b) {
        if (clk.at_or_before_first(t.key_frames[b])) {
            w = t.key_weights[b];
        } else if (clk.at_or_after_last(t.key_frames[e - 1])) {
            w = t.key_weights[e - 1];
        } else {
            const uint32_t frame = clk.search();
            uint32_t lo = b, hi = e - 1;               // key_frames[lo] <= frame < key_frames[hi]
            while (hi - lo > 1) {                      // first key whose frame is > `frame`
                const uint32_t mid = (lo + hi) / 2;
                if (t.key_frames[mid] > frame) hi = mid; else lo = mid;
            }
            const uint32_t lf = t.key_frames[lo], rf = t.key_frames[hi];
            if (clk.exact(lf)) {
                w = t.key_weights[lo];
            } else {
                const float bary = clk.bary(lf, rf);
                w = t.key_weights[lo] * (1.0f - bary) + t.key_weights[hi] * bary;
            }
        }
    }
    return w;
}

// Motion set (mmdx_motion_set_*): clip c of the bank is the single-motion table with key_off advanced by c * (nb+1) (morphs:
// c * (nm+1)) -- the offsets stored there are absolute into the concatenated key arrays -- so a clip goes through eval_bone_pose /
// eval_morph_rate itself.
__device__ __forceinline__ BoneTrackParams clip_of(BoneTrackParams p, uint32_t clip) {
    p.key_off += size_t(clip) * (size_t(p.nb) + 1);
    return p;
}
__device__ __forceinline__ MorphTrackParams clip_of(MorphTrackParams t, uint32_t clip) {
    t.key_off += size_t(clip) * (size_t(t.nm) + 1);
    return t;
}

// ---- poses of an instance's bones ------------------------------------------------------------------------------------------------

// one motion at the instance's clock (p.frames / p.times)
template <class Clock>
struct MotionPose {
    const BoneTrackParams &p;
    Clock clk;
    __device__ __forceinline__ MotionPose(const BoneTrackParams &p, uint32_t i) : p(p), clk(clock_of<Clock>(p.frames, p.times, i)) {}
    __device__ __forceinline__ void pose(uint32_t bone, float4 &t, float4 &q) const { eval_bone_pose(p, bone, clk, t, q); }
};

// one clip of a set at a clock.  A clip id outside [0, n_clips) (MMDX_CLIP_NONE included) plays nothing: the rest pose of
// Poser::ResetPosing, and no table is read.
template <class Clock>
struct ClipPose {
    const BoneTrackParams &p;
    uint32_t clip, n_clips;
    Clock clk;
    __device__ __forceinline__ ClipPose(const BoneTrackParams &p, uint32_t clip, uint32_t n_clips, Clock clk)
        : p(p), clip(clip), n_clips(n_clips), clk(clk) {}
    // the clip of instance i at the instance's clock (mmdx_motion_set_eval_bones*)
    __device__ __forceinline__ ClipPose(const BoneTrackParams &p, const uint32_t *clips, uint32_t n_clips, uint32_t i)
        : ClipPose(p, clips[i], n_clips, clock_of<Clock>(p.frames, p.times, i)) {}
    __device__ __forceinline__ void pose(uint32_t bone, float4 &t, float4 &q) const {
        t = make_float4(0.f, 0.f, 0.f, 0.f); q = make_float4(0.f, 0.f, 0.f, 1.f);   // Poser::ResetPosing
        if (clip < n_clips) eval_bone_pose(clip_of(p, clip), bone, clk, t, q);
    }
};

// The operand rows of instance i of a cross-fade (motion_blend.hpp), read the same way for poses and for rates: the side that is
// evaluated first is A, or B when the weight says the row is B, and only a row that blends reads B as the second side -- an end-point
// row is the set call's row bit for bit and reads nothing of the other clip, neither its id and time nor (below) its tables.
template <class Clock>
struct BlendRow {
    float w;
    bool mix;
    uint32_t clip0, clip1 = 0xFFFFFFFFu;
    Clock clk0, clk1;
    __device__ __forceinline__ BlendRow(const BlendOperands &o, uint32_t i) : w(o.weights[i]) {
        const uint32_t side = blend_side(w);
        const bool first_b = side == kBlendB;
        mix = side == kBlendMix;
        clip0 = (first_b ? o.clips_b : o.clips_a)[i];
        clk1 = clk0 = clock_of<Clock>(nullptr, first_b ? o.times_b : o.times_a, i);
        if (mix) {
            clip1 = o.clips_b[i];
            clk1 = clock_of<Clock>(nullptr, o.times_b, i);
        }
    }
};

// a cross-fade of two clips of a set, blended in registers (blend_pose)
template <class Clock>
struct BlendPose {
    const BlendRow<Clock> row;
    const ClipPose<Clock> first, second;
    __device__ __forceinline__ BlendPose(const BoneTrackParams &p, const BlendOperands &o, uint32_t i)
        : row(o, i), first(p, row.clip0, o.n_clips, row.clk0), second(p, row.clip1, o.n_clips, row.clk1) {}
    __device__ __forceinline__ void pose(uint32_t bone, float4 &t, float4 &q) const {
        first.pose(bone, t, q);
        if (row.mix) {
            float4 tb, qb;
            second.pose(bone, tb, qb);
            blend_pose(t, q, tb, qb, row.w);
        }
    }
};

// ---- rates of an instance's morphs: the same three ---------------------------------------------------------------------------------

template <class Clock>
struct MotionRate {
    const MorphTrackParams &t;
    Clock clk;
    __device__ __forceinline__ MotionRate(const MorphTrackParams &t, uint32_t i) : t(t), clk(clock_of<Clock>(t.frames, t.times, i)) {}
    __device__ __forceinline__ float rate(uint32_t m) const { return eval_morph_rate(t, m, clk); }
};

// an id outside the bank plays nothing: rate 0, no table read
template <class Clock>
struct ClipRate {
    const MorphTrackParams &t;
    uint32_t clip, n_clips;
    Clock clk;
    __device__ __forceinline__ ClipRate(const MorphTrackParams &t, uint32_t clip, uint32_t n_clips, Clock clk)
        : t(t), clip(clip), n_clips(n_clips), clk(clk) {}
    __device__ __forceinline__ ClipRate(const MorphTrackParams &t, const uint32_t *clips, uint32_t n_clips, uint32_t i)
        : ClipRate(t, clips[i], n_clips, clock_of<Clock>(t.frames, t.times, i)) {}
    __device__ __forceinline__ float rate(uint32_t m) const { return clip < n_clips ? eval_morph_rate(clip_of(t, clip), m, clk) : 0.f; }
};

template <class Clock>
struct BlendRate {
    const BlendRow<Clock> row;
    const ClipRate<Clock> first, second;
    __device__ __forceinline__ BlendRate(const MorphTrackParams &t, const BlendOperands &o, uint32_t i)
        : row(o, i), first(t, row.clip0, o.n_clips, row.clk0), second(t, row.clip1, o.n_clips, row.clk1) {}
    __device__ __forceinline__ float rate(uint32_t m) const {
        const float r = first.rate(m);
        return row.mix ? blend_rate(r, second.rate(m), row.w) : r;
    }
};

}  // namespace mmdx

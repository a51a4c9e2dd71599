// kernels_morph_track.inl -- the VMD morph-track kernels: per-instance morph rates from a motion, a motion set or a cross-fade.
// A piece of kernels.hip (included inside namespace mmdx { namespace {), in the bit-exact build only.

// ---- VMD morph tracks -> per-instance morph rates (Motion::GetMorphPose: eval_morph_rate, clip_source.hpp) ---
// One thread per (instance, model morph) -- which instance: lane_item (instance_list.hpp), every instance or the listed ones; what it
// plays: a rate source (clip_source.hpp) built per lane, a wave spans several instances.  Operand rows and the rate row by the
// instance's row.
template <class Source, class Instances, class... Operands>
__device__ __forceinline__ void morph_track_body(const MorphTrackParams &t, const Instances &sel, const Operands &...operands) {
    LaneItem it;
    if (!lane_item<kThreads>(sel, t.ni, t.nm, it)) return;
    t.out[it.at] = Source(t, operands..., it.ln.row).rate(it.item);
}

template <class Clock>
__global__ __launch_bounds__(kThreads) void morph_track_eval_kernel(const MorphTrackParams t) {
    morph_track_body<MotionRate<Clock>>(t, AllInstances{});
}

// mmdx_motion_set_eval_morphs*
template <class Clock>
__global__ __launch_bounds__(kThreads) void morph_track_eval_set_kernel(MorphTrackParams t, const uint32_t *clips, const uint32_t n_clips) {
    morph_track_body<ClipRate<Clock>>(t, AllInstances{}, clips, n_clips);
}

// mmdx_motion_set_blend_morphs_time (motion_blend.hpp)
template <class Clock>
__global__ __launch_bounds__(kThreads) void morph_track_blend_set_kernel(const MorphTrackParams t, const BlendOperands o) {
    morph_track_body<BlendRate<Clock>>(t, AllInstances{}, o);
}

// mmdx_motion_set_blend_morphs_time_select: t.ni = the list's capacity
template <class Clock>
__global__ __launch_bounds__(kThreads) void morph_track_blend_set_select_kernel(const MorphTrackParams t, const BlendOperands o,
                                                                                const InstanceList list) {
    morph_track_body<BlendRate<Clock>>(t, ListedInstances{list}, o);
}

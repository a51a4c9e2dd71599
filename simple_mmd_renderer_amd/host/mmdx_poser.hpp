// mmdx_poser.hpp -- C++ host mirror of the hot-path slice of the reference's mmd::Poser, over the C
// ABI in include/mmdx.h.  Header-only; link with libmmdx.so.  No HIP headers needed.
//
// Mirrors (reference file:line, L/ = 3rd_party/libmmd/include/mmd/):
//   mmd::Poser::pose_image, SetMorphPose, ResetPosing (rates only), Deform    L/motion/poser.inl:17-43
//   the palette hook PhysicsReactor::GetPoserBoneImage(...).skinning_matrix_   L/motion/physics.inl:32-40
//   the viewer's struct Vertex + UpdateDeformedVertices()                      main.cpp:50-54, :821-863
//   SetBonePose, PrePhysicsPosing / PostPhysicsPosing (bone solve -> palette)  L/motion/poser_impl.inl:362-394, :466-469
//   mmd::MotionPlayer(motion, poser)::SeekFrame                                L/motion/poser_impl.inl:522-548
//   the loaders' entry points (PmxReader / PmdReader / VmdReader ::Read*)      through Poser::FromFile, Motion
// Same names and argument meaning; errors surface as mmdx::Error (the reference's loaders throw
// mmd::exception, its Deform has no error path at all).
#pragma once

#include <cstdint>
#include <algorithm>
#include <cstring>
#include <memory>
#include <new>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/mmdx.h"

namespace mmdx {

struct Error : std::runtime_error {
    mmdx_status status;
    Error(mmdx_status s, const std::string &what) : std::runtime_error(what), status(s) {}
};

inline void check(mmdx_status s) {
    if (s != MMDX_OK) throw Error(s, mmdx_last_error_string());
}

struct Vector3f { float x, y, z; };                       // = mmd::Vector3f (12 bytes, packed)
struct Vertex { float pos[3]; float normal[3]; float uv[2]; };  // = main.cpp:50-54
static_assert(sizeof(Vector3f) == 12 && sizeof(Vertex) == 32, "layout");

// Flat model description the application fills once from its loader (mmd::Model getters).
struct ModelData {
    std::vector<float> positions, normals, uvs;           // [NV][3], [NV][3], [NV][2]
    std::vector<int32_t> skin_type, bone_ids;             // [NV], [NV][4]
    std::vector<float> bone_weights;                      // [NV][4]
    std::vector<int32_t> bone_parent;                     // [NB]
    std::vector<int32_t> morph_type;                      // [NM]
    std::vector<uint32_t> morph_offset, morph_index;      // [NM+1], [E]
    std::vector<float> morph_value;                       // [E][3]
    uint32_t n_vertices = 0, n_bones = 0, n_morphs = 0;
};

// Page-locked storage for the buffers handed to the deform calls, e.g.
//   std::vector<Vertex, mmdx::PinnedAllocator<Vertex>> vertices;
// (the viewer's `vertices` array of main.cpp:735): outputs in such memory are written by the kernel directly.
template <class T>
struct PinnedAllocator {
    using value_type = T;
    PinnedAllocator() = default;
    template <class U>
    PinnedAllocator(const PinnedAllocator<U> &) {}
    T *allocate(std::size_t n) {
        void *p = nullptr;
        if (mmdx_host_malloc(&p, n * sizeof(T)) != MMDX_OK) throw std::bad_alloc();
        return static_cast<T *>(p);
    }
    void deallocate(T *p, std::size_t) noexcept { (void)mmdx_host_free(p); }
    template <class U>
    bool operator==(const PinnedAllocator<U> &) const { return true; }
    template <class U>
    bool operator!=(const PinnedAllocator<U> &) const { return false; }
};

class Poser {
public:
    struct PoseImage {                                    // = mmd::Poser::PoseImage
        std::vector<Vector3f> coordinates;
        std::vector<Vector3f> normals;
    } pose_image;

    // `normalize` = run Model::Normalize's retagging, as both of the reference's readers do at load.  `extra_flags`: the engine's
    // opt-ins -- MMDX_CREATE_FAST_MATH (results within the stated tolerance instead of bit-identical), MMDX_CREATE_TILE_ORDER
    // (pose_image in the engine's vertex order: remap the index buffer once through VertexOrder()).
    explicit Poser(const ModelData &m, bool normalize = true, uint32_t extra_flags = 0)
        : nv_(m.n_vertices), nb_(m.n_bones), nm_(m.n_morphs) {
        mmdx_model_desc d;
        std::memset(&d, 0, sizeof(d));
        d.struct_size = sizeof(d);
        d.flags = (normalize ? MMDX_CREATE_NORMALIZE : 0) | extra_flags;
        d.n_vertices = nv_; d.n_bones = nb_; d.n_morphs = nm_;
        d.positions = m.positions.data(); d.normals = m.normals.data();
        d.uvs = m.uvs.empty() ? nullptr : m.uvs.data();
        d.skin_type = m.skin_type.data(); d.bone_ids = m.bone_ids.data();
        d.bone_weights = m.bone_weights.data();
        d.bone_parent = m.bone_parent.empty() ? nullptr : m.bone_parent.data();
        d.morph_type = m.morph_type.data(); d.morph_offset = m.morph_offset.data();
        d.morph_index = m.morph_index.data(); d.morph_value = m.morph_value.data();
        check(mmdx_model_create(&d, &model_));
        pose_image.coordinates.resize(nv_);
        pose_image.normals.resize(nv_);
        morph_rates_.assign(nm_, 0.0f);
        palette_.assign(size_t(nb_) * 16, 0.0f);
        for (uint32_t b = 0; b < nb_; ++b)
            for (int k = 0; k < 4; ++k) palette_[size_t(b) * 16 + k * 5] = 1.0f;
        Deform();  // the reference's constructor ends with ResetPosing(); Deform() (poser_impl.inl:126-127)
    }
    // From a .pmx / .pmd file through the bundled loaders: the GPU model AND the rig (bone solve on the
    // device, so PrePhysicsPosing() works without libmmd).  Names are kept for MotionPlayer.
    static Poser *FromFile(const std::string &path) {
        mmdx_pmx_t pmx = nullptr;
        const bool pmd = path.size() > 4 && (path.substr(path.size() - 4) == ".pmd" || path.substr(path.size() - 4) == ".PMD");
        check(pmd ? mmdx_pmd_load_file(path.c_str(), &pmx) : mmdx_pmx_load_file(path.c_str(), &pmx));
        Poser *p = nullptr;
        try {
            p = new Poser(pmx);
        } catch (...) {
            mmdx_pmx_destroy(pmx);
            throw;
        }
        mmdx_pmx_destroy(pmx);
        return p;
    }
    ~Poser() {
        if (skeleton_) mmdx_skeleton_destroy(skeleton_);
        mmdx_model_destroy(model_);
    }
    Poser(const Poser &) = delete;
    Poser &operator=(const Poser &) = delete;

    void ResetPosing() {
        std::fill(morph_rates_.begin(), morph_rates_.end(), 0.0f);
        for (uint32_t b = 0; b < uint32_t(bone_poses_.size() / 8); ++b) {
            float *q = bone_poses_.data() + size_t(b) * 8;
            q[0] = q[1] = q[2] = q[3] = q[4] = q[5] = q[6] = 0.0f; q[7] = 1.0f;
        }
        if (skeleton_) { PrePhysicsPosing(); PostPhysicsPosing(); }       // as the reference does (:138-139)
    }
    void SetMorphPose(size_t index, float weight) { morph_rates_.at(index) = weight; }
    // = Poser::SetBonePose(index, Motion::BonePose(translation, rotation)); quaternion x, y, z, w
    void SetBonePose(size_t index, const float translation[3], const float rotation[4]) {
        float *q = bone_poses_.data() + index * 8;
        if (index * 8 + 8 > bone_poses_.size()) throw Error(MMDX_ERR_BAD_INDEX, "SetBonePose: bone index out of range");
        std::memcpy(q, translation, 12); q[3] = 0.0f; std::memcpy(q + 4, rotation, 16);
    }
    // Bone solve on the device (bone morphs, append bones, IK incl. nested IK): local poses -> skinning matrices, in the
    // reference's two steps (main.cpp:1801-1810).  Only for posers that own a rig (FromFile).  PrePhysicsPosing() runs
    // the pre-physics bone list; SkinningMatrix(b) of those bones is then what a reactor's kinematic bodies read
    // (PoserMotionState::Reset).  A reactor hands the transforms of the bodies it moved to SetPhysicsTransforms() --
    // what PoserMotionState::Synchronize() writes, with `strict` marking the bodies Fix() applies to
    // (mmd-bullet_impl.inl:34-56) -- and PostPhysicsPosing() applies them and runs the post-physics list.
    void PrePhysicsPosing() {
        if (!skeleton_) throw Error(MMDX_ERR_UNSUPPORTED, "this Poser has no rig: fill SkinningMatrix() yourself");
        check(mmdx_skeleton_solve_pre(skeleton_, model_, 1, bone_poses_.data(), nm_ ? morph_rates_.data() : nullptr,
                                      MMDX_WEIGHTS_SHARED, palette_.data()));
        physics_bones_.clear(); physics_strict_.clear(); physics_skinning_.clear();
        post_pending_ = true;       // the rows of the post-physics bones are unspecified until PostPhysicsPosing()
    }
    void SetPhysicsTransforms(const std::vector<int32_t> &bones, const std::vector<uint8_t> &strict,
                              const float *skinning /*[bones.size()][16]*/) {
        physics_bones_ = bones;
        physics_strict_ = strict;
        physics_strict_.resize(bones.size(), 0);
        physics_skinning_.assign(skinning, skinning + bones.size() * 16);
    }
    void PostPhysicsPosing() {
        if (!skeleton_) throw Error(MMDX_ERR_UNSUPPORTED, "this Poser has no rig: fill SkinningMatrix() yourself");
        mmdx_physics_overrides ov;
        ov.struct_size = sizeof(ov);
        ov.n_bones = uint32_t(physics_bones_.size());
        ov.bone = physics_bones_.data(); ov.strict = physics_strict_.data(); ov.skinning = physics_skinning_.data();
        check(mmdx_skeleton_solve_post(skeleton_, model_, 1, ov.n_bones ? &ov : nullptr, 0, palette_.data()));
        post_pending_ = false;
    }

    // original_to_engine[file vertex] = its position in pose_image of an MMDX_CREATE_TILE_ORDER poser (what the viewer's index
    // buffer is remapped through, main.cpp:781-787); the identity-free inverse comes back in engine_to_original if asked for.
    std::vector<uint32_t> VertexOrder(std::vector<uint32_t> *engine_to_original = nullptr) const {
        std::vector<uint32_t> o2e(nv_);
        if (engine_to_original) engine_to_original->resize(nv_);
        check(mmdx_model_get_vertex_order(model_, engine_to_original ? engine_to_original->data() : nullptr, o2e.data()));
        return o2e;
    }

    const std::vector<std::string> &bone_names() const { return bone_names_; }
    const std::vector<std::string> &morph_names() const { return morph_names_; }
    std::vector<float> &morph_rates() { return morph_rates_; }
    std::vector<float> &bone_poses() { return bone_poses_; }      // [NB][8]: t.xyz, 0, q.xyzw

    // What a PhysicsReactor-derived tap reads out of the reference Poser after PostPhysicsPosing():
    // float[16], row-vector convention, translation in elements 12..14.
    // (Between PrePhysicsPosing() and PostPhysicsPosing() only the pre-physics bones' matrices are valid -- what a reactor's
    // kinematic bodies read; the frame's palette is final after PostPhysicsPosing(), as in the reference, main.cpp:1810.)
    float *SkinningMatrix(size_t bone) { return palette_.data() + bone * 16; }
    void SetSkinningMatrices(const float *palette /*[NB][16]*/) {
        std::memcpy(palette_.data(), palette, palette_.size() * sizeof(float));
        post_pending_ = false;      // the caller supplied the whole palette
    }

    void Deform() {
        require_final_palette();
        check(mmdx_deform(model_, morph_rates_.data(), palette_.data(),
                          reinterpret_cast<float *>(pose_image.coordinates.data()),
                          reinterpret_cast<float *>(pose_image.normals.data())));
    }

    // Deform + repack in ONE pass on the GPU: replaces main.cpp:1821 and :1824 together.  With a vector on
    // PinnedAllocator (below) the kernel stores the vertices straight into it; a plain vector goes through the
    // library's bounce buffer (one extra CPU copy).
    template <class Alloc>
    void UpdateDeformedVertices(std::vector<Vertex, Alloc> &vertices, float mmd_to_meter = 0.1f) {
        vertices.resize(nv_);
        require_final_palette();
        check(mmdx_deform_vertex32(model_, morph_rates_.data(), palette_.data(), mmd_to_meter,
                                   vertices.data()));
    }

    // Culling and LOD of a crowd of this model on the device (mmdx.h, mmdx_cull_bounds): the boxes a mmdx_deform_batched_bounds call
    // on handle() left in device memory against the planes and LOD distances of `view`; list l (visible instances of level l, ascending)
    // goes to ids_dev + l * list_stride, its length to counts_dev[l] -- what mmdx_instance_select.ids / .count take.  A view in host
    // memory is validated and passed by value; with view_on_device it is read when the kernel runs (a recorded call: at every replay).
    // Asynchronous on the model's stream.  list_stride 0 = n_instances.
    void CullBounds(const float *bounds_dev, uint32_t n_instances, const mmdx_cull_view *view, bool view_on_device, uint32_t *ids_dev,
                    uint32_t *counts_dev, uint32_t *levels_dev = nullptr, uint32_t list_stride = 0) {
        mmdx_cull_args a{};
        a.struct_size = sizeof(a);
        a.flags = view_on_device ? uint32_t(MMDX_CULL_VIEW_ON_DEVICE) : 0u;
        a.n_instances = n_instances;
        a.list_stride = list_stride ? list_stride : n_instances;
        a.bounds = bounds_dev; a.view = view;
        a.out_ids = ids_dev; a.out_counts = counts_dev; a.out_levels = levels_dev;
        check(mmdx_cull_bounds(model_, &a));
    }
    // The six planes (left, right, bottom, top, near, far) of a column-major view-projection matrix, e.g. &HMM_Mat4.Elements[0][0]
    static void PlanesFromMatrix(const float m[16], bool depth_zero_to_one, float out_planes[6][4]) {
        check(mmdx_cull_planes_from_matrix(m, depth_zero_to_one ? 1u : 0u, out_planes));
    }

    mmdx_model_t handle() const { return model_; }
    mmdx_skeleton_t skeleton() const { return skeleton_; }
    uint32_t vertex_count() const { return nv_; }
    uint32_t bone_count() const { return nb_; }
    uint32_t morph_count() const { return nm_; }

private:
    // Until round 2 PrePhysicsPosing() solved both bone lists; since the physics seam it solves the pre-physics list only.  A
    // host that still calls PrePhysicsPosing() and then deforms would skin with unspecified rows for the post-physics bones:
    // refuse loudly instead.
    void require_final_palette() const {
        if (post_pending_)
            throw Error(MMDX_ERR_INVALID_ARGUMENT, "Deform() after PrePhysicsPosing() without PostPhysicsPosing(): the post-physics "
                                                   "bones' skinning matrices are not solved yet (main.cpp:1801-1810 calls both)");
    }
    bool post_pending_ = false;

    explicit Poser(mmdx_pmx_t pmx) {
        mmdx_model_desc d;
        check(mmdx_pmx_get_model_desc(pmx, &d));
        nv_ = d.n_vertices; nb_ = d.n_bones; nm_ = d.n_morphs;
        check(mmdx_model_create(&d, &model_));
        mmdx_skeleton_desc sd;
        check(mmdx_pmx_get_skeleton_desc(pmx, &sd));
        sd.create_flags |= MMDX_SKELETON_PHYSICS_SEAM;      // PrePhysicsPosing | a reactor's writes | PostPhysicsPosing
        const mmdx_status st = mmdx_skeleton_create(&sd, &skeleton_);
        if (st != MMDX_OK) { mmdx_model_destroy(model_); throw Error(st, mmdx_last_error_string()); }
        char buf[1024];
        for (uint32_t b = 0; b < nb_; ++b) { check(mmdx_pmx_get_name(pmx, MMDX_PMX_NAME_BONE, b, buf, sizeof(buf))); bone_names_.push_back(buf); }
        for (uint32_t m = 0; m < nm_; ++m) { check(mmdx_pmx_get_name(pmx, MMDX_PMX_NAME_MORPH, m, buf, sizeof(buf))); morph_names_.push_back(buf); }
        pose_image.coordinates.resize(nv_);
        pose_image.normals.resize(nv_);
        morph_rates_.assign(nm_, 0.0f);
        palette_.assign(size_t(nb_) * 16, 0.0f);
        bone_poses_.assign(size_t(nb_) * 8, 0.0f);
        ResetPosing();
        Deform();
    }

    uint32_t nv_ = 0, nb_ = 0, nm_ = 0;
    mmdx_model_t model_ = nullptr;
    mmdx_skeleton_t skeleton_ = nullptr;
    std::vector<float> morph_rates_, palette_, bone_poses_;
    std::vector<int32_t> physics_bones_;                  // what a reactor moved this frame (SetPhysicsTransforms)
    std::vector<uint8_t> physics_strict_;
    std::vector<float> physics_skinning_;
    std::vector<std::string> bone_names_, morph_names_;
};

// = mmd::Motion filled by VmdReader::ReadMotion
class Motion {
public:
    explicit Motion(const std::string &vmd_path) { check(mmdx_vmd_load_file(vmd_path.c_str(), &vmd_)); }
    ~Motion() { mmdx_vmd_destroy(vmd_); }
    Motion(const Motion &) = delete;
    Motion &operator=(const Motion &) = delete;
    mmdx_vmd_t handle() const { return vmd_; }
    uint32_t GetLength() const {
        mmdx_vmd_info info;
        info.struct_size = sizeof(info);
        check(mmdx_vmd_get_info(vmd_, &info));
        return info.max_frame;
    }

private:
    mmdx_vmd_t vmd_ = nullptr;
};

// = mmd::MotionPlayer: associates the motion's tracks with the poser's bones and morphs by name at
// construction; SeekFrame / SeekTime evaluate every track at `frame` / `time` seconds (on the device) and hand the results to
// the poser through SetMorphPose / SetBonePose, like the reference's loop over its name maps.
class MotionPlayer {
public:
    MotionPlayer(const Motion &motion, Poser &poser) : poser_(poser) {
        std::vector<const char *> bn, mn;
        for (const std::string &s : poser.bone_names()) bn.push_back(s.c_str());
        for (const std::string &s : poser.morph_names()) mn.push_back(s.c_str());
        check(mmdx_vmd_bind_bones(motion.handle(), uint32_t(bn.size()), bn.data(), &bones_));
        const mmdx_status st = mmdx_vmd_bind_morphs(motion.handle(), uint32_t(mn.size()), mn.data(), &morphs_);
        if (st != MMDX_OK) { mmdx_bone_motion_destroy(bones_); throw Error(st, mmdx_last_error_string()); }
        uint32_t nb = 0, mapped = 0, keys = 0, curves = 0;
        check(mmdx_bone_motion_get_info(bones_, &nb, &mapped, &keys, &curves));
        mapped_bones_ = mapped;
    }
    ~MotionPlayer() {
        mmdx_bone_motion_destroy(bones_);
        mmdx_morph_motion_destroy(morphs_);
    }
    MotionPlayer(const MotionPlayer &) = delete;
    MotionPlayer &operator=(const MotionPlayer &) = delete;

    void SeekFrame(size_t frame) {
        const uint32_t f = uint32_t(frame);
        if (poser_.morph_count())
            check(mmdx_morph_motion_eval(morphs_, poser_.handle(), 1, &f, 0, poser_.morph_rates().data()));
        if (poser_.bone_count())
            check(mmdx_bone_motion_eval(bones_, poser_.handle(), 1, &f, 0, poser_.bone_poses().data()));
    }
    // = MotionPlayer::SeekTime (L/motion/poser_impl.inl:548-555): every track at `time` seconds, interpolated at the fractional
    // frame time * 30 the way the reference's GetMorphPose / GetBonePose(name, double time) do (include/mmdx.h,
    // mmdx_morph_motion_eval_time).  Not SeekFrame(size_t(time * 30)): that steps at 30 fps whatever the display rate.
    void SeekTime(double time) {
        if (poser_.morph_count())
            check(mmdx_morph_motion_eval_time(morphs_, poser_.handle(), 1, &time, 0, poser_.morph_rates().data()));
        if (poser_.bone_count())
            check(mmdx_bone_motion_eval_time(bones_, poser_.handle(), 1, &time, 0, poser_.bone_poses().data()));
    }
    uint32_t mapped_bones() const { return mapped_bones_; }

private:
    Poser &poser_;
    mmdx_bone_motion_t bones_ = nullptr;
    mmdx_morph_motion_t morphs_ = nullptr;
    uint32_t mapped_bones_ = 0;
};

// A crowd of posers that share one model, each with its own MotionPlayer over whichever Motion it likes
// (L/motion/poser_impl.inl:522-555): the motions become the clips of one bank (mmdx_motion_set_t), bound to the poser's bones
// and morphs by name like MotionPlayer does, and instance i plays clip clips[i] at times[i] seconds (SeekTime) or frames[i]
// (SeekFrame).  One call evaluates the whole crowd; clips[i] == MMDX_CLIP_NONE is a poser after ResetPosing().  The arrays are
// host memory by default; with on_device = true clips, times / frames and the output are device memory and the call is
// asynchronous on the poser's stream (and recordable into a graph).  The motions may be destroyed after construction.
class MotionSet {
public:
    // in_place_bone >= 0: the set of the motions IN PLACE (mmdx.h, mmdx_bone_motion_in_place) -- every key of that bone loses its
    // translation on in_place_axes (MMDX_ROOT_X | _Y | _Z), so the poses stay where they are and the placements carry the walk
    // (Animator::RootMotion with a set that kept it).  in_place_turn: mmdx_bone_motion_in_place_turn instead -- the bone's rotation
    // becomes the identity as well, and the placements carry the turning too (Animator::RootTurn).
    MotionSet(const std::vector<const Motion *> &motions, Poser &poser, int in_place_bone = -1, uint32_t in_place_axes = 0,
              bool in_place_turn = false) : poser_(poser) {
        std::vector<const char *> bn, mn;
        for (const std::string &s : poser.bone_names()) bn.push_back(s.c_str());
        for (const std::string &s : poser.morph_names()) mn.push_back(s.c_str());
        std::vector<mmdx_bone_motion_t> bones(motions.size(), nullptr);
        std::vector<mmdx_morph_motion_t> morphs(motions.size(), nullptr);
        mmdx_status st = MMDX_OK;
        for (size_t c = 0; c < motions.size() && st == MMDX_OK; ++c) {
            st = mmdx_vmd_bind_bones(motions[c]->handle(), uint32_t(bn.size()), bn.data(), &bones[c]);
            if (st == MMDX_OK && in_place_bone >= 0) {
                mmdx_bone_motion_t moving = bones[c];
                bones[c] = nullptr;
                st = in_place_turn ? mmdx_bone_motion_in_place_turn(moving, uint32_t(in_place_bone), in_place_axes, &bones[c])
                                   : mmdx_bone_motion_in_place(moving, uint32_t(in_place_bone), in_place_axes, &bones[c]);
                mmdx_bone_motion_destroy(moving);
            }
            if (st == MMDX_OK) st = mmdx_vmd_bind_morphs(motions[c]->handle(), uint32_t(mn.size()), mn.data(), &morphs[c]);
        }
        if (st == MMDX_OK) st = mmdx_motion_set_create(uint32_t(motions.size()), bones.data(), morphs.data(), &set_);
        const std::string why = st == MMDX_OK ? "" : mmdx_last_error_string();
        for (mmdx_bone_motion_t b : bones) mmdx_bone_motion_destroy(b);          // the set holds copies of the tables
        for (mmdx_morph_motion_t m : morphs) mmdx_morph_motion_destroy(m);
        if (st != MMDX_OK) throw Error(st, why);
    }
    ~MotionSet() { mmdx_motion_set_destroy(set_); }
    MotionSet(const MotionSet &) = delete;
    MotionSet &operator=(const MotionSet &) = delete;

    uint32_t clip_count() const {
        mmdx_motion_set_info info;
        info.struct_size = sizeof(info);
        check(mmdx_motion_set_get_info(set_, &info));
        return info.n_clips;
    }
    // out_palettes[i][bone][16] = the skinning matrices of instance i: SeekTime / SeekFrame + Pre/PostPhysicsPosing of its poser
    void SeekTimePalettes(uint32_t n, const uint32_t *clips, const double *times, float *out_palettes, bool on_device = false) {
        check(mmdx_skeleton_solve_motion_set_time(poser_.skeleton(), set_, poser_.handle(), n, clips, times, flags(on_device), out_palettes));
    }
    void SeekFramePalettes(uint32_t n, const uint32_t *clips, const uint32_t *frames, float *out_palettes, bool on_device = false) {
        check(mmdx_skeleton_solve_motion_set(poser_.skeleton(), set_, poser_.handle(), n, clips, frames, flags(on_device), out_palettes));
    }
    // out_poses[i][bone][8] = the evaluated tracks alone, unsolved: the rows BlendPoses / AddPoses take.  With n = clip_count(),
    // clips[i] = i and times[i] = 0 these are the reference rows of AddPoses.
    void SeekTimePoses(uint32_t n, const uint32_t *clips, const double *times, float *out_poses, bool on_device = false) {
        check(mmdx_motion_set_eval_bones_time(set_, poser_.handle(), n, clips, times, flags(on_device), out_poses));
    }
    // A poser on its way from one motion to another: instance i is weights[i] of the way from clip clips_a[i] at times_a[i] to
    // clip clips_b[i] at times_b[i] (lerp of the translations, NLerp of the rotations -- what libmmd does between two keys);
    // below 1e-7 the row is clip a's and above 1 - 1e-7 clip b's, bit for bit, and only that clip is evaluated.
    void BlendTimePalettes(uint32_t n, const uint32_t *clips_a, const double *times_a, const uint32_t *clips_b, const double *times_b,
                           const float *weights, float *out_palettes, bool on_device = false) {
        mmdx_motion_blend_args a;
        a.struct_size = sizeof(a);
        a.n_instances = n;
        a.clips_a = clips_a; a.clips_b = clips_b;
        a.times_a = times_a; a.times_b = times_b;
        a.weights = weights;
        a.flags = flags(on_device);
        check(mmdx_skeleton_solve_motion_set_blend_time(poser_.skeleton(), set_, poser_.handle(), &a, out_palettes));
    }
    // The bone solve for a listed subset of the crowd (mmdx.h, mmdx_skeleton_solve_select): out_palettes[i] for the first *count
    // (NULL = n_ids) instances i of ids, bit for bit what the plain solve writes; every other row keeps its bytes.  poses [n][bones][8],
    // morph_rates [n][morphs] (or NULL) and out_palettes [n][bones][16] are device memory; ids / count are device memory too (what
    // mmdx_cull_bounds wrote; asynchronous on the poser's stream) or, with list_on_device = false, host memory.
    void SolveSelect(uint32_t n, const float *poses, const float *morph_rates, const uint32_t *ids, const uint32_t *count, uint32_t n_ids,
                     float *out_palettes, bool list_on_device = true) {
        mmdx_instance_select s{};
        s.struct_size = sizeof(s);
        s.flags = list_on_device ? uint32_t(MMDX_SELECT_ON_DEVICE) : 0u;
        s.ids = ids; s.count = count; s.n_ids = n_ids;
        check(mmdx_skeleton_solve_select(poser_.skeleton(), poser_.handle(), n, poses, morph_rates,
                                         MMDX_POSES_ON_DEVICE | MMDX_OUT_ON_DEVICE | (morph_rates ? uint32_t(MMDX_WEIGHTS_ON_DEVICE) : 0u),
                                         &s, out_palettes));
    }
    // Where every instance stands (mmdx.h, mmdx_palette_place): out_palettes[i][bone] = palettes[i][bone] * W[i], W[i] from the pose
    // {tx, ty, tz, 0, qx, qy, qz, qw} at placements + 8 * i ("a world bone") or, with matrix = true, the 16 floats at placements +
    // 16 * i -- the layout of the viewer's g_state.model_matrix.  out_palettes may be palettes (in place).  Host arrays by default;
    // with on_device = true all three are device memory and the call is asynchronous on the poser's stream.
    void PlacePalettes(uint32_t n, const float *palettes, const float *placements, float *out_palettes, bool matrix = false,
                       bool on_device = false) {
        mmdx_place_args a{};
        a.struct_size = sizeof(a);
        a.flags = (on_device ? uint32_t(MMDX_PALETTE_ON_DEVICE | MMDX_PLACE_ON_DEVICE | MMDX_OUT_ON_DEVICE) : 0u) |
                  (matrix ? uint32_t(MMDX_PLACE_MATRIX) : 0u);
        a.n_instances = n;
        a.palettes = palettes; a.placements = placements; a.out_palettes = out_palettes;
        check(mmdx_palette_place(poser_.handle(), &a));
    }
    // A conservative box per instance from the palette alone, before any deform (mmdx.h, mmdx_palette_bounds): out_bounds[i] =
    // {min xyz, max xyz} contains every position a deform of instance i from `palettes` with this pos_scale writes while no slot
    // weight exceeds morph_scale.  What mmdx_cull_bounds takes, one frame earlier than the deform's own bounds.
    void PaletteBounds(uint32_t n, const float *palettes, float *out_bounds, float pos_scale = 1.0f, float morph_scale = 1.0f,
                       bool on_device = false) {
        mmdx_palette_bounds_args a{};
        a.struct_size = sizeof(a);
        a.flags = on_device ? uint32_t(MMDX_PALETTE_ON_DEVICE | MMDX_OUT_ON_DEVICE) : 0u;
        a.n_instances = n;
        a.palettes = palettes; a.out_bounds = out_bounds;
        a.pos_scale = pos_scale; a.morph_scale = morph_scale;
        check(mmdx_palette_bounds(poser_.handle(), &a));
    }
    // out_rates[i][morph] = the morph rates of instance i (what mmdx_deform_batched takes as per-instance weights)
    void SeekTimeMorphRates(uint32_t n, const uint32_t *clips, const double *times, float *out_rates, bool on_device = false) {
        check(mmdx_motion_set_eval_morphs_time(set_, poser_.handle(), n, clips, times, flags(on_device), out_rates));
    }
    void SeekFrameMorphRates(uint32_t n, const uint32_t *clips, const uint32_t *frames, float *out_rates, bool on_device = false) {
        check(mmdx_motion_set_eval_morphs(set_, poser_.handle(), n, clips, frames, flags(on_device), out_rates));
    }
    // = Motion::GetLength() of every clip over the tracks bound to the poser: its largest key frame; seconds = frames / 30.0
    std::vector<uint32_t> ClipFrames() const {
        std::vector<uint32_t> frames(clip_count());
        check(mmdx_motion_set_clip_frames(set_, frames.data()));
        return frames;
    }
    // The blend calls over ready-made operands -- mmdx::Animator::operands(): the animator's device arrays, outputs on the device
    void BlendTimePalettes(const mmdx_motion_blend_args &operands, float *out_palettes) {
        check(mmdx_skeleton_solve_motion_set_blend_time(poser_.skeleton(), set_, poser_.handle(), &operands, out_palettes));
    }
    void BlendTimeMorphRates(const mmdx_motion_blend_args &operands, float *out_rates) {
        check(mmdx_motion_set_blend_morphs_time(set_, poser_.handle(), &operands, out_rates));
    }
    // The same for a listed subset of the crowd (mmdx.h, the *_blend_*_time_select calls): only the first *count (NULL = n_ids)
    // instances of ids are evaluated, their rows bit for bit the plain call's; every other row of the output keeps its bytes, so a
    // crowd's track evaluation costs what is in view.  The clocks still advance for everyone (Animator::Advance).  ids / count are
    // device memory (what mmdx_cull_bounds wrote; asynchronous on the poser's stream) or, with list_on_device = false, host memory.
    void BlendTimePalettes(const mmdx_motion_blend_args &operands, const uint32_t *ids, const uint32_t *count, uint32_t n_ids,
                           float *out_palettes, bool list_on_device = true) {
        const mmdx_instance_select s = select(ids, count, n_ids, list_on_device);
        check(mmdx_skeleton_solve_motion_set_blend_time_select(poser_.skeleton(), set_, poser_.handle(), &operands, &s, out_palettes));
    }
    void BlendTimePoses(const mmdx_motion_blend_args &operands, const uint32_t *ids, const uint32_t *count, uint32_t n_ids,
                        float *out_poses, bool list_on_device = true) {
        const mmdx_instance_select s = select(ids, count, n_ids, list_on_device);
        check(mmdx_motion_set_blend_bones_time_select(set_, poser_.handle(), &operands, &s, out_poses));
    }
    void BlendTimeMorphRates(const mmdx_motion_blend_args &operands, const uint32_t *ids, const uint32_t *count, uint32_t n_ids,
                             float *out_rates, bool list_on_device = true) {
        const mmdx_instance_select s = select(ids, count, n_ids, list_on_device);
        check(mmdx_motion_set_blend_morphs_time_select(set_, poser_.handle(), &operands, &s, out_rates));
    }
    // Layers (mmdx.h, mmdx_pose_blend / mmdx_rate_blend): out[i][item] = the cross-fade's blend of a[i][item] and b[i][item] at
    // weights[i] * masks[mask_ids[i]][item] -- the upper body from one animator over the legs of another, a talking face over a
    // dancing body.  a, b, out are [n][row_items][8] poses (BlendPoses) or [n][row_items] rates (BlendRates); out may be a or b;
    // mask_ids may be NULL (no masks: the cross-fade itself) and holds MMDX_MASK_NONE for an instance without one.  Items whose
    // effective weight is below 1e-7 never read b, so the layer's rows need evaluating for the instances that wear it only.  Host
    // arrays by default; with on_device = true everything is device memory and the call is asynchronous on the poser's stream
    // (recordable); ids / count / n_ids then restrict it to a listed subset (NULL ids = everyone), every other row keeps its bytes.
    void BlendPoses(uint32_t n, uint32_t row_items, const float *a, const float *b, const float *weights, const uint32_t *mask_ids,
                    const float *masks, uint32_t n_masks, float *out, bool on_device = false, const uint32_t *ids = nullptr,
                    const uint32_t *count = nullptr, uint32_t n_ids = 0, bool list_on_device = true) {
        const mmdx_row_blend_args r = row_blend_args(n, row_items, a, b, weights, mask_ids, masks, n_masks, out, on_device);
        const mmdx_instance_select s = select(ids, count, n_ids, list_on_device);
        check(mmdx_pose_blend(poser_.handle(), &r, ids ? &s : nullptr));
    }
    void BlendRates(uint32_t n, uint32_t row_items, const float *a, const float *b, const float *weights, const uint32_t *mask_ids,
                    const float *masks, uint32_t n_masks, float *out, bool on_device = false, const uint32_t *ids = nullptr,
                    const uint32_t *count = nullptr, uint32_t n_ids = 0, bool list_on_device = true) {
        const mmdx_row_blend_args r = row_blend_args(n, row_items, a, b, weights, mask_ids, masks, n_masks, out, on_device);
        const mmdx_instance_select s = select(ids, count, n_ids, list_on_device);
        check(mmdx_rate_blend(poser_.handle(), &r, ids ? &s : nullptr));
    }
    // Additive layers (mmdx.h, mmdx_pose_add / mmdx_rate_add): out[i][item] = a[i][item] with the difference between b[i][item] and
    // refs[ref_ids[i]][item] applied at weights[i] * masks[mask_ids[i]][item] the way a bone morph is -- breathing, a recoil, a nod on
    // top of whatever the base plays; weights above 1 exaggerate.  ref_ids may be NULL and holds MMDX_REF_NONE where b already is a
    // difference.  refs [n_refs][row_items][8] (poses) or [n_refs][row_items] (rates) are the rows SeekTimePoses / SeekTimeMorphRates
    // write for clips 0 .. n_refs - 1 at time 0.  Everything else as BlendPoses / BlendRates.
    void AddPoses(uint32_t n, uint32_t row_items, const float *a, const float *b, const float *weights, const uint32_t *mask_ids,
                  const float *masks, uint32_t n_masks, const uint32_t *ref_ids, const float *refs, uint32_t n_refs, float *out,
                  bool on_device = false, const uint32_t *ids = nullptr, const uint32_t *count = nullptr, uint32_t n_ids = 0,
                  bool list_on_device = true) {
        const mmdx_row_add_args r = row_add_args(n, row_items, a, b, weights, mask_ids, masks, n_masks, ref_ids, refs, n_refs, out, on_device);
        const mmdx_instance_select s = select(ids, count, n_ids, list_on_device);
        check(mmdx_pose_add(poser_.handle(), &r, ids ? &s : nullptr));
    }
    void AddRates(uint32_t n, uint32_t row_items, const float *a, const float *b, const float *weights, const uint32_t *mask_ids,
                  const float *masks, uint32_t n_masks, const uint32_t *ref_ids, const float *refs, uint32_t n_refs, float *out,
                  bool on_device = false, const uint32_t *ids = nullptr, const uint32_t *count = nullptr, uint32_t n_ids = 0,
                  bool list_on_device = true) {
        const mmdx_row_add_args r = row_add_args(n, row_items, a, b, weights, mask_ids, masks, n_masks, ref_ids, refs, n_refs, out, on_device);
        const mmdx_instance_select s = select(ids, count, n_ids, list_on_device);
        check(mmdx_rate_add(poser_.handle(), &r, ids ? &s : nullptr));
    }
    // A mask row for BlendPoses from the hierarchy (mmdx_skeleton_subtree_mask, host only): `inside` for every bone that is one of
    // roots or has one among its ancestors, `outside` for the rest.
    std::vector<float> SubtreeMask(const std::vector<uint32_t> &roots, float inside = 1.0f, float outside = 0.0f) const {
        std::vector<float> mask(poser_.bone_names().size());
        check(mmdx_skeleton_subtree_mask(poser_.skeleton(), uint32_t(roots.size()), roots.data(), inside, outside, mask.data()));
        return mask;
    }
    mmdx_motion_set_t handle() const { return set_; }
    Poser &poser() const { return poser_; }

private:
    static mmdx_row_blend_args row_blend_args(uint32_t n, uint32_t row_items, const float *a, const float *b, const float *weights,
                                              const uint32_t *mask_ids, const float *masks, uint32_t n_masks, float *out, bool on_device) {
        mmdx_row_blend_args r{};
        r.struct_size = sizeof(r);
        r.flags = on_device ? uint32_t(MMDX_BLEND_A_ON_DEVICE | MMDX_BLEND_B_ON_DEVICE | MMDX_BLEND_PARAMS_ON_DEVICE | MMDX_OUT_ON_DEVICE) : 0u;
        r.n_instances = n; r.row_items = row_items;
        r.a = a; r.b = b; r.weights = weights;
        r.mask_ids = mask_ids; r.masks = masks; r.n_masks = n_masks;
        r.out = out;
        return r;
    }
    static mmdx_row_add_args row_add_args(uint32_t n, uint32_t row_items, const float *a, const float *b, const float *weights,
                                          const uint32_t *mask_ids, const float *masks, uint32_t n_masks, const uint32_t *ref_ids,
                                          const float *refs, uint32_t n_refs, float *out, bool on_device) {
        mmdx_row_add_args r{};
        r.struct_size = sizeof(r);
        r.flags = on_device ? uint32_t(MMDX_BLEND_A_ON_DEVICE | MMDX_BLEND_B_ON_DEVICE | MMDX_BLEND_PARAMS_ON_DEVICE | MMDX_OUT_ON_DEVICE) : 0u;
        r.n_instances = n; r.row_items = row_items;
        r.a = a; r.b = b; r.weights = weights;
        r.mask_ids = mask_ids; r.masks = masks; r.n_masks = n_masks;
        r.ref_ids = ref_ids; r.refs = refs; r.n_refs = n_refs;
        r.out = out;
        return r;
    }
    static mmdx_instance_select select(const uint32_t *ids, const uint32_t *count, uint32_t n_ids, bool on_device) {
        mmdx_instance_select s{};
        s.struct_size = sizeof(s);
        s.flags = on_device ? uint32_t(MMDX_SELECT_ON_DEVICE) : 0u;
        s.ids = ids; s.count = count; s.n_ids = n_ids;
        return s;
    }
    static uint32_t flags(bool on_device) { return on_device ? uint32_t(MMDX_FRAMES_ON_DEVICE | MMDX_OUT_ON_DEVICE) : 0u; }
    Poser &poser_;
    mmdx_motion_set_t set_ = nullptr;
};

// The clocks of a crowd: the reference's g_state.time += dt (main.cpp:1757) for one MotionPlayer becomes one launch for all posers.
// Every instance has a clip playing, a clip it is fading to, their clocks and the fade weight, all in device memory; Advance(dt)
// steps them -- loop wrap, hold, "then" chains, the fade and its hand-over, pending requests (mmdx.h states the arithmetic) -- and
// operands() is what MotionSet::BlendTimePalettes / BlendTimeMorphRates take.  table: one mmdx_animator_clip per clip of the set
// (empty = every clip loops over its own length).
class EventSet;
class Animator {
public:
    Animator(MotionSet &set, uint32_t n_instances, const std::vector<mmdx_animator_clip> &table = {}) : set_(set), n_(n_instances) {
        mmdx_animator_desc d{};
        d.struct_size = sizeof(d);
        d.n_instances = n_instances;
        d.clips = table.empty() ? nullptr : table.data();
        d.n_clips = uint32_t(table.size());
        check(mmdx_animator_create(set.handle(), &d, &anim_));
    }
    ~Animator() { mmdx_animator_destroy(anim_); }
    Animator(const Animator &) = delete;
    Animator &operator=(const Animator &) = delete;

    // one step for every instance, on the poser's stream; a recorded graph freezes dt -- record AdvanceDeviceDt instead
    void Advance(double dt) { check(mmdx_animator_advance(anim_, set_.poser().handle(), &dt, 0)); }
    void AdvanceDeviceDt(const double *dt_device) { check(mmdx_animator_advance(anim_, set_.poser().handle(), dt_device, MMDX_ANIM_DT_ON_DEVICE)); }
    // Root motion (mmdx.h, mmdx_animator_root_motion): placements [n][8] in device memory, the pose form of PlacePalettes, receive
    // what the playing clips of `moving` -- a set with this animator's clip count that kept the root's translation -- move bone
    // root_bone by during the step that Advance is ABOUT to take, turned by each placement's heading.  Call it before Advance with
    // the same dt, or call Step, which does both in that order.
    void RootMotion(MotionSet &moving, uint32_t root_bone, uint32_t axes, float *placements_device, double dt) {
        root_motion(moving, root_bone, axes, placements_device, &dt, 0);
    }
    void RootMotionDeviceDt(MotionSet &moving, uint32_t root_bone, uint32_t axes, float *placements_device, const double *dt_device) {
        root_motion(moving, root_bone, axes, placements_device, dt_device, MMDX_ANIM_DT_ON_DEVICE);
    }
    void Step(MotionSet &moving, uint32_t root_bone, uint32_t axes, float *placements_device, double dt) {
        RootMotion(moving, root_bone, axes, placements_device, dt);
        Advance(dt);
    }
    void StepDeviceDt(MotionSet &moving, uint32_t root_bone, uint32_t axes, float *placements_device, const double *dt_device) {
        RootMotionDeviceDt(moving, root_bone, axes, placements_device, dt_device);
        AdvanceDeviceDt(dt_device);
    }
    // Root motion that turns (mmdx.h, mmdx_animator_root_motion_turn): the same, and each placement's heading [4..7] is multiplied
    // by the root's rotation delta; normalize = MMDX_ROOT_NORMALIZE.  `moving` kept the root's translation and rotation; the poses
    // come from a set built with in_place_turn.
    void RootTurn(MotionSet &moving, uint32_t root_bone, uint32_t axes, float *placements_device, double dt, bool normalize = false) {
        root_turn(moving, root_bone, axes, placements_device, &dt, normalize ? uint32_t(MMDX_ROOT_NORMALIZE) : 0u);
    }
    void RootTurnDeviceDt(MotionSet &moving, uint32_t root_bone, uint32_t axes, float *placements_device, const double *dt_device,
                          bool normalize = false) {
        root_turn(moving, root_bone, axes, placements_device, dt_device,
                  MMDX_ANIM_DT_ON_DEVICE | (normalize ? uint32_t(MMDX_ROOT_NORMALIZE) : 0u));
    }
    void StepTurn(MotionSet &moving, uint32_t root_bone, uint32_t axes, float *placements_device, double dt, bool normalize = false) {
        RootTurn(moving, root_bone, axes, placements_device, dt, normalize);
        Advance(dt);
    }
    // Clip markers (mmdx.h, mmdx_animator_events): out_fired [n] in device memory receives, per instance, the channels of the markers
    // of `events` that the step Advance is ABOUT to take passes; call it before Advance with the same dt.  With n_lists > 0, list l
    // (out_ids + l * list_stride, ascending instance ids, its length in out_counts[l]) holds the instances whose mask meets
    // list_masks[l] -- and, with levels (mmdx_cull_bounds' out_levels), are not culled -- ready for any select call.  dt_on_device:
    // dt is a device double (record this form); dominant: MMDX_EVENTS_DOMINANT_SIDE.
    inline void Events(EventSet &events, uint32_t *out_fired, const double *dt, bool dt_on_device = false, uint32_t n_lists = 0,
                       const uint32_t *list_masks = nullptr, uint32_t list_stride = 0, uint32_t *out_ids = nullptr,
                       uint32_t *out_counts = nullptr, const uint32_t *levels = nullptr, bool dominant = false);
    // instance ids[j] fades over fades[j] seconds (NULL: at once) to clips[j], started at start_times[j] (NULL: 0); host lists
    void Request(uint32_t n, const uint32_t *ids, const uint32_t *clips, const float *fades = nullptr, const double *start_times = nullptr,
                 bool on_device = false) {
        check(mmdx_animator_request(anim_, set_.poser().handle(), n, ids, clips, fades, start_times, on_device ? uint32_t(MMDX_TIMES_ON_DEVICE) : 0u));
    }
    // host arrays in / out; NULL members are left alone (state.struct_size and n_instances are filled in here)
    void SetState(mmdx_animator_arrays state) {
        state.struct_size = sizeof(state); state.n_instances = n_;
        check(mmdx_animator_set_state(anim_, set_.poser().handle(), &state));
    }
    void GetState(mmdx_animator_arrays state) {
        state.struct_size = sizeof(state); state.n_instances = n_;
        check(mmdx_animator_get_state(anim_, set_.poser().handle(), &state));
    }
    mmdx_motion_blend_args operands() {
        mmdx_motion_blend_args a;
        check(mmdx_animator_operands(anim_, &a));
        return a;
    }
    mmdx_animator_arrays device_arrays() {
        mmdx_animator_arrays a{};
        a.struct_size = sizeof(a);
        check(mmdx_animator_device_arrays(anim_, &a));
        return a;
    }
    mmdx_animator_t handle() const { return anim_; }

private:
    void root_motion(MotionSet &moving, uint32_t root_bone, uint32_t axes, float *placements, const double *dt, uint32_t flags) {
        mmdx_root_motion_args a{};
        a.struct_size = sizeof(a);
        a.flags = flags;
        a.root_bone = root_bone; a.axes = axes;
        a.dt = dt; a.placements = placements;
        check(mmdx_animator_root_motion(anim_, moving.handle(), set_.poser().handle(), &a));
    }
    void root_turn(MotionSet &moving, uint32_t root_bone, uint32_t axes, float *placements, const double *dt, uint32_t flags) {
        mmdx_root_turn_args a{};
        a.struct_size = sizeof(a);
        a.flags = flags;
        a.root_bone = root_bone; a.axes = axes;
        a.dt = dt; a.placements = placements;
        check(mmdx_animator_root_motion_turn(anim_, moving.handle(), set_.poser().handle(), &a));
    }
    MotionSet &set_;
    uint32_t n_;
    mmdx_animator_t anim_ = nullptr;
};

// The markers of an animator's clips (mmdx.h, mmdx_event_set_create): {time in seconds, clip, channel < 32} in any order.  The set
// copies what it needs of the animator and may outlive it.
class EventSet {
public:
    EventSet(Animator &animator, const std::vector<mmdx_event_marker> &markers) {
        mmdx_event_set_desc d{};
        d.struct_size = sizeof(d);
        d.n_markers = uint32_t(markers.size());
        d.markers = markers.empty() ? nullptr : markers.data();
        check(mmdx_event_set_create(animator.handle(), &d, &set_));
    }
    ~EventSet() { mmdx_event_set_destroy(set_); }
    EventSet(const EventSet &) = delete;
    EventSet &operator=(const EventSet &) = delete;
    mmdx_event_set_t handle() const { return set_; }

private:
    mmdx_event_set_t set_ = nullptr;
};

inline void Animator::Events(EventSet &events, uint32_t *out_fired, const double *dt, bool dt_on_device, uint32_t n_lists,
                             const uint32_t *list_masks, uint32_t list_stride, uint32_t *out_ids, uint32_t *out_counts,
                             const uint32_t *levels, bool dominant) {
    mmdx_events_args a{};
    a.struct_size = sizeof(a);
    a.flags = (dt_on_device ? uint32_t(MMDX_ANIM_DT_ON_DEVICE) : 0u) | (dominant ? uint32_t(MMDX_EVENTS_DOMINANT_SIDE) : 0u);
    a.dt = dt; a.out_fired = out_fired;
    a.n_lists = n_lists; a.list_stride = list_stride;
    for (uint32_t l = 0; l < n_lists && l < MMDX_EVENTS_MAX_LISTS; ++l) a.list_mask[l] = list_masks[l];
    a.levels = levels; a.out_ids = out_ids; a.out_counts = out_counts;
    check(mmdx_animator_events(anim_, events.handle(), set_.poser().handle(), &a));
}

// Bone sockets (mmdx.h, mmdx_palette_sockets): where a character's hand, head or saddle is, for every instance, on the device.  The
// reference-side equivalent for one Poser is bone_images_[b].global_offset_matrix_inv_ * bone_images_[b].skinning_matrix_.  A set
// is created on a model handle: bones [n] index the model's bones, rest_positions [n][3] are those bones' Model::Bone::GetPosition,
// offsets (NULL = none) are [n][8] poses {tx, ty, tz, 0, qx, qy, qz, qw} or, with offsets_are_matrices, [n][16] matrices: the
// attachment's frame inside the bone's.  has_offset (NULL = every socket has one) names the sockets that do.
class SocketSet {
public:
    SocketSet(mmdx_model_t model, uint32_t n, const uint32_t *bones, const float *rest_positions, const float *offsets = nullptr,
              bool offsets_are_matrices = false, const uint8_t *has_offset = nullptr) : n_(n) {
        mmdx_socket_set_desc d{};
        d.struct_size = sizeof(d);
        d.flags = offsets && offsets_are_matrices ? uint32_t(MMDX_SOCKET_OFFSET_MATRIX) : 0u;
        d.n_sockets = n;
        d.bone = bones; d.rest_position = rest_positions; d.offset = offsets; d.has_offset = has_offset;
        check(mmdx_socket_set_create(model, &d, &set_));
    }
    ~SocketSet() { mmdx_socket_set_destroy(set_); }
    SocketSet(const SocketSet &) = delete;
    SocketSet &operator=(const SocketSet &) = delete;

    // out_sockets [sockets][n][16], socket-major: slab(out_sockets, n, s) is an [n][16] placement array for the PlacePalettes(...,
    // matrix = true, on_device = true) of another model's crowd.  On palettes that went through PlacePalettes the matrices are world
    // frames.  Host arrays by default; with on_device = true both are device memory and the call is asynchronous on the model's
    // stream (and records into its graph).  select (NULL = every instance): what mmdx_cull_bounds wrote, device operands only.
    void Sockets(uint32_t n_instances, const float *palettes, float *out_sockets, bool on_device = false,
                 const mmdx_instance_select *select = nullptr) {
        mmdx_sockets_args a{};
        a.struct_size = sizeof(a);
        a.flags = on_device ? uint32_t(MMDX_PALETTE_ON_DEVICE | MMDX_OUT_ON_DEVICE) : 0u;
        a.n_instances = n_instances;
        a.palettes = palettes; a.out_sockets = out_sockets; a.select = select;
        check(mmdx_palette_sockets(set_, &a));
    }
    static float *slab(float *out_sockets, uint32_t n_instances, uint32_t socket) { return out_sockets + size_t(socket) * n_instances * 16; }
    uint32_t size() const { return n_; }
    mmdx_socket_set_t handle() const { return set_; }

private:
    uint32_t n_;
    mmdx_socket_set_t set_ = nullptr;
};

// Spring bones (mmdx.h, mmdx_spring_step): chains of bones that swing behind their parents -- hair, skirts, ribbons -- for every
// instance of a crowd, on the device.  The reference moves such bones with Bullet, once per Poser; this is the crowd's substitute,
// not a port of it.  A set is created on a skeleton handle from a filled mmdx_spring_set_desc (the arrays are copied); Step rewrites
// the chains' rows of device palettes [n][bones][16] in place, after PlacePalettes for a simulation in world space, before it for
// one in model space.
class SpringSet {
public:
    SpringSet(mmdx_skeleton_t skeleton, mmdx_spring_set_desc desc) {
        desc.struct_size = sizeof(desc);
        check(mmdx_spring_set_create(skeleton, &desc, &set_));
    }
    ~SpringSet() { mmdx_spring_set_destroy(set_); }
    SpringSet(const SpringSet &) = delete;
    SpringSet &operator=(const SpringSet &) = delete;

    // One step of every chain of every instance (select: of the listed ones), asynchronous on `model`'s stream.  dt: one float, host
    // memory, or device memory with dt_on_device (what a recorded frame takes, together with a device list or none).
    void Step(mmdx_model_t model, uint32_t n_instances, float *device_palettes, const float *dt, bool dt_on_device = false,
              const mmdx_instance_select *select = nullptr, bool reset = false) {
        mmdx_spring_args a{};
        a.struct_size = sizeof(a);
        a.flags = uint32_t(MMDX_PALETTE_ON_DEVICE) | (dt_on_device ? uint32_t(MMDX_SPRING_DT_ON_DEVICE) : 0u) |
                  (reset ? uint32_t(MMDX_SPRING_RESET) : 0u);
        a.n_instances = n_instances;
        a.palettes = device_palettes; a.dt = dt; a.select = select;
        check(mmdx_spring_step(set_, model, &a));
    }
    // every joint back to the rigid continuation of its parent
    void Reset(mmdx_model_t model, uint32_t n_instances, float *device_palettes, const mmdx_instance_select *select = nullptr) {
        const float zero = 0.0f;
        Step(model, n_instances, device_palettes, &zero, false, select, true);
    }
    // [n_instances][joints][6] = {current tail, previous tail}: save and restore
    void GetState(mmdx_model_t model, uint32_t n_instances, float *out) { check(mmdx_spring_get_state(set_, model, n_instances, out)); }
    void SetState(mmdx_model_t model, uint32_t n_instances, const float *in) { check(mmdx_spring_set_state(set_, model, n_instances, in)); }
    mmdx_spring_set_info Info() const {
        mmdx_spring_set_info i{};
        i.struct_size = sizeof(i);
        check(mmdx_spring_set_get_info(set_, &i));
        return i;
    }
    mmdx_spring_set_t handle() const { return set_; }

private:
    mmdx_spring_set_t set_ = nullptr;
};

// Look-at (mmdx.h, mmdx_palette_aim): heads and eyes of a crowd turn to per-instance targets, on the device.  A set is created on a
// skeleton handle from a filled mmdx_aim_set_desc (the arrays are copied); Aim rewrites the rows of the aims' subtrees of device
// palettes [n][bones][16] in place, after PlacePalettes for targets in world space, and BEFORE SpringSet::Step: hair anchors on the
// head row.
class AimSet {
public:
    AimSet(mmdx_skeleton_t skeleton, mmdx_aim_set_desc desc) {
        desc.struct_size = sizeof(desc);
        check(mmdx_aim_set_create(skeleton, &desc, &set_));
    }
    ~AimSet() { mmdx_aim_set_destroy(set_); }
    AimSet(const AimSet &) = delete;
    AimSet &operator=(const AimSet &) = delete;

    // Every aim of every instance (select: of the listed ones), asynchronous on `model`'s stream.  targets: {x, y, z, weight} every
    // `stride` floats (0: one for everyone), host memory, or device memory with targets_on_device (what a recorded frame takes,
    // together with a device list or none).  A slab of SocketSet::Sockets goes in as SocketSet::slab(...) + 12 with stride 16.
    void Aim(mmdx_model_t model, uint32_t n_instances, float *device_palettes, const float *targets, uint32_t stride = 4,
             bool targets_on_device = true, const mmdx_instance_select *select = nullptr) {
        mmdx_aim_args a{};
        a.struct_size = sizeof(a);
        a.flags = uint32_t(MMDX_PALETTE_ON_DEVICE) | (targets_on_device ? uint32_t(MMDX_AIM_TARGETS_ON_DEVICE) : 0u);
        a.n_instances = n_instances;
        a.target_stride = stride;
        a.palettes = device_palettes; a.targets = targets; a.select = select;
        check(mmdx_palette_aim(set_, model, &a));
    }
    mmdx_aim_set_info Info() const {
        mmdx_aim_set_info i{};
        i.struct_size = sizeof(i);
        check(mmdx_aim_set_get_info(set_, &i));
        return i;
    }
    mmdx_aim_set_t handle() const { return set_; }

private:
    mmdx_aim_set_t set_ = nullptr;
};

// Reach (mmdx.h, mmdx_palette_reach): two-bone IK puts hands and feet of a crowd on per-instance targets, on the device.  A set is
// created on a skeleton handle from a filled mmdx_reach_set_desc (the arrays are copied); Reach rewrites the rows of the limbs'
// subtrees of device palettes [n][bones][16] in place, AFTER AimSet::Aim (an aimed spine carries the arms) and BEFORE
// SpringSet::Step (sleeves anchor on the rows it rewrites).
class ReachSet {
public:
    ReachSet(mmdx_skeleton_t skeleton, mmdx_reach_set_desc desc) {
        desc.struct_size = sizeof(desc);
        check(mmdx_reach_set_create(skeleton, &desc, &set_));
    }
    ~ReachSet() { mmdx_reach_set_destroy(set_); }
    ReachSet(const ReachSet &) = delete;
    ReachSet &operator=(const ReachSet &) = delete;

    // Every reach of every instance (select: of the listed ones), asynchronous on `model`'s stream.  targets: {x, y, z, weight}
    // every `stride` floats (0: one for everyone), host memory, or device memory with targets_on_device (what a recorded frame
    // takes, together with a device list or none).  A slab of SocketSet::Sockets goes in as SocketSet::slab(...) + 12 with stride 16.
    void Reach(mmdx_model_t model, uint32_t n_instances, float *device_palettes, const float *targets, uint32_t stride = 4,
               bool targets_on_device = true, const mmdx_instance_select *select = nullptr) {
        mmdx_reach_args a{};
        a.struct_size = sizeof(a);
        a.flags = uint32_t(MMDX_PALETTE_ON_DEVICE) | (targets_on_device ? uint32_t(MMDX_REACH_TARGETS_ON_DEVICE) : 0u);
        a.n_instances = n_instances;
        a.target_stride = stride;
        a.palettes = device_palettes; a.targets = targets; a.select = select;
        check(mmdx_palette_reach(set_, model, &a));
    }
    mmdx_reach_set_info Info() const {
        mmdx_reach_set_info i{};
        i.struct_size = sizeof(i);
        check(mmdx_reach_set_get_info(set_, &i));
        return i;
    }
    mmdx_reach_set_t handle() const { return set_; }

private:
    mmdx_reach_set_t set_ = nullptr;
};

// Ground (mmdx.h, mmdx_ground_place / mmdx_ground_targets): a regular height field lifts placements and the feet's reach targets on
// the device.  A ground is created from a filled mmdx_ground_desc (the heights are copied).  Place runs AFTER root motion and BEFORE
// the placement is used; Targets runs AFTER SocketSet::Sockets of the feet and BEFORE the feet's ReachSet::Reach, and its drop is
// what the NEXT frame's Place reads.
class Ground {
public:
    explicit Ground(mmdx_ground_desc desc) {
        desc.struct_size = sizeof(desc);
        check(mmdx_ground_create(&desc, &ground_));
    }
    ~Ground() { mmdx_ground_destroy(ground_); }
    Ground(const Ground &) = delete;
    Ground &operator=(const Ground &) = delete;

    // placements[i][1] = (h(x, z) + y_offset) + drop[i] of every instance (select: of the listed ones), asynchronous on `model`'s
    // stream.  device_placements [n][MMDX_POSE_FLOATS]; device_drop [n] or nullptr.
    void Place(mmdx_model_t model, uint32_t n_instances, float *device_placements, const float *device_drop = nullptr, float y_offset = 0.0f,
               const mmdx_instance_select *select = nullptr) {
        mmdx_ground_place_args a{};
        a.struct_size = sizeof(a);
        a.n_instances = n_instances;
        a.y_offset = y_offset;
        a.placements = device_placements; a.drop = device_drop; a.select = select;
        check(mmdx_ground_place(ground_, model, &a));
    }
    // Reach targets [n_feet][n][4] and the hip drop [n] (or nullptr) from the feet's world points: foot f of instance i at
    // device_points + f*slab_stride + i*point_stride floats.  A SocketSet::Sockets output goes in as SocketSet::slab(...) + 12 with
    // the default strides (16 and n*16).
    void Targets(mmdx_model_t model, uint32_t n_instances, uint32_t n_feet, const float *device_placements, const float *device_points,
                 float *device_out_targets, float *device_out_drop, float max_step, float max_drop, uint32_t point_stride = 16,
                 uint32_t slab_stride = 0, const mmdx_instance_select *select = nullptr) {
        mmdx_ground_targets_args a{};
        a.struct_size = sizeof(a);
        a.n_instances = n_instances; a.n_feet = n_feet;
        a.placements = device_placements; a.points = device_points;
        a.point_stride = point_stride;
        a.slab_stride = slab_stride ? slab_stride : n_instances * point_stride;
        a.out_targets = device_out_targets; a.out_drop = device_out_drop;
        a.max_step = max_step; a.max_drop = max_drop; a.select = select;
        check(mmdx_ground_targets(ground_, model, &a));
    }
    mmdx_ground_info Info() const {
        mmdx_ground_info i{};
        i.struct_size = sizeof(i);
        check(mmdx_ground_get_info(ground_, &i));
        return i;
    }
    mmdx_ground_t handle() const { return ground_; }

private:
    mmdx_ground_t ground_ = nullptr;
};

}  // namespace mmdx

/* mmdx.h -- C ABI of the MI355X-native per-frame deformation engine for MMD/PMX models.
 *
 * This is the drop-in boundary for ONE path of CU-Production/simple_mmd_renderer: the per-vertex
 * morph-target blend + BDEF1/2/4/SDEF linear-blend skinning that the vendored libmmd evaluates on
 * one CPU thread every frame, plus the viewer's repack into its 32-byte vertex stream:
 *
 *     reference (L/ = 3rd_party/libmmd/include/mmd/)              replaced by
 *     ----------------------------------------------------------  -------------------------------
 *     mmd::Model vertex/skin/morph stores  L/model/model.inl:21-104,  mmdx_model_create()
 *         :334-517, :719-726; Model::Normalize L/model/model_impl.inl:406-452
 *     Poser::SetMorphPose + morph part of PrePhysicsPosing +        morph_weights argument of
 *         UpdateMorphTransform  L/motion/poser_impl.inl:328-346,       mmdx_deform*()
 *         :362-365, :384-386, :478-480
 *     Poser::BoneImage::skinning_matrix_ (the palette, read through  palette argument of
 *         PhysicsReactor::GetPoserBoneImage L/motion/physics.inl:32-40) mmdx_deform*()
 *     Poser::Deform -> Poser::pose_image  L/motion/poser_impl.inl:396-461,  mmdx_deform*(), layout
 *         L/motion/poser.inl:17-20                                       MMDX_OUT_SOA
 *     UpdateDeformedVertices (struct Vertex, x0.1 scale, uv copy)    mmdx_deform*(), layout
 *         main.cpp:50-54, :821-863                                       MMDX_OUT_VERTEX32
 *     call site frame() main.cpp:1821 + :1824                        one mmdx_deform() call
 *
 * Everything else of the viewer (bone solve, VMD evaluation, Bullet, sokol draw loop) is untouched:
 * the host keeps producing morph rates and the bone palette and hands them over per frame.
 *
 * Conventions
 *   - Matrices: row-vector, row-major float[16], y = x * M, translation in elements 12..14
 *     (L/util/math.inl:383-395; identical to an OpenGL column-major float[16]).
 *   - No exceptions cross this boundary: every call returns an mmdx_status; the text of the last
 *     error on the calling thread is available from mmdx_last_error_string().
 *   - All indices are validated in mmdx_model_create(); mmdx_deform*() can only fail on argument
 *     errors or HIP runtime errors.
 *   - A model handle owns its device allocations and one HIP stream; calls on one handle are not
 *     re-entrant; different handles (and devices) may be driven from different host threads.
 *   - Results are bit-identical to the reference's CPU path (the kernels are compiled with
 *     -ffp-contract=off and keep the reference's operation order); see DESIGN.md.
 *   - Measurement and A/B helpers that no reference interface corresponds to (event timers, per-kernel
 *     profiling, copy / fill / store-pattern ceilings, launch-shape overrides) live in mmdx_bench.h.
 */
#ifndef MMDX_H_INCLUDED
#define MMDX_H_INCLUDED

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__)
#define MMDX_API __attribute__((visibility("default")))
#else
#define MMDX_API
#endif

/* 2: mmdx_skeleton_desc.create_flags (was reserved0), the physics seam and graph entry points, unknown flag bits are
 *    rejected, bench / debug entry points moved to mmdx_bench.h (same library). */
/* 3: mmdx_placement_info.store_flags (the library keeps no table of array addresses any more: the caller carries the probe's
 *    verdict into mmdx_deform_args.flags); shared morph rates that did not change are detected by the library itself.
 *    Added later without a version change (additive, same struct sizes): MMDX_OUT_PITCHED with
 *    mmdx_deform_args.out_instance_pitch (was reserved0), mmdx_model_output_pitch, mmdx_crowd_output_alloc_pitched.  A library
 *    without them rejects the flag bit as unknown, so a caller that needs pitched outputs fails loudly there.
 *    mmdx_deform_batched_bounds (a new entry point; mmdx_deform_args unchanged).
 *    mmdx_deform_batched_select with mmdx_instance_select (a new entry point and structure; mmdx_deform_args unchanged).
 *    mmdx_cull_bounds with mmdx_cull_view / mmdx_cull_args and mmdx_cull_planes_from_matrix (new entry points and structures;
 *    nothing existing changes).
 *    mmdx_palette_place with mmdx_place_args, MMDX_PLACE_ON_DEVICE and MMDX_PLACE_MATRIX (a new entry point, structure and two
 *    flag bits no other call accepts; nothing existing changes).
 *    mmdx_palette_bounds with mmdx_palette_bounds_args, and mmdx_model_get_bone_boxes with mmdx_bone_box_info (two new entry points
 *    and structures; mmdx_model_info, mmdx_deform_args and every existing call are unchanged).
 *    mmdx_skeleton_solve_select (a new entry point that takes the existing mmdx_instance_select; nothing existing changes).
 *    mmdx_motion_set_clip_frames and the mmdx_animator_* family with mmdx_animator_desc / _clip / _info / _arrays and
 *    MMDX_ANIM_DT_ON_DEVICE (new entry points, structures and a flag bit no other call accepts; nothing existing changes).
 *    mmdx_motion_set_blend_bones_time_select, mmdx_motion_set_blend_morphs_time_select and
 *    mmdx_skeleton_solve_motion_set_blend_time_select (new entry points over the existing mmdx_motion_blend_args and
 *    mmdx_instance_select; nothing existing changes).
 *    mmdx_pose_blend and mmdx_rate_blend with mmdx_row_blend_args, MMDX_MASK_NONE and MMDX_BLEND_A_ON_DEVICE / _B_ / _PARAMS_, and
 *    mmdx_skeleton_subtree_mask (new entry points, a structure and three flag bits no other call accepts; nothing existing changes).
 *    mmdx_animator_root_motion with mmdx_root_motion_args and MMDX_ROOT_X / _Y / _Z, mmdx_bone_motion_in_place, and
 *    mmdx_bone_motion_get_keys with mmdx_bone_motion_keys (three new entry points and two structures; nothing existing changes).
 *    mmdx_pose_add and mmdx_rate_add with mmdx_row_add_args and MMDX_REF_NONE (two new entry points and a structure over the
 *    blend's flag bits; nothing existing changes).
 *    mmdx_animator_root_motion_turn with mmdx_root_turn_args and MMDX_ROOT_NORMALIZE, and mmdx_bone_motion_in_place_turn (two new
 *    entry points, a structure and a flag bit no other call accepts; nothing existing changes).
 *    mmdx_socket_set_create / _destroy / _get_info and mmdx_palette_sockets with mmdx_socket_set_desc / _info, mmdx_sockets_args and
 *    MMDX_SOCKET_OFFSET_MATRIX (four new entry points, three structures and a flag of the new desc alone; nothing existing changes).
 *    mmdx_spring_set_create / _destroy / _get_info, mmdx_spring_step and mmdx_spring_get_state / _set_state with
 *    mmdx_spring_set_desc / _info, mmdx_spring_args, MMDX_SPRING_RESET and MMDX_SPRING_DT_ON_DEVICE (six new entry points, three
 *    structures and two flag bits no other call accepts; nothing existing changes).
 *    mmdx_aim_set_create / _destroy / _get_info and mmdx_palette_aim with mmdx_aim_set_desc / _info, mmdx_aim_args and
 *    MMDX_AIM_TARGETS_ON_DEVICE (four new entry points, three structures and a flag bit no other call accepts; nothing existing
 *    changes).
 *    mmdx_reach_set_create / _destroy / _get_info and mmdx_palette_reach with mmdx_reach_set_desc / _info, mmdx_reach_args,
 *    MMDX_REACH_TARGETS_ON_DEVICE and MMDX_REACH_KEEP_END_ROTATION (four new entry points, three structures, a flag bit no other
 *    call accepts and a flag of the new desc alone; nothing existing changes).
 *    mmdx_ground_create / _destroy / _get_info, mmdx_ground_place and mmdx_ground_targets with mmdx_ground_desc / _info,
 *    mmdx_ground_place_args and mmdx_ground_targets_args (five new entry points and four structures; nothing existing changes). */
#define MMDX_ABI_VERSION 3u

typedef int32_t mmdx_status;
enum {
    MMDX_OK = 0,
    MMDX_ERR_INVALID_ARGUMENT = 1, /* NULL / size / flag problems                                  */
    MMDX_ERR_BAD_INDEX = 2,        /* a bone, vertex or morph index in the model is out of range   */
    MMDX_ERR_NO_DEVICE = 3,        /* no usable HIP device (the product has no CPU fallback)       */
    MMDX_ERR_HIP = 4,              /* a HIP runtime call failed; see mmdx_last_error_string()      */
    MMDX_ERR_OUT_OF_MEMORY = 5,
    MMDX_ERR_UNSUPPORTED = 6       /* e.g. morph group cycle, > 65535 bones in one vertex tile     */
};

/* Deform-type tags = PMX / libmmd values (L/model/model.inl:23-28).  Any other value is legal and
 * takes the reference's `default:` branch, i.e. is evaluated as BDEF2 (poser_impl.inl:417-418).
 * SDEF is evaluated as BDEF2 as well: the reference's spherical-deform code is commented out
 * ("UNDONE", poser_impl.inl:438-458). */
enum { MMDX_SKIN_BDEF1 = 0, MMDX_SKIN_BDEF2 = 1, MMDX_SKIN_BDEF4 = 2, MMDX_SKIN_SDEF = 3 };

/* Morph-type tags (L/model/model.inl:488-498).  Only GROUP and VERTEX move vertices; BONE feeds the
 * host's bone solve; UV / EXT_UV / MATERIAL are ignored by the reference path and by this engine. */
enum { MMDX_MORPH_GROUP = 0, MMDX_MORPH_VERTEX = 1, MMDX_MORPH_BONE = 2, MMDX_MORPH_UV = 3,
       MMDX_MORPH_MATERIAL = 8 };

/* mmdx_model_desc.flags */
enum {
    MMDX_CREATE_NORMALIZE = 1u << 0, /* apply Model::Normalize retagging (needs bone_parent)        */
    MMDX_CREATE_HOST_ONLY = 1u << 1, /* build + validate the plan only; touch no device (for tests
                                        and tools on machines without a GPU; deform then fails)     */
    MMDX_CREATE_F16_POSITIONS = 1u << 2, /* keep base positions and morph offsets as IEEE binary16 in
                                        HBM (rounded to nearest even once, here); arithmetic stays
                                        f32.  Bandwidth-stress configuration, not reference parity */
    MMDX_CREATE_FAST_MATH = 1u << 3, /* OPT-IN: the deform kernels of this model may contract a multiply and the add
                                        that consumes it into one fused multiply-add (one rounding instead of two), as
                                        any compiler does to L/motion/poser_impl.inl:396-437 at -ffp-contract=fast.
                                        Same operations in the same order, same epsilon tests and morph skips; results
                                        are then NOT bit-identical to libmmd's but within the tolerance stated and
                                        tested in tests/test_fast_math.py: |x - x_ref| <= 1e-5 * (1 + |x_ref|) per
                                        position component (measured on the benchmark models: 2.4e-6, a handful of
                                        binary32 ulps), <= 2e-6 per normal component (measured 1.8e-7), binary16
                                        positions within that plus one binary16 ulp.  Buys 5-8 % throughput.
                                        Without this flag (the default) every result is bit-identical to the reference's. */
    MMDX_CREATE_TILE_ORDER = 1u << 4 /* OPT-IN: every output array of this model (pose_image SoA, the 32-byte vertex, the
                                        f16 layout) holds the vertices in the ENGINE's order instead of the file's: inside
                                        each run of 512 consecutive file vertices they are sorted by deform class and
                                        morph-row length (mmdx_model_get_vertex_order returns the permutation).  Values
                                        are bit-identical to the default's, only their position in the array changes.
                                        The kernels then store straight from registers -- no on-chip transpose, no
                                        per-instance barrier: 3 % for the shared-morph crowd, 9 % for batches with per-instance morph weights
                                        (use with mmdx_crowd_output_alloc).  A renderer
                                        adopts it by remapping its index buffer once at load (main.cpp:781-787:
                                        index[i] = original_to_engine[index[i]]); INTEGRATION.md 1d''.                  */
};

/* Flat model description.  All pointers are host pointers, borrowed for the duration of the call. */
typedef struct mmdx_model_desc {
    uint32_t struct_size; /* = sizeof(mmdx_model_desc)                                             */
    uint32_t flags;       /* MMDX_CREATE_*                                                         */
    uint32_t n_vertices, n_bones, n_morphs;
    uint32_t reserved0;
    const float *positions;    /* [NV][3]                                                          */
    const float *normals;      /* [NV][3]                                                          */
    const float *uvs;          /* [NV][2] or NULL (zeros)                                          */
    const int32_t *skin_type;  /* [NV] MMDX_SKIN_* (raw PMX tag)                                    */
    const int32_t *bone_ids;   /* [NV][4]  BDEF1: [0]; BDEF2/SDEF: [0],[1]; BDEF4: [0..3]          */
    const float *bone_weights; /* [NV][4]  BDEF2/SDEF: [0] = weight of bone [0]; BDEF4: [0..3]     */
    const float *sdef_params;  /* [NV][9] C,R0,R1 or NULL -- accepted, validated for size only      */
    const int32_t *bone_parent; /* [NB] (-1 = none) or NULL; used only by MMDX_CREATE_NORMALIZE    */
    const int32_t *morph_type;  /* [NM] MMDX_MORPH_*                                               */
    const uint32_t *morph_offset; /* [NM+1] entry range of morph m = [off[m], off[m+1])            */
    const uint32_t *morph_index;  /* [E] vertex index (VERTEX) / morph index (GROUP) / other       */
    const float *morph_value;     /* [E][3] offset xyz (VERTEX) / {rate,-,-} (GROUP) / other       */
} mmdx_model_desc;

typedef struct mmdx_model_s *mmdx_model_t;

/* Output layouts */
enum {
    MMDX_OUT_SOA = 0,      /* out_a = f32 pos[NI][NV][3], out_b = f32 nrm[NI][NV][3]
                              (= Poser::pose_image.coordinates / .normals)                          */
    MMDX_OUT_VERTEX32 = 1, /* out_a = struct{f32 pos[3]; f32 normal[3]; f32 uv[2];}[NI][NV]
                              (= main.cpp:50-54); out_b unused                                     */
    MMDX_OUT_SOA_POS16 = 2 /* out_a = f16 pos[NI][NV][3], out_b = f32 nrm[NI][NV][3]               */
};

/* mmdx_deform_args.flags */
enum {
    MMDX_PALETTE_ON_DEVICE = 1u << 0, /* palettes is a device pointer (else host, copied per call)  */
    MMDX_WEIGHTS_ON_DEVICE = 1u << 1, /* morph_weights is a device pointer                          */
    MMDX_OUT_ON_DEVICE = 1u << 2,     /* out_a/out_b are device pointers (else host; D2H + sync)   */
    MMDX_WEIGHTS_SHARED = 1u << 3,    /* one morph_weights[NM] for all instances (crowd with shared
                                         facial state): the morph pass runs once per call          */
    MMDX_MORPH_UNCHANGED = 1u << 4,   /* with MMDX_WEIGHTS_SHARED and NI > 1: the morph weights are those of the
                                         previous such call on this model (a crowd whose facial state
                                         changes less often than its poses): the morphed positions of that
                                         call are reused and the morph pass is skipped; morph_weights is
                                         not read.  An error without such an earlier call.
                                         WITHOUT this flag the library finds out by itself (the reference's vertex_images_
                                         depends on morph_rates_ only, L/motion/poser_impl.inl:362-386): shared rates in host
                                         memory are compared with the ones of the pass whose result the handle holds and the
                                         pass (launch and upload) is skipped when they are bit for bit the same; shared rates
                                         in device memory are compared by the morph pass itself, on the device, which then
                                         skips its walk over the morph table (the launch remains: ~2 us instead of ~9).  The
                                         flag is the caller's promise and saves that launch too.                  */
    /* Hints for crowds whose outputs stream through the caches (device arrays of >= 512 MB per call): how the kernel
       writes them -- cached non-temporal stores (best where the arrays' physical backing is in the fast store mode, see
       mmdx_crowd_output_alloc) or write-through stores (~5 % faster everywhere else, 2 % slower in the fast mode).
       mmdx_crowd_output_alloc returns the right one for its arrays in mmdx_placement_info.store_flags; a caller who has
       measured its own arrays (mmdx_bench_store_pattern against mmdx_bench_fill, mmdx_bench.h) can say so too.  Without
       a hint such outputs are written through (six plain allocations in seven are not in the fast mode).  The decision
       is made from the call's arguments alone: the library remembers nothing about array addresses.  Results are
       identical either way; kernels without a write-through flavour ignore the hint; the two exclude each other.   */
    MMDX_OUT_STORES_WRITE_THROUGH = 1u << 5,
    MMDX_OUT_STORES_CACHED = 1u << 6,
    /* Instance pitch: instance i of out_a and out_b starts at element i * out_instance_pitch instead of i * NV, counted in
       vertices of the layout (12 / 12 bytes for MMDX_OUT_SOA, 32 for MMDX_OUT_VERTEX32, 6 / 12 for MMDX_OUT_SOA_POS16), so
       the arrays hold [NI][pitch] vertices.  out_instance_pitch >= NV.  THE GAP IS NEVER WRITTEN: the bytes of vertices
       [NV, pitch) of every instance keep whatever they held, on every output path (device, page-locked host, pageable
       host).  A pitch from mmdx_model_output_pitch starts every instance on a 64-byte boundary -- the layout a renderer
       needs to bind instances of one vertex buffer at aligned offsets, and the one whose crowd stores run the fast
       copy-out for any vertex count.  Without the flag out_instance_pitch is not read. */
    MMDX_OUT_PITCHED = 1u << 7
};

typedef struct mmdx_deform_args {
    uint32_t struct_size;  /* = sizeof(mmdx_deform_args)                                           */
    uint32_t flags;        /* MMDX_*_ON_DEVICE | MMDX_WEIGHTS_SHARED                               */
    uint32_t n_instances;  /* NI >= 1                                                              */
    uint32_t out_layout;   /* MMDX_OUT_*                                                           */
    const float *morph_weights; /* [NI][NM], or [NM] with MMDX_WEIGHTS_SHARED; may be NULL if NM==0 */
    const float *palettes;      /* [NI][NB][16]                                                    */
    void *out_a;
    void *out_b;
    float pos_scale; /* positions are multiplied by this AFTER the transform, as a separate f32
                        multiply (main.cpp:848-850 uses 0.1f); 1.0f = leave as pose_image          */
    uint32_t out_instance_pitch; /* with MMDX_OUT_PITCHED: vertices from one instance's output to the next's
                                    (>= NV); read only with that flag                              */
} mmdx_deform_args;

typedef struct mmdx_model_info {
    uint32_t struct_size;
    uint32_t n_vertices, n_bones, n_morphs;
    uint32_t n_slots;          /* vertex-morph applications in the reference's traversal order      */
    uint32_t n_entries;        /* vertex-morph entries after group expansion                       */
    uint32_t n_entries_padded; /* ... incl. the padding of the sliced-ELL gather table               */
    uint32_t n_tiles, tile_vertices;
    uint32_t n_bdef1, n_bdef2, n_bdef4; /* after optional Normalize; SDEF/unknown count as bdef2   */
    uint32_t max_tile_bones;
    uint64_t device_bytes;     /* static streams resident in HBM                                   */
    uint32_t device_ordinal;
    uint32_t flags;
    uint32_t reserved0;
} mmdx_model_info;

/* ---- library / device ------------------------------------------------------------------------ */
MMDX_API uint32_t mmdx_abi_version(void);
MMDX_API const char *mmdx_last_error_string(void);
MMDX_API mmdx_status mmdx_device_count(int32_t *count);
/* Device for the models, motions and buffers the CALLING THREAD creates from now on (like hipSetDevice), and the
 * default for threads that never select one.  A handle stays on the device it was created on and may be used
 * from any thread, one call at a time per handle; handles on different devices (or on the same one: each has its
 * own stream) run concurrently from different host threads -- the in-process form of the instance-sharded crowd. */
MMDX_API mmdx_status mmdx_device_select(int32_t ordinal);
MMDX_API mmdx_status mmdx_device_name(int32_t ordinal, char *buf, size_t buf_size);

/* ---- model ----------------------------------------------------------------------------------- */
MMDX_API mmdx_status mmdx_model_create(const mmdx_model_desc *desc, mmdx_model_t *out_model);
MMDX_API mmdx_status mmdx_model_destroy(mmdx_model_t model);
MMDX_API mmdx_status mmdx_model_get_info(mmdx_model_t model, mmdx_model_info *info);
/* Post-Normalize skin tags in ORIGINAL vertex order: type[NV] (0,1,2), ids[NV][4], weights[NV][4]. */
MMDX_API mmdx_status mmdx_model_get_skin(mmdx_model_t model, int32_t *type, int32_t *ids,
                                         float *weights);
/* The engine's vertex order (a permutation of [0, NV) that only moves vertices inside their tile of 512 consecutive file
 * vertices): engine_to_original[e] = file index of the vertex at position e of an MMDX_CREATE_TILE_ORDER model's outputs,
 * original_to_engine = its inverse (what an index buffer is remapped through).  Either pointer may be NULL.  Defined for every
 * model; only MMDX_CREATE_TILE_ORDER models write their outputs in this order. */
MMDX_API mmdx_status mmdx_model_get_vertex_order(mmdx_model_t model, uint32_t *engine_to_original /*[NV]*/,
                                                 uint32_t *original_to_engine /*[NV]*/);
/* Host-side flattening of group morphs: slot_weights[n_slots] for one set of morph rates, exactly
 * what the device consumes (a slot whose chain hits the reference's `rate < 1e-7` skip gets 0). */
MMDX_API mmdx_status mmdx_model_slot_weights(mmdx_model_t model, const float *morph_weights,
                                             float *slot_weights);
/* Borrow an external HIP stream (hipStream_t) instead of the handle's own; NULL restores it.  Every entry point that takes
 * `model` -- deform, bounds, select, cull, place, palette bounds, the motion and rig calls, graph recording, mmdx_sync --
 * then enqueues on that stream and on no other.
 *  - Order across a switch: work enqueued after the switch starts after ALL work this model enqueued before it, on whichever
 *    stream (the new stream waits for an event on the old one; the host never blocks, and a switch to the stream the model
 *    already has does nothing).  The model's device state -- morphed positions, scratch buffers -- moves with it safely.
 *  - A switch between mmdx_graph_begin and mmdx_graph_end is refused (MMDX_ERR_INVALID_ARGUMENT), the recording goes on.
 *  - A graph replays on the stream it was recorded on, also after the model has left that stream.
 *  - Lifetime: the borrowed stream must stay alive until the model has been switched away from it (or destroyed) AND the
 *    graphs recorded on it are destroyed.  mmdx_model_destroy waits for the model's current stream, which is ordered behind
 *    everything earlier.
 *  - The stream must belong to the model's device: another device's stream is refused (MMDX_ERR_INVALID_ARGUMENT).
 * A host-only model has no stream: MMDX_ERR_NO_DEVICE. */
MMDX_API mmdx_status mmdx_model_set_stream(mmdx_model_t model, void *hip_stream);

/* ---- HIP-graph replay of a frame's device work ------------------------------------------------------
 * Between mmdx_graph_begin and mmdx_graph_end everything the library enqueues on `model`'s stream is RECORDED instead
 * of executed: mmdx_deform_batched, mmdx_morph_motion_eval, mmdx_bone_motion_eval and mmdx_skeleton_solve* called with
 * this model and every operand in device memory (MMDX_*_ON_DEVICE).  mmdx_graph_launch then replays the whole sequence
 * with ONE submission (asynchronous, on the model's stream); the recorded calls read and write the same device
 * addresses on every replay, so a frame is "update the inputs in place, launch".  What it buys is host time: a
 * frame of motion -> poses -> palettes -> vertices is four to six launches (~4 us of host time each); the device-side
 * gaps between dependent kernels are the same either way.  Rules: run the same sequence once un-captured first (it
 * sizes the handles' scratch buffers; a call that would have to allocate while recording fails), no host operands,
 * no mmdx_profile_enable while recording, one recording per model at a time; mmdx_graph_end on the thread that called
 * mmdx_graph_begin.
 * Lifetime: a graph holds raw device addresses of the scratch buffers of every handle that took part in the recording
 * (the model, and skeletons / motions called with it).  While the graph is alive those handles are pinned: a later call
 * on them that would have to GROW such a buffer fails with MMDX_ERR_INVALID_ARGUMENT instead of moving it (size the
 * buffers with an un-recorded call of the largest shape first); destroying a pinned handle is allowed and invalidates
 * the graph -- mmdx_graph_launch then fails, it never replays into freed memory.  A skeleton or motion destroyed WHILE
 * a recording that used it is in progress poisons that recording (mmdx_graph_end reports it and returns no graph; its
 * device blocks are freed at mmdx_graph_end, the runtime refuses frees on a recording thread); a model destroyed in
 * the middle of its own recording ends the recording.  Recorded calls come from the thread that called
 * mmdx_graph_begin. */
typedef struct mmdx_graph_s *mmdx_graph_t;
MMDX_API mmdx_status mmdx_graph_begin(mmdx_model_t model);
MMDX_API mmdx_status mmdx_graph_end(mmdx_model_t model, mmdx_graph_t *out_graph);
MMDX_API mmdx_status mmdx_graph_launch(mmdx_graph_t graph);
MMDX_API void mmdx_graph_destroy(mmdx_graph_t graph);

/* ---- the hot path ---------------------------------------------------------------------------- */
/* deform(model, morph_weights, bone_palette, out_verts): one instance, host pointers, synchronous.
 * out_pos/out_nrm = f32[NV][3] each = Poser::pose_image after Poser::Deform(). */
MMDX_API mmdx_status mmdx_deform(mmdx_model_t model, const float *morph_weights /*[NM]*/,
                                 const float *palette /*[NB][16]*/, float *out_pos, float *out_nrm);
/* Same, producing the viewer's interleaved 32-byte vertices (Deform + UpdateDeformedVertices). */
MMDX_API mmdx_status mmdx_deform_vertex32(mmdx_model_t model, const float *morph_weights,
                                          const float *palette, float pos_scale,
                                          void *out_vertices /*[NV] x 32 B*/);
/* General / crowd form.  Asynchronous on the handle's stream when every pointer is a device pointer;
 * otherwise returns after the copies have completed. */
MMDX_API mmdx_status mmdx_deform_batched(mmdx_model_t model, const mmdx_deform_args *args);
/* mmdx_deform_batched plus where every instance ended up, for culling, LOD and shadow-frustum fitting without reading the
 * vertices back or passing over them again: out_bounds[i][6] = {min x, min y, min z, max x, max y, max z} of instance i.
 * Everything else is exactly mmdx_deform_batched(model, args): same flags, layouts, pitch, morph modes, output paths, graph
 * recording and validation (unknown flag bits included); the outputs are bit-identical.
 * Contract:
 *  - bounds are taken over the positions AS WRITTEN: vertices [0, NV) of the instance, never the pitch gap; pos_scale applied;
 *    for MMDX_OUT_SOA_POS16 the binary16 values widened to f32.  So every bound is a value that occurs in the output.
 *  - comparisons follow IEEE rules: NaN coordinates are skipped, a component that is NaN at every vertex gives NaN, +-inf take
 *    part, -0.0 and +0.0 compare equal (which of the two is returned is unspecified).
 *  - out_bounds lives where the outputs live: a device pointer (4-byte aligned) with MMDX_OUT_ON_DEVICE, written in the
 *    model's stream order like the outputs; otherwise a host pointer, filled when the call returns.  NULL is
 *    MMDX_ERR_INVALID_ARGUMENT.
 * Routes: a single frame that mmdx_deform_batched gives to its one-frame kernel (MMDX_FRAME_KERNEL) and per-instance weights
 * under the opt-in MMDX_FUSED_PACK=1 run the crowd kernel's bounds flavour instead.  That flavour stores cached: a bounds call
 * accepts MMDX_OUT_STORES_WRITE_THROUGH and ignores it.  The per-(instance, tile) partial bounds live in a per-call scratch
 * buffer of the handle, which a recorded graph pins like the others (see the graph section). */
MMDX_API mmdx_status mmdx_deform_batched_bounds(mmdx_model_t model, const mmdx_deform_args *args, float *out_bounds /*[NI][6]*/);

/* ---- deforming a subset of a crowd: an instance list and a count that may live in device memory -------------------------------
 * For a renderer that has decided ON THE GPU (from mmdx_deform_batched_bounds' result, say) which instances are in view:
 * no read-back, no re-packing of palettes, every instance keeps its slot of the vertex buffer. */
enum { MMDX_SELECT_ON_DEVICE = 1u << 0 };   /* ids and count are device pointers (else host memory, copied per call) */
typedef struct mmdx_instance_select {
    uint32_t struct_size;   /* = sizeof(mmdx_instance_select)                                                        */
    uint32_t flags;         /* MMDX_SELECT_*; unknown bits are MMDX_ERR_INVALID_ARGUMENT                              */
    const uint32_t *ids;    /* [n_ids] instance indices into the call's arrays, any order                            */
    const uint32_t *count;  /* optional: how many leading ids are in use; NULL = n_ids; lives where ids lives        */
    uint32_t n_ids;         /* capacity of ids; the launch is sized from it                                          */
    uint32_t reserved0;     /* 0                                                                                     */
} mmdx_instance_select;
/* mmdx_deform_batched (out_bounds == NULL) or mmdx_deform_batched_bounds (out_bounds != NULL) for the listed instances only.
 *  1. `args` means what it means for mmdx_deform_batched: n_instances = NI is the extent of palettes, morph_weights, out_a, out_b
 *     (and out_bounds); instance i reads row i and writes at i * NV or i * out_instance_pitch.  The list only says which i take part.
 *  2. For every listed i < NI the bytes written to out_a, out_b and out_bounds[i] are identical to what mmdx_deform_batched /
 *     mmdx_deform_batched_bounds write for that instance with the same args: every layout, pos_scale, dense and pitched, shared /
 *     per-instance / no morph weights, MMDX_MORPH_UNCHANGED and the automatic morph skip, tile-order and fast-math models.  The
 *     store hints MMDX_OUT_STORES_* are accepted and ignored (select launches store cached).
 *  3. Nothing else is written: outputs and bounds rows of instances that are not listed keep what they held, as does every
 *     instance's pitch gap.  Palettes and per-instance weights of unlisted instances may hold anything (uninitialised memory,
 *     NaN): if they are read at all they influence no written byte.
 *  4. The first min(*count, n_ids) ids are used.  *count == 0 or n_ids == 0 is a valid call that writes no instance; the shared
 *     morph pass and its skip record behave as in the plain call, so a later MMDX_MORPH_UNCHANGED call is legal.
 *  5. An id >= NI: in a host list the call fails with MMDX_ERR_INVALID_ARGUMENT before anything is launched; in a device list the
 *     entry is skipped on the device (nothing read or written for it).  An id that occurs twice is allowed and costs twice (both
 *     writers store the same bytes).
 *  6. The GPU-resident crowd form only: MMDX_PALETTE_ON_DEVICE | MMDX_OUT_ON_DEVICE are required, and MMDX_WEIGHTS_ON_DEVICE when
 *     morph_weights is passed; out_bounds is then a device pointer.  Anything else is MMDX_ERR_INVALID_ARGUMENT (the staging and
 *     bounce copies of host operands move whole arrays and cannot honour rule 3).  A host-resident list is supported (a host-side
 *     culler can use the call too): it is copied to a scratch buffer of the handle in stream order, and the call returns after
 *     its work has completed, like every call that borrows host memory.
 *  7. With a device list the call is asynchronous on the handle's stream like the plain device call and records into a graph
 *     (mmdx_graph_begin / mmdx_graph_end; a host list is refused while recording).  A replay uses whatever ids / *count hold in
 *     device memory at replay time.  ids and count are 4-byte aligned.
 *  8. select == NULL is MMDX_ERR_INVALID_ARGUMENT: callers who want every instance call the plain entry points.
 * The launch is sized from n_ids: workgroups whose list positions lie behind *count return at once, so a capacity far above the
 * usual count costs little, but keep n_ids to what the list can hold. */
MMDX_API mmdx_status mmdx_deform_batched_select(mmdx_model_t model, const mmdx_deform_args *args,
                                                const mmdx_instance_select *select, float *out_bounds /* [NI][6] or NULL */);
MMDX_API mmdx_status mmdx_sync(mmdx_model_t model);

/* ---- culling and LOD on the device: the boxes of mmdx_deform_batched_bounds -> the lists of mmdx_deform_batched_select ----------
 * The middle of the GPU-resident crowd loop: bounds (one box per instance, device memory) are tested against up to 16 planes and
 * sorted by distance into up to 4 level-of-detail lists, without a read-back.  List l is out_ids + l * list_stride with its length
 * at out_counts + l: EXACTLY what mmdx_instance_select.ids / .count take (MMDX_SELECT_ON_DEVICE, n_ids = n_instances), so a frame is
 * mmdx_deform_batched_bounds -> mmdx_cull_bounds -> mmdx_deform_batched_select, recorded once and replayed.
 *
 * The arithmetic is part of the contract (the library is built with -ffp-contract=off).  Every operation is binary32,
 * unfused, in this order, with m(a, b) = a > b ? a : b; a row of bounds is {min x, min y, min z, max x, max y, max z}:
 *   box      lo = min - margin, hi = max + margin, per component.
 *   plane p  px = a >= 0 ? hi.x : lo.x, likewise py (b) and pz (c); s = ((a*px + b*py) + c*pz) + d.  The instance is culled iff
 *            s < 0 for some p < n_planes.  A NaN s never culls: a row that was never written (NaN) stays visible, and so does every
 *            instance against a NaN plane.
 *   level    from the box WITHOUT the margin: dx = m(m(min.x - eye.x, eye.x - max.x), 0.0f), likewise dy, dz;
 *            d2 = (dx*dx + dy*dy) + dz*dz; level = the number of k < n_lods - 1 with d2 >= lod_distance[k] * lod_distance[k]
 *            (a NaN d2 gives level 0).
 *   lists    list l holds the visible instances of level l IN ASCENDING INSTANCE ORDER (no atomics decide an order: two runs, and
 *            a CPU restatement of the lines above, agree byte for byte); out_counts[l] is its length, out_counts[l] = 0 for
 *            n_lods <= l < MMDX_CULL_MAX_LODS; entries of out_ids behind a count keep what they held; out_levels[i] (when given)
 *            = the level of instance i, or MMDX_CULLED, for every i < n_instances.
 * n_instances == 0 is valid and writes only the zero counts.
 * The planes are used as given (not normalised): the box is grown by `margin` in world units, which moves a plane's verdict by
 * margin * (|a| + |b| + |c|), i.e. in PLANE UNITS; planes from mmdx_cull_planes_from_matrix are not unit length, so a caller who
 * wants `margin` to act as a distance to the plane normalises them first.  margin is how stale bounds are used safely: bounds of the previous frame,
 * grown by how far an instance can move in one frame. */
#define MMDX_CULL_MAX_PLANES 16
#define MMDX_CULL_MAX_LODS    4
#define MMDX_CULLED 0xFFFFFFFFu

typedef struct mmdx_cull_view {       /* POD, 4-byte aligned, host OR device memory                                     */
    float    planes[MMDX_CULL_MAX_PLANES][4]; /* (a,b,c,d); a point is inside when a*x+b*y+c*z+d >= 0                  */
    uint32_t n_planes;                /* 0..16; 0 = nothing is culled                                                   */
    uint32_t n_lods;                  /* 1..4 lists                                                                     */
    float    eye[3];                  /* LOD distances are measured from here to the box                                */
    float    margin;                  /* >= 0: the box is grown by this on every side before the plane test             */
    float    lod_distance[MMDX_CULL_MAX_LODS - 1]; /* ascending; level = how many of the first n_lods-1 the box has reached */
    uint32_t reserved0;               /* 0                                                                              */
} mmdx_cull_view;

enum { MMDX_CULL_VIEW_ON_DEVICE = 1u << 0 }; /* view is a device pointer, read when the kernel RUNS */

typedef struct mmdx_cull_args {
    uint32_t struct_size, flags;      /* = sizeof(mmdx_cull_args); MMDX_CULL_*, unknown bits: MMDX_ERR_INVALID_ARGUMENT */
    uint32_t n_instances;             /* rows of bounds                                                                 */
    uint32_t list_stride;             /* list l starts at out_ids + l * list_stride; >= n_instances                     */
    const float *bounds;              /* device [NI][6], as mmdx_deform_batched_bounds writes it                        */
    const mmdx_cull_view *view;
    uint32_t *out_ids;                /* device [n_lods][list_stride]                                                   */
    uint32_t *out_counts;             /* device [MMDX_CULL_MAX_LODS]; entries >= n_lods are written 0                   */
    uint32_t *out_levels;             /* device [NI] or NULL: level of instance i, or MMDX_CULLED                       */
} mmdx_cull_args;

/* `model` supplies the device, the stream (the call is asynchronous on it, in order with the model's deform calls), the graph
 * recording and, for crowds large enough to take two launches, a per-chunk count scratch that a recorded graph pins like the
 * model's other scratch buffers (run the call once un-recorded first, see the graph section).
 *  - A view in host memory (no flag) is validated in full before anything touches the device -- n_planes > 16, n_lods outside 1..4,
 *    a negative or NaN margin, descending or NaN lod_distance[0 .. n_lods-2], reserved0 != 0: MMDX_ERR_INVALID_ARGUMENT -- and
 *    then passed to the kernel BY VALUE: it may be changed or freed as soon as the call returns, and the call records into a graph
 *    (every replay then uses the recorded view).  It is read by the CPU: pass device memory with the flag only.
 *  - A view in device memory (MMDX_CULL_VIEW_ON_DEVICE) is read when the kernel runs: a recorded call reads it afresh at every
 *    replay, so a frame is "write the new planes and eye into the view, launch".  It cannot be checked: on the device n_planes and
 *    n_lods are clamped to their maxima (n_lods == 0 acts as 1) and a NaN or negative margin acts as the arithmetic says.  out_ids
 *    must have room for the n_lods the view holds when the kernel runs (MMDX_CULL_MAX_LODS lists always suffice).
 *  - list_stride < n_instances, a NULL bounds / view / out_ids / out_counts, device pointers that are not 4-byte aligned and a
 *    struct_size mismatch are MMDX_ERR_INVALID_ARGUMENT; a MMDX_CREATE_HOST_ONLY model is MMDX_ERR_NO_DEVICE (after validation).
 *    bounds and out_ids may be NULL when n_instances == 0. */
MMDX_API mmdx_status mmdx_cull_bounds(mmdx_model_t model, const mmdx_cull_args *args);
/* The six frustum planes of a clip-space transform, pure host code.  m is column-major as HandmadeMath's HMM_Mat4 stores it (and
 * OpenGL): element (r, c) is m[c*4+r], clip = m * (x, y, z, 1).  With row_r = (m[r], m[4+r], m[8+r], m[12+r]) the planes are, in
 * this order: left row3 + row0, right row3 - row0, bottom row3 + row1, top row3 - row1, near row3 + row2 (depth in [-w, w]) or
 * row2 alone when depth_zero_to_one (depth in [0, w]), far row3 - row2.  Each component is one binary32 add or subtract; the planes
 * are NOT normalised (see `margin` above). */
MMDX_API mmdx_status mmdx_cull_planes_from_matrix(const float m[16], uint32_t depth_zero_to_one, float out_planes[6][4]);

/* ---- plain device-memory helpers (thin hipMalloc / hipMemcpy wrappers) ----------------------- */
/* So that C, C++ and ctypes callers can keep palettes and outputs resident in HBM without linking
 * the HIP runtime themselves. */
MMDX_API mmdx_status mmdx_device_malloc(void **ptr, size_t bytes);
MMDX_API mmdx_status mmdx_device_free(void *ptr);
/* Page-locked host memory: palettes / rates handed to mmdx_deform*() from here move over PCIe by DMA
 * without the runtime's staging copy, and OUTPUT buffers from here (or any hipHostMalloc / hipHostRegister
 * memory) are written by the kernel directly -- no device-side staging buffer, no device-to-host copy
 * command: the single-model drop-in path (the viewer's vertex buffer, main.cpp:735-863).  Pageable
 * memory works everywhere too: frame-sized inputs / outputs go through page-locked bounce buffers owned by
 * the model (one extra CPU memcpy), larger ones through the runtime's staging copies. */
MMDX_API mmdx_status mmdx_host_malloc(void **ptr, size_t bytes);
MMDX_API mmdx_status mmdx_host_free(void *ptr);
MMDX_API mmdx_status mmdx_memcpy_h2d(void *dst_device, const void *src_host, size_t bytes);
MMDX_API mmdx_status mmdx_memcpy_d2h(void *dst_host, const void *src_device, size_t bytes);
MMDX_API mmdx_status mmdx_device_memset(void *dst_device, int value, size_t bytes);
MMDX_API mmdx_status mmdx_device_synchronize(void);
/* Placement-aware allocation of a crowd's output arrays ([n_instances][NV] in `out_layout`; out_b stays
 * NULL for MMDX_OUT_VERTEX32).  On MI355X the store rate of the crowd's output pattern is bimodal in WHERE
 * the driver places the arrays (same virtual addresses, different physical backing: ~0.97 or ~0.75 of the
 * linear-fill rate, stable for the life of the allocation; tools/archive/probes/alloc_probe.py, alloc_kernel_probe.py),
 * and the deform kernel follows it.  This helper allocates, times the store-only replay of the pattern
 * against a linear fill, and retries up to `max_tries` times (about one placement in seven is the fast
 * one; ~5 ms per try), keeping the best placement seen, then waits until the driver's background wipe of
 * the freed candidates no longer shows.  max_tries <= 1: plain allocation.  Free both arrays with
 * mmdx_device_free() (or hipFree: the library keeps no record of the arrays).  What the probe found comes back in
 * mmdx_placement_info.store_flags: OR it into mmdx_deform_args.flags of the crowd calls that write these arrays
 * (MMDX_OUT_STORES_* above) -- a performance hint only, results never depend on it, and its lifetime is the caller's:
 * it describes the physical backing of THIS allocation and is void once the arrays are freed. */
typedef struct mmdx_placement_info {
    uint32_t struct_size;
    uint32_t tries;          /* allocations made                                                        */
    uint32_t probed;         /* 0: layout / vertex count not probe-able, plain allocation               */
    float store_GBs;         /* store-only replay on the returned arrays                                */
    float fill_GBs;          /* linear fill of the same bytes (the yardstick)                           */
    uint32_t store_flags;    /* MMDX_OUT_STORES_CACHED (fast store mode found), MMDX_OUT_STORES_WRITE_THROUGH
                                (not found), or 0 (not probed: the library's default applies)            */
} mmdx_placement_info;
MMDX_API mmdx_status mmdx_crowd_output_alloc(mmdx_model_t model, uint32_t n_instances, int32_t out_layout,
                                             uint32_t max_tries, void **out_a_device, void **out_b_device,
                                             mmdx_placement_info *info /* may be NULL */);
/* The smallest instance pitch >= NV (in vertices, see MMDX_OUT_PITCHED) that starts every instance of `out_layout` on a
 * 64-byte boundary: NV rounded up to a multiple of 16 for MMDX_OUT_SOA, of 32 for MMDX_OUT_SOA_POS16, of 2 for
 * MMDX_OUT_VERTEX32 (at most 31 vertices of gap per instance).  Any pitch that keeps instances 16-byte aligned (a multiple of
 * 4 / 8 / 1) already takes the kernel's 16-byte copy-out; the 64-byte one is also as fast as a dense crowd whose vertex count is
 * a multiple of 16.  Plain arithmetic on the model: works on MMDX_CREATE_HOST_ONLY models.  MMDX_OUT_SOA_POS16
 * goes with MMDX_CREATE_F16_POSITIONS models only (MMDX_ERR_UNSUPPORTED otherwise, as in mmdx_deform_batched). */
MMDX_API mmdx_status mmdx_model_output_pitch(mmdx_model_t model, int32_t out_layout, uint32_t *pitch);
/* mmdx_crowd_output_alloc for pitched outputs: the arrays hold [n_instances][pitch] vertices of `out_layout` (pitch >= NV)
 * and the placement probe replays the pitched store pattern.  With a pitch that keeps every instance 16-byte aligned (one
 * from mmdx_model_output_pitch) the probe runs for any vertex count.  Pass the same pitch, with MMDX_OUT_PITCHED and
 * info->store_flags, to the mmdx_deform_batched calls that write these arrays. */
MMDX_API mmdx_status mmdx_crowd_output_alloc_pitched(mmdx_model_t model, uint32_t n_instances, int32_t out_layout,
                                                     uint32_t pitch, uint32_t max_tries, void **out_a_device,
                                                     void **out_b_device, mmdx_placement_info *info /* may be NULL */);

/* ---- PMX 2.0 loader (the data format on the input side of the path) --------------------------- */
/* From-scratch parser for the fields the deformation path consumes; replaces, for those fields,
 * PmxReader::ReadModel (L/reader/pmx_reader_impl.inl:16-449) + FileReader (L/util/dwarf_impl.inl:29-130)
 * with the same observable semantics (1/2-byte indices zero-extended, 4-byte sign-extended; UTF-16LE
 * or UTF-8 text; unknown deform / morph types are errors).  Display frames, rigid bodies and joints
 * are not read. */
typedef struct mmdx_pmx_s *mmdx_pmx_t;

typedef struct mmdx_pmx_info {
    uint32_t struct_size;
    uint32_t n_vertices, n_indices, n_textures, n_materials, n_bones, n_morphs, n_morph_entries;
    uint32_t extra_uv;        /* additional UV sets per vertex (skipped)                            */
    uint32_t utf8;            /* text encoding of the file: 1 = UTF-8, 0 = UTF-16LE                 */
    uint8_t index_width[8];   /* vertex, texture, material, bone, morph, rigid body; 2 spare        */
    uint64_t bytes_consumed;  /* file offset just behind the morph block                           */
} mmdx_pmx_info;

typedef struct mmdx_pmx_arrays {      /* pointers into the parsed model, valid until destroy       */
    uint32_t struct_size;
    uint32_t reserved0;
    const uint32_t *triangles;             /* [n_indices] original winding                         */
    const uint32_t *material_index_count;  /* [n_materials] consecutive index ranges               */
    const float *bone_rest_position;       /* [n_bones][3]                                         */
    const int32_t *bone_parent;            /* [n_bones], -1 = none                                 */
    const int32_t *bone_transform_level;   /* [n_bones]                                            */
    const uint16_t *bone_flags;            /* [n_bones] raw PMX bone flag word                     */
    const uint8_t *morph_panel;            /* [n_morphs]                                           */
    const float *edge_scale;               /* [n_vertices]                                         */
} mmdx_pmx_arrays;

enum { MMDX_PMX_NAME_MODEL = 0, MMDX_PMX_NAME_BONE = 1, MMDX_PMX_NAME_MORPH = 2,
       MMDX_PMX_NAME_MATERIAL = 3, MMDX_PMX_NAME_TEXTURE = 4 };

MMDX_API mmdx_status mmdx_pmx_parse(const void *data, size_t size, mmdx_pmx_t *out_pmx);
MMDX_API mmdx_status mmdx_pmx_load_file(const char *path, mmdx_pmx_t *out_pmx);
/* PMD 1.0, the older format: replaces PmdReader::ReadModel (L/reader/pmd_reader_impl.inl:16-566) for the same
 * fields and yields the same kind of handle, so every mmdx_pmx_* accessor below serves it (incl. the rig: PMD
 * bone types and IK list are converted to flag words, append and IK tables exactly as libmmd converts them;
 * a second IK record of one bone appends a bone, so n_bones can exceed the file's count).  All vertices
 * are BDEF2 with weight byte * 0.01f; morph indices are resolved through the base morph. */
MMDX_API mmdx_status mmdx_pmd_parse(const void *data, size_t size, mmdx_pmx_t *out_pmx);
MMDX_API mmdx_status mmdx_pmd_load_file(const char *path, mmdx_pmx_t *out_pmx);
MMDX_API void mmdx_pmx_destroy(mmdx_pmx_t pmx);
MMDX_API mmdx_status mmdx_pmx_get_info(mmdx_pmx_t pmx, mmdx_pmx_info *info);
/* Fills `desc` with pointers into `pmx` (valid until mmdx_pmx_destroy) and MMDX_CREATE_NORMALIZE,
 * ready for mmdx_model_create(): the reference's reader ends with model.Normalize() too. */
MMDX_API mmdx_status mmdx_pmx_get_model_desc(mmdx_pmx_t pmx, mmdx_model_desc *desc);
MMDX_API mmdx_status mmdx_pmx_get_arrays(mmdx_pmx_t pmx, mmdx_pmx_arrays *arrays);
/* Names as UTF-8 (bone and morph names are what VMD motion data is keyed by). */
MMDX_API mmdx_status mmdx_pmx_get_name(mmdx_pmx_t pmx, int32_t kind, uint32_t index, char *buf,
                                       size_t buf_size);

/* ---- VMD motion loader + morph-rate evaluation on the device (the per-frame input side) --------- */
/* Replaces, for morph tracks, VmdReader::ReadMotion (L/reader/vmd_reader_impl.inl:9-79),
 * MotionPlayer's name mapping (L/motion/poser_impl.inl:522-537) and Motion::GetMorphPose
 * (L/motion/motion_impl.inl:382-424): the rates a crowd needs -- [instances][morphs], every instance at
 * its own frame -- are produced in HBM, ready for mmdx_deform_batched(MMDX_WEIGHTS_ON_DEVICE).  Bone
 * keyframes are exposed raw (for a host bone solve) and evaluated on the device further below. */
typedef struct mmdx_vmd_s *mmdx_vmd_t;
typedef struct mmdx_morph_motion_s *mmdx_morph_motion_t;

typedef struct mmdx_vmd_info {
    uint32_t struct_size;
    uint32_t n_bone_records, n_morph_records; /* as stored in the file                              */
    uint32_t n_bone_tracks, n_morph_tracks;   /* distinct names                                     */
    uint32_t n_bone_keys, n_morph_keys;       /* after "last record for a (name, frame) wins"       */
    uint32_t max_frame;
    uint64_t bytes_consumed;                  /* camera / light / shadow sections follow; not read  */
} mmdx_vmd_info;

typedef struct mmdx_vmd_bone_key {            /* one 111-byte VMD bone record minus the name         */
    uint32_t frame;
    float translation[3];
    float rotation[4];                        /* quaternion x, y, z, w                               */
    int8_t interpolation[64];                 /* x, y, z, rotation: 16 bytes each, control points at
                                                 [0],[4],[8],[12] in units of 1/127                  */
} mmdx_vmd_bone_key;

enum { MMDX_FRAMES_ON_DEVICE = 1u << 0 };     /* with MMDX_OUT_ON_DEVICE for mmdx_morph_motion_eval  */
enum { MMDX_TIMES_ON_DEVICE = MMDX_FRAMES_ON_DEVICE };   /* the same bit, for the *_time entry points     */

MMDX_API mmdx_status mmdx_vmd_parse(const void *data, size_t size, mmdx_vmd_t *out_vmd);
MMDX_API mmdx_status mmdx_vmd_load_file(const char *path, mmdx_vmd_t *out_vmd);
MMDX_API void mmdx_vmd_destroy(mmdx_vmd_t vmd);
MMDX_API mmdx_status mmdx_vmd_get_info(mmdx_vmd_t vmd, mmdx_vmd_info *info);
MMDX_API mmdx_status mmdx_vmd_track_name(mmdx_vmd_t vmd, int32_t is_morph, uint32_t track, char *buf,
                                         size_t buf_size);   /* UTF-8 */
MMDX_API mmdx_status mmdx_vmd_bone_track(mmdx_vmd_t vmd, uint32_t track, const mmdx_vmd_bone_key **keys,
                                         uint32_t *n_keys);  /* sorted by frame */
MMDX_API mmdx_status mmdx_vmd_morph_track(mmdx_vmd_t vmd, uint32_t track, const uint32_t **frames,
                                          const float **weights, uint32_t *n_keys);
/* Associate the motion's morph tracks with a model's morphs by name (UTF-8, e.g. from
 * mmdx_pmx_get_name); morphs without a track evaluate to 0. */
MMDX_API mmdx_status mmdx_vmd_bind_morphs(mmdx_vmd_t vmd, uint32_t n_morphs,
                                          const char *const *morph_names_utf8,
                                          mmdx_morph_motion_t *out_motion);
MMDX_API mmdx_status mmdx_morph_motion_get_info(mmdx_morph_motion_t motion, uint32_t *n_morphs,
                                                uint32_t *n_mapped, uint32_t *n_keys);
/* out_weights[i][m] = rate of model morph m at frames[i], i < n_instances.  Runs on `model`'s device
 * and stream when `model` is given (so a following mmdx_deform_batched sees the result), else on the
 * selected device's default stream.  flags: MMDX_FRAMES_ON_DEVICE | MMDX_OUT_ON_DEVICE. */
MMDX_API mmdx_status mmdx_morph_motion_eval(mmdx_morph_motion_t motion, mmdx_model_t model,
                                            uint32_t n_instances, const uint32_t *frames,
                                            uint32_t flags, float *out_weights);
/* Time-based evaluation: MotionPlayer::SeekTime(double time) (L/motion/poser_impl.inl:548-555), i.e.
 * Motion::GetMorphPose(name, double time) (L/motion/motion_impl.inl:426-465) and GetBonePose(name, double
 * time) (:321-380) -- NOT the frame path at frame floor(time * 30):
 *   1. dframe = time * 30.0 in double; the clamps compare the key frames as doubles: the first key when
 *      first >= dframe, the last key when last <= dframe;
 *   2. the bracket is upper_bound(size_t(dframe)) (truncation);
 *   3. bary = (float)((dframe - left) / (right - left)), a double subtraction and division rounded once to
 *      float (the frame path: float(frame - left) / float(right - left) in f32);
 *   4. no exact-hit shortcut: at dframe == a key's frame the left key is interpolated at bary 0 (a curved
 *      key's first presample, the translation lerp and the renormalising NLerp still run; a morph weight next
 *      to an infinite one gives NaN), so SeekTime(k / 30.0) may differ from SeekFrame(k) in the last bits;
 *   5. dframe just below a key can round bary up to 1.0f: the curve's last sample and NLerp's right key;
 *   6. negative times and -inf give the first key, times past the end and +inf the last key.  NaN is
 *      undefined in the reference: host times that are NaN are rejected (MMDX_ERR_INVALID_ARGUMENT); device
 *      times that are NaN take the first key.
 * times[n_instances] are seconds, one per instance; flags, stream, device and graph rules as for the frame
 * entry points, MMDX_TIMES_ON_DEVICE (= MMDX_FRAMES_ON_DEVICE) for device times.  Unknown flag bits are
 * rejected.  out_weights[i][m] = rate of model morph m at times[i]. */
MMDX_API mmdx_status mmdx_morph_motion_eval_time(mmdx_morph_motion_t motion, mmdx_model_t model,
                                                 uint32_t n_instances, const double *times,
                                                 uint32_t flags, float *out_weights);
MMDX_API void mmdx_morph_motion_destroy(mmdx_morph_motion_t motion);


/* ---- Bone tracks -> local bone poses on the device; skeleton -> bone palette ---------------------- */
/* The per-frame input side of the palette.  mmdx_bone_motion_eval replaces
 * Motion::GetBonePose (L/motion/motion_impl.inl:255-319: clamp to the first / last key, exact key hit,
 * else per-channel presampled-Bezier blend of the translation and NLerp of the rotation,
 * L/util/math_impl.inl:1260-1282, :1372-1428) together with VmdReader's control-point set-up
 * (L/reader/vmd_reader_impl.inl:31-60) and MotionPlayer's name mapping + SeekFrame
 * (L/motion/poser_impl.inl:522-548), for every (instance, bone) at once.  mmdx_skeleton_solve replaces
 * Poser::UpdateBoneTransform + UpdateBoneSkinningMatrix (L/motion/poser_impl.inl:142-166, :320-326) in
 * the reference's evaluation order (pre-physics bones, then post-physics bones, each sorted by transform
 * level then index, L/motion/poser_impl.inl:107-109, :500-510) and writes the float[16] palettes
 * mmdx_deform_batched(MMDX_PALETTE_ON_DEVICE) consumes.  Both are bit-exact against libmmd. */
typedef struct mmdx_bone_motion_s *mmdx_bone_motion_t;
typedef struct mmdx_skeleton_s *mmdx_skeleton_t;

enum { MMDX_POSES_ON_DEVICE = 1u << 4 };      /* with MMDX_OUT_ON_DEVICE (and MMDX_WEIGHTS_*) for
                                                 mmdx_skeleton_solve*                                 */
enum { MMDX_POSE_FLOATS = 8 };                /* one local pose: translation xyz, 0, quaternion xyzw  */

/* Associate the motion's bone tracks with a model's bones by name (UTF-8); bones without a track keep
 * the rest pose (zero translation, identity rotation), as after Poser::ResetPosing. */
MMDX_API mmdx_status mmdx_vmd_bind_bones(mmdx_vmd_t vmd, uint32_t n_bones,
                                         const char *const *bone_names_utf8,
                                         mmdx_bone_motion_t *out_motion);
MMDX_API mmdx_status mmdx_bone_motion_get_info(mmdx_bone_motion_t motion, uint32_t *n_bones,
                                               uint32_t *n_mapped, uint32_t *n_keys,
                                               uint32_t *n_curves);
/* The host key tables of a bound motion, as mmdx_vmd_bind_bones / mmdx_bone_motion_in_place built them and as they are uploaded on
 * first use: what each model bone received from the file (an adopter can look at what was bound; the tests compare an in-place
 * copy with its source byte for byte).  Host only.  The pointers are the handle's own arrays, read-only, valid until
 * mmdx_bone_motion_destroy.  NULL motion / out or a struct_size mismatch: MMDX_ERR_INVALID_ARGUMENT. */
typedef struct mmdx_bone_motion_keys {
    uint32_t struct_size;            /* = sizeof(mmdx_bone_motion_keys), set by the caller                                         */
    uint32_t n_bones, n_keys, n_curves;
    const uint32_t *key_off;         /* [n_bones + 1]: the keys of bone b are key_off[b] .. key_off[b + 1]                         */
    const uint32_t *key_frame;       /* [n_keys], ascending inside a bone                                                          */
    const float *key_tr;             /* [n_keys][4]: translation xyz, 0                                                            */
    const float *key_rot;            /* [n_keys][4]: quaternion xyzw                                                               */
    const uint32_t *key_curve;       /* [n_keys][4]: curve table id for x, y, z, rotation; 0xFFFFFFFF = linear                     */
    const float *lut;                /* [n_curves][32]: the presampled curves                                                      */
} mmdx_bone_motion_keys;
MMDX_API mmdx_status mmdx_bone_motion_get_keys(mmdx_bone_motion_t motion, mmdx_bone_motion_keys *out);
/* out_poses[i][b][MMDX_POSE_FLOATS] = local pose of model bone b at frames[i].  Stream and device as
 * for mmdx_morph_motion_eval.  flags: MMDX_FRAMES_ON_DEVICE | MMDX_OUT_ON_DEVICE. */
MMDX_API mmdx_status mmdx_bone_motion_eval(mmdx_bone_motion_t motion, mmdx_model_t model,
                                           uint32_t n_instances, const uint32_t *frames,
                                           uint32_t flags, float *out_poses);
/* out_poses[i][b][MMDX_POSE_FLOATS] = local pose of model bone b at times[i] seconds (Motion::GetBonePose(name,
 * double time), L/motion/motion_impl.inl:321-380; points 1-6 at mmdx_morph_motion_eval_time).  flags:
 * MMDX_TIMES_ON_DEVICE | MMDX_OUT_ON_DEVICE. */
MMDX_API mmdx_status mmdx_bone_motion_eval_time(mmdx_bone_motion_t motion, mmdx_model_t model,
                                                uint32_t n_instances, const double *times,
                                                uint32_t flags, float *out_poses);
MMDX_API void mmdx_bone_motion_destroy(mmdx_bone_motion_t motion);

enum {                                        /* bits of the PMX bone flag word the skeleton reads    */
    MMDX_BONE_HAS_IK = 0x0020, MMDX_BONE_APPEND_ROTATE = 0x0100, MMDX_BONE_APPEND_TRANSLATE = 0x0200,
    MMDX_BONE_POST_PHYSICS = 0x1000
};

typedef struct mmdx_skeleton_desc {           /* e.g. straight from mmdx_pmx_get_arrays               */
    uint32_t struct_size;
    uint32_t n_bones;
    const float *rest_position;               /* [n_bones][3]                                         */
    const int32_t *parent;                    /* [n_bones]; outside [0, n_bones) = none               */
    const int32_t *transform_level;           /* [n_bones] or NULL (all 0); compared as unsigned, like
                                                 the reference's size_t cast                          */
    const uint16_t *flags;                    /* [n_bones] PMX bone flag word, or NULL (all 0)        */
    /* append (inherit) bones -- read where flags has MMDX_BONE_APPEND_*; NULL if no bone has them     */
    const int32_t *append_parent;             /* [n_bones]; outside [0, n_bones) = the bone does not
                                                 append (L/motion/poser_impl.inl:50-56)               */
    const float *append_ratio;                /* [n_bones]                                            */
    /* CCD-IK -- read where flags has MMDX_BONE_HAS_IK; NULL if no bone has it                         */
    const int32_t *ik_target;                 /* [n_bones]                                            */
    const int32_t *ik_loop_count;             /* [n_bones]; negative or > 256 means 256 (:94)         */
    const float *ik_angle_limit;              /* [n_bones] radians per link step                      */
    const uint32_t *ik_link_offset;           /* [n_bones+1] into the link arrays                     */
    const int32_t *ik_link_bone;              /* [L] target-side link first                           */
    const uint8_t *ik_link_limited;           /* [L]                                                  */
    const float *ik_link_lo, *ik_link_hi;     /* [L][3] Euler limits (either order; min/max is taken) */
    /* bone morphs (Poser::UpdateMorphTransform, MORPH_TYPE_BONE, L/motion/poser_impl.inl:347-354) -- the
     * model's morph table as in mmdx_model_desc; only group (0) and bone (2) morphs are read.  n_morphs
     * == 0 / NULL: no bone morphs (morph_rotation_ = identity, morph_translation_ = 0).                */
    uint32_t n_morphs;
    uint32_t create_flags;                    /* MMDX_SKELETON_*                                      */
    const int32_t *morph_type;                /* [n_morphs] PMX morph type                            */
    const uint32_t *morph_offset;             /* [n_morphs+1]                                         */
    const uint32_t *morph_index;              /* [E] group: morph index; bone: bone index             */
    const float *morph_value;                 /* [E][3] group: rate in [0]; bone: translation         */
    const float *morph_rotation;              /* [E][4] bone: rotation xyzw; NULL = identity          */
} mmdx_skeleton_desc;

enum {
    MMDX_SKELETON_PHYSICS_SEAM = 1u << 0      /* the skeleton will be solved in two steps with a physics reactor's
                                                 writes in between (mmdx_skeleton_solve_pre / _post): compiles the
                                                 ordered solver, which keeps per-bone state between the steps, for
                                                 rigs without IK / append bones too                              */
};

typedef struct mmdx_skeleton_info {
    uint32_t struct_size;
    uint32_t n_bones, n_pre_physics, n_post_physics;
    uint32_t max_chain;                       /* longest parent chain (parallel solver), else 0       */
    uint32_t solver;                          /* MMDX_SOLVER_*                                        */
    uint32_t n_ik_bones, n_ik_links, n_append_bones;
    uint32_t n_bone_morph_entries;            /* applications of a bone-morph entry (groups expanded)  */
    uint32_t n_solve_rounds;                  /* ordered solver: rounds the evaluation sequence was cut
                                                 into (independent bones share a round), else 0         */
    uint32_t n_ik_rounds_16_lanes;            /* ... of which rounds made of CCD-IK solves on plain chains: these
                                                 run with sixteen lanes per solve (ABI 3)                */
} mmdx_skeleton_info;

enum {
    MMDX_SOLVER_PARALLEL_FK = 0,  /* no IK / append: one thread per (instance, bone), bit-exact      */
    MMDX_SOLVER_SERIAL = 1        /* IK / append present: the reference's evaluation sequence; bones
                                     (and IK solves) that touch disjoint state run side by side, the
                                     rest in order; sin/cos/asin/acos/atan2 through the device's double
                                     libm like the reference's through the host's     */
};

/* Index validation happens here (MMDX_ERR_BAD_INDEX), so solve cannot read out of range.
 * Nested IK -- a link or target that is itself an IK bone -- is solved the way the reference's recursion does
 * (UpdateBoneTransform re-enters itself for links and target, L/motion/poser_impl.inl:196-206), up to 3 solves
 * deep.  MMDX_ERR_UNSUPPORTED: deeper nesting, or an IK bone that is (indirectly) part of its own solve (endless
 * recursion in the reference). */
MMDX_API mmdx_status mmdx_skeleton_create(const mmdx_skeleton_desc *desc, mmdx_skeleton_t *out_skeleton);
MMDX_API mmdx_status mmdx_skeleton_get_info(mmdx_skeleton_t skeleton, mmdx_skeleton_info *info);
/* out_palettes[i][b][16] from poses[i][b][MMDX_POSE_FLOATS].  flags: MMDX_POSES_ON_DEVICE |
 * MMDX_OUT_ON_DEVICE.  Runs on `model`'s stream when given, so the deform call that follows sees it. */
MMDX_API mmdx_status mmdx_skeleton_solve(mmdx_skeleton_t skeleton, mmdx_model_t model,
                                         uint32_t n_instances, const float *poses, uint32_t flags,
                                         float *out_palettes);
/* Bone tracks -> palettes in one call: out_palettes[i][b][16] at frames[i] -- bit for bit what mmdx_bone_motion_eval followed by
 * mmdx_skeleton_solve computes (MotionPlayer::SeekFrame + Pre/PostPhysicsPosing for every instance, main.cpp:1793-1810).  On a
 * skeleton that runs the parallel FK solver it is ONE launch and the [NI][NB][8] local poses never leave the chip (a workgroup per
 * instance keeps them in LDS); skeletons with append bones / IK and those of more than 2 048 bones take the two launches, the poses
 * in the motion's scratch buffer.  `motion` must have been bound to this skeleton's bones.  flags: MMDX_FRAMES_ON_DEVICE |
 * MMDX_OUT_ON_DEVICE; stream and device as for mmdx_bone_motion_eval; recordable into a graph. */
MMDX_API mmdx_status mmdx_skeleton_solve_motion(mmdx_skeleton_t skeleton, mmdx_bone_motion_t motion, mmdx_model_t model,
                                                uint32_t n_instances, const uint32_t *frames, uint32_t flags,
                                                float *out_palettes);
/* The same at times[i] seconds: bit for bit mmdx_bone_motion_eval_time followed by mmdx_skeleton_solve (MotionPlayer::SeekTime,
 * L/motion/poser_impl.inl:548-555; points 1-6 at mmdx_morph_motion_eval_time).  One launch on parallel-FK skeletons of up to
 * 2 048 bones, else the two launches.  flags: MMDX_TIMES_ON_DEVICE | MMDX_OUT_ON_DEVICE; recordable into a graph. */
MMDX_API mmdx_status mmdx_skeleton_solve_motion_time(mmdx_skeleton_t skeleton, mmdx_bone_motion_t motion, mmdx_model_t model,
                                                     uint32_t n_instances, const double *times, uint32_t flags,
                                                     float *out_palettes);

/* ---- Motion sets: every instance of a crowd plays its own clip ------------------------------------------------------------------
 * In the reference every Poser has its own MotionPlayer over whichever Motion it likes (L/motion/poser_impl.inl:522-555), so instance
 * i playing clip c[i] at t[i] is plain reference behaviour.  A motion set is an immutable bank of clips bound to ONE model's bones
 * and / or morphs; the entry points below take a clip index per instance next to the per-instance frame or time, and the result for
 * instance i is, bit for bit, what the single-motion entry point (mmdx_bone_motion_eval*, mmdx_morph_motion_eval*,
 * mmdx_skeleton_solve_motion*) returns for clip clips[i] at frames[i] / times[i] -- Motion::GetBonePose / GetMorphPose
 * (L/motion/motion_impl.inl:255-380, :382-465) of that instance's Motion.  One launch whatever the mix of clips, nothing for the
 * host to partition or gather.
 *
 * mmdx_motion_set_create COPIES the host tables of the given motions: the motions and their mmdx_vmd_t may be destroyed afterwards.
 * At least one of the two arrays must be given; all bone motions must be bound to the same number of bones and all morph motions to
 * the same number of morphs (MMDX_ERR_INVALID_ARGUMENT otherwise, as for n_clips == 0, a NULL element, or keys that in total do not
 * fit 32-bit offsets).  An entry point of the side the set was created without returns MMDX_ERR_INVALID_ARGUMENT.
 *
 * clips[n_instances]: MMDX_CLIP_NONE = this instance plays nothing -- its row is still written: poses {0,0,0,0, 0,0,0,1} per bone
 * (Poser::ResetPosing), rates 0, the palette the solve of the rest pose.  A HOST clip index >= n_clips that is not MMDX_CLIP_NONE
 * returns MMDX_ERR_BAD_INDEX; a DEVICE clip index >= n_clips behaves as MMDX_CLIP_NONE.  No row of the output is left unwritten
 * and nothing is read out of range.
 *
 * flags: MMDX_FRAMES_ON_DEVICE (= MMDX_TIMES_ON_DEVICE) | MMDX_OUT_ON_DEVICE; unknown bits are rejected.  MMDX_FRAMES_ON_DEVICE
 * means BOTH clips and frames / times are device pointers; without it both are host pointers, copied through a scratch of the set
 * in stream order.  The *_time forms follow points 1-6 at mmdx_morph_motion_eval_time (host NaN rejected, device NaN takes the
 * first key).  Stream, device, first-use upload and graph recording as for mmdx_bone_motion_eval / mmdx_skeleton_solve_motion: run
 * the call once before recording it; a set destroyed while a graph holds it invalidates the graph. */
typedef struct mmdx_motion_set_s *mmdx_motion_set_t;
enum { MMDX_CLIP_NONE = 0xFFFFFFFFu };        /* this instance plays nothing: rest pose, all rates 0  */

typedef struct mmdx_motion_set_info {
    uint32_t struct_size;
    uint32_t n_clips, n_bones, n_morphs;      /* n_bones / n_morphs 0 when that side was not given    */
    uint32_t n_bone_keys, n_morph_keys;       /* sums over the clips                                  */
    uint32_t n_curves;                        /* presampled curve tables; byte-identical ones of
                                                 different clips are stored once                      */
} mmdx_motion_set_info;

MMDX_API mmdx_status mmdx_motion_set_create(uint32_t n_clips, const mmdx_bone_motion_t *bone_motions /* [n_clips] or NULL */,
                                            const mmdx_morph_motion_t *morph_motions /* [n_clips] or NULL */,
                                            mmdx_motion_set_t *out_set);
MMDX_API mmdx_status mmdx_motion_set_get_info(mmdx_motion_set_t set, mmdx_motion_set_info *info);
MMDX_API void mmdx_motion_set_destroy(mmdx_motion_set_t set);
/* out_poses[i][b][MMDX_POSE_FLOATS] = local pose of model bone b in clip clips[i] at frames[i] / times[i] seconds. */
MMDX_API mmdx_status mmdx_motion_set_eval_bones(mmdx_motion_set_t set, mmdx_model_t model, uint32_t n_instances,
                                                const uint32_t *clips, const uint32_t *frames, uint32_t flags, float *out_poses);
MMDX_API mmdx_status mmdx_motion_set_eval_bones_time(mmdx_motion_set_t set, mmdx_model_t model, uint32_t n_instances,
                                                     const uint32_t *clips, const double *times, uint32_t flags, float *out_poses);
/* out_weights[i][m] = rate of model morph m in clip clips[i] at frames[i] / times[i] seconds. */
MMDX_API mmdx_status mmdx_motion_set_eval_morphs(mmdx_motion_set_t set, mmdx_model_t model, uint32_t n_instances,
                                                 const uint32_t *clips, const uint32_t *frames, uint32_t flags, float *out_weights);
MMDX_API mmdx_status mmdx_motion_set_eval_morphs_time(mmdx_motion_set_t set, mmdx_model_t model, uint32_t n_instances,
                                                      const uint32_t *clips, const double *times, uint32_t flags, float *out_weights);
/* out_palettes[i][b][16]: bit for bit mmdx_motion_set_eval_bones* followed by mmdx_skeleton_solve.  One launch on parallel-FK
 * skeletons of up to 2 048 bones (a workgroup per instance, its clip id and clock read once, the poses in LDS); skeletons with
 * append bones / IK and larger ones take the two launches, the poses in the set's scratch buffer.  The set's bone motions must have
 * been bound to this skeleton's bones (MMDX_ERR_INVALID_ARGUMENT on another bone count). */
MMDX_API mmdx_status mmdx_skeleton_solve_motion_set(mmdx_skeleton_t skeleton, mmdx_motion_set_t set, mmdx_model_t model,
                                                    uint32_t n_instances, const uint32_t *clips, const uint32_t *frames,
                                                    uint32_t flags, float *out_palettes);
MMDX_API mmdx_status mmdx_skeleton_solve_motion_set_time(mmdx_skeleton_t skeleton, mmdx_motion_set_t set, mmdx_model_t model,
                                                         uint32_t n_instances, const uint32_t *clips, const double *times,
                                                         uint32_t flags, float *out_palettes);

/* ---- Cross-fade between two clips of a motion set, per instance ----------------------------------------------------------------
 * Rewriting clips[i] makes instance i jump from one clip to the other.  The reference has no cross-fade, but it has the operations
 * one is made of, and uses them between two keys of one track: l*(1-lambda) + r*lambda per channel for translations and morph
 * weights (L/motion/motion_impl.inl:364-372, :462) and NLerp(l, r)[lambda] for rotations (L/util/math_impl.inl:1260-1282).  The
 * blend is exactly those operations applied between two clips, so it is held to the same bar: bit for bit against code that runs
 * the real libmmd.
 *
 * For instance i, a = clips_a[i], b = clips_b[i], w = weights[i]: A is the row the mmdx_motion_set_eval_*_time call writes for
 * (a, times_a[i]) -- the rest pose / rate 0 for MMDX_CLIP_NONE or a device id >= n_clips -- and B the same for (b, times_b[i]).
 *   !(w >= 1e-7f)      the row is A, every bit (w < 1e-7f, negative, a device NaN); clip b is not evaluated, no table of it read
 *   w > 1.0f - 1e-7f   the row is B, every bit; clip a is not evaluated
 *   otherwise          translation  A.t.c * (1.0f - w) + B.t.c * w  for c = x, y, z (float, unfused, this order), fourth float 0
 *                      rotation     the middle branch of NLerpProxy::operator[]: dot = A.q . B.q (4 terms, left to right);
 *                                   (1-w)*A.q - w*B.q when dot < 0, else (1-w)*A.q + w*B.q; Normalize = * 1.0f / float(sqrt(double(
 *                                   sum of squares)))
 *                      morph rate   A.r * (1.0f - w) + B.r * w
 * The short circuits are NLerp's, applied to the whole row: a crowd in which few instances are mid-transition pays one evaluation
 * for the rest.  The palette call is bit for bit the blended poses followed by mmdx_skeleton_solve.
 *
 * Host operands are checked before the first HIP call: a clip id >= n_clips other than MMDX_CLIP_NONE in either array returns
 * MMDX_ERR_BAD_INDEX, a NaN time or weight MMDX_ERR_INVALID_ARGUMENT.  Device operands follow the rules above (a NaN time takes
 * the first key).  flags: MMDX_TIMES_ON_DEVICE | MMDX_OUT_ON_DEVICE, unknown bits rejected; MMDX_TIMES_ON_DEVICE makes ALL FIVE
 * operand arrays device pointers.  Only the time clock is offered; more than two clips and per-bone weights are mmdx_pose_blend's (below); advancing and wrapping
 * the clocks, the fade weight and the hand-over at the end of a fade are mmdx_animator_advance's (below).  Stream, device,
 * first-use upload, graph recording and pinning as for mmdx_skeleton_solve_motion_set_time: run the call once before recording it. */
typedef struct mmdx_motion_blend_args {
    uint32_t struct_size, n_instances;    /* = sizeof(mmdx_motion_blend_args); NI >= 1            */
    const uint32_t *clips_a, *clips_b;    /* [n_instances]                                        */
    const double *times_a, *times_b;      /* [n_instances] seconds                                */
    const float *weights;                 /* [n_instances] 0 = a, 1 = b                           */
    uint32_t flags;                       /* MMDX_TIMES_ON_DEVICE | MMDX_OUT_ON_DEVICE            */
} mmdx_motion_blend_args;

MMDX_API mmdx_status mmdx_motion_set_blend_bones_time(mmdx_motion_set_t set, mmdx_model_t model, const mmdx_motion_blend_args *args,
                                                      float *out_poses /* [NI][NB][MMDX_POSE_FLOATS] */);
MMDX_API mmdx_status mmdx_motion_set_blend_morphs_time(mmdx_motion_set_t set, mmdx_model_t model, const mmdx_motion_blend_args *args,
                                                       float *out_weights /* [NI][NM] */);
/* One launch on parallel-FK skeletons of up to 2 048 bones (both clip ids, both clocks and the weight read once per workgroup, the
 * blend in registers, the poses in LDS); skeletons with append bones / IK and larger ones take the blend into the set's pose
 * scratch, then mmdx_skeleton_solve. */
MMDX_API mmdx_status mmdx_skeleton_solve_motion_set_blend_time(mmdx_skeleton_t skeleton, mmdx_motion_set_t set, mmdx_model_t model,
                                                               const mmdx_motion_blend_args *args,
                                                               float *out_palettes /* [NI][NB][16] */);

/* ---- Crowd animator: clocks, loops and cross-fades advanced on the device -----------------------------------------------------
 * The reference's whole clock is g_state.time += dt for one MotionPlayer (main.cpp:1757) plus Motion::GetLength(); a crowd has one
 * such clock per Poser.  An animator keeps a playback state per instance in device memory and advances all of them with one
 * launch from a single dt.  Its arrays ARE the five operand arrays of the blend calls above (mmdx_animator_operands), so a recorded
 * frame is: rewrite 8 bytes (dt), launch.
 *
 * Clip lengths.  mmdx_motion_set_clip_frames returns, per clip, the largest key frame over the clip's bone and morph tracks,
 * whichever sides the set has: Motion::GetLength() (L/motion/motion_impl.inl:223-244) of a motion holding those tracks, 0 for a clip
 * without keys.  Host only, computed at mmdx_motion_set_create.  A clip's length in seconds is double(last_frame) / 30.0.
 *
 * The state, eleven arrays of [n_instances] in device memory (mmdx_animator_arrays):
 *   clips_a, clips_b  u32  the clip playing and the clip being faded to            initially MMDX_CLIP_NONE both
 *   times_a, times_b  f64  their clocks, seconds                                   0
 *   weights           f32  blend weight, 0 = a, 1 = b                              0
 *   speed             f32  playback rate, may be negative                          1
 *   fade_rate         f32  weight per second, 0 = not fading                       0
 *   req_clip          u32  pending request, MMDX_ANIM_NO_REQUEST = none; MMDX_CLIP_NONE is a valid request (fade out to rest)
 *   req_fade          f32  the request's fade, seconds                             0
 *   req_time          f64  start time of the requested clip                        0
 *   loops             u32  steps in which clock a wrapped                          0
 * and a per-clip table [n_clips] from mmdx_animator_desc.clips: length (seconds; <= 0 or NaN = the clip's own length, see above),
 * mode MMDX_ANIM_LOOP / _HOLD / _THEN, and for _THEN the clip that follows (`next`, a clip id or MMDX_CLIP_NONE) and the fade into
 * it (`fade`, seconds).  clips == NULL: every clip loops over its own length.
 *
 * mmdx_animator_advance.  The arithmetic is part of the contract: IEEE operations only, no libm, unfused (-ffp-contract=off), so
 * a host restatement agrees bit for bit.  A NaN dt changes nothing.  Otherwise, for every instance, in this order
 * (L(c), mode(c), next(c), fade(c) = the table row of clip c):
 *   1. s = double(speed) * dt
 *   2. times_a = wrap(clips_a, times_a + s); loops += 1 if that wrap folded the clock
 *   3. only if fade_rate > 0:
 *        times_b = wrap(clips_b, times_b + s)                       (never counted in loops)
 *        weights = weights + float(dt) * fade_rate                  (float; the product and the sum are two roundings)
 *        if !(weights >= 0): weights = 0
 *        if weights > 1.0f - 1e-7f (the blend's "the row is B" threshold): PROMOTE -- clips_a = clips_b, times_a = times_b,
 *            clips_b = MMDX_CLIP_NONE, times_b = 0, weights = 0, fade_rate = 0
 *   4. only if fade_rate == 0 now, pick a transition (c, fade, t0):
 *        req_clip != MMDX_ANIM_NO_REQUEST                           -> (req_clip, req_fade, req_time)
 *        else clips_a < n_clips, mode(clips_a) == MMDX_ANIM_THEN and times_a >= L(clips_a) - double(fade(clips_a))
 *                                                                   -> (next(clips_a), fade(clips_a), 0.0)
 *        and if there is one: !(fade > 0): clips_a = c, times_a = t0 (a switch at once);
 *                             otherwise clips_b = c, times_b = t0, weights = 0, fade_rate = 1.0f / fade;
 *                             then req_clip = MMDX_ANIM_NO_REQUEST.
 *      So a request that arrives during a fade waits until that fade is promoted and starts in the same step as the promotion.
 *   clamp(t, L) = t > L ? L : (t >= 0 ? t : 0)                      (a NaN clock becomes 0)
 *   wrap(c, t):  c >= n_clips (MMDX_CLIP_NONE, an id out of range): t, the rest pose has no length
 *                mode(c) is not MMDX_ANIM_LOOP: clamp(t, L(c))
 *                MMDX_ANIM_LOOP, !(L > 0): 0
 *                MMDX_ANIM_LOOP, L > 0: if t < 0 or t >= L: t = clamp(t - floor(t / L) * L, L) -- a division, a floor, a multiply
 *                and a subtraction -- and the clock has folded, once per step however many lengths the step spans; else t.
 *   The evaluators clamp outside [first key, last key], so a clock that lands exactly on L shows the last key for one step.
 * The call always advances ALL instances: a culled character's clock keeps running, only its solve and deform are skipped by the
 * select calls.  One lane per instance, on `model`'s stream, in order with the solve that follows.
 * dt: a host double, passed to the kernel BY VALUE -- a recorded graph freezes that value, every replay takes the same step.  With
 * MMDX_ANIM_DT_ON_DEVICE dt is a device pointer (8-byte aligned) read when the kernel RUNS: a replay is "rewrite 8 bytes, launch".
 * A host NaN dt is MMDX_ERR_INVALID_ARGUMENT; a device NaN dt leaves every array unchanged.
 *
 * Every call of the family takes a `model` for the device, the stream and the graph recording, like the motion-set calls (NULL: the
 * selected device's default stream).  The state is allocated and initialised on the device of the first call that needs it
 * (mmdx_animator_operands and _device_arrays: the calling thread's selected device) and stays there: a model of another device is
 * MMDX_ERR_INVALID_ARGUMENT.  Creating, destroying and mmdx_animator_get_info need no device.  Graph rules are the motion set's: run
 * a call once before recording it; host lists, mmdx_animator_set_state and _get_state are refused while recording; the handle is
 * pinned while a graph holds its addresses and destroying it invalidates the graph. */
#define MMDX_ANIM_NO_REQUEST 0xFFFFFFFEu
enum { MMDX_ANIM_LOOP = 0, MMDX_ANIM_HOLD = 1, MMDX_ANIM_THEN = 2 };   /* mmdx_animator_clip.mode                                */
enum { MMDX_ANIM_DT_ON_DEVICE = 1u << 10 };                             /* mmdx_animator_advance: dt is a device pointer          */

typedef struct mmdx_animator_s *mmdx_animator_t;

typedef struct mmdx_animator_clip {
    double length;             /* seconds; <= 0 or NaN: the clip's own length, double(last_frame) / 30.0                          */
    uint32_t mode;             /* MMDX_ANIM_LOOP / _HOLD / _THEN; anything else: MMDX_ERR_INVALID_ARGUMENT                        */
    uint32_t next;             /* _THEN: the clip that follows, < n_clips or MMDX_CLIP_NONE (else MMDX_ERR_BAD_INDEX)             */
    float fade;                /* _THEN: seconds of cross-fade into `next`; <= 0: switch at once; NaN: MMDX_ERR_INVALID_ARGUMENT  */
    uint32_t reserved0;        /* 0                                                                                               */
} mmdx_animator_clip;

typedef struct mmdx_animator_desc {
    uint32_t struct_size;      /* = sizeof(mmdx_animator_desc)                                                                    */
    uint32_t n_instances;      /* NI >= 1, fixed for the life of the handle                                                       */
    const mmdx_animator_clip *clips; /* [n_clips] host, or NULL: every clip loops over its own length                             */
    uint32_t n_clips;          /* with clips: must equal the set's clip count; ignored when clips == NULL                         */
    uint32_t reserved0;        /* 0                                                                                               */
} mmdx_animator_desc;

typedef struct mmdx_animator_info {
    uint32_t struct_size;
    uint32_t n_instances, n_clips;
    int32_t device_ordinal;    /* where the state lives, -1 = not allocated yet                                                   */
} mmdx_animator_info;

/* The eleven arrays: device addresses from mmdx_animator_device_arrays, host arrays for mmdx_animator_set_state / _get_state.   */
typedef struct mmdx_animator_arrays {
    uint32_t struct_size, n_instances;
    uint32_t *clips_a, *clips_b;
    double *times_a, *times_b;
    float *weights, *speed, *fade_rate;
    uint32_t *req_clip;
    float *req_fade;
    double *req_time;
    uint32_t *loops;
} mmdx_animator_arrays;

MMDX_API mmdx_status mmdx_motion_set_clip_frames(mmdx_motion_set_t set, uint32_t *last_frames /* [n_clips] */);
/* The animator copies what it needs of the set (clip count and lengths): the set may be destroyed afterwards. */
MMDX_API mmdx_status mmdx_animator_create(mmdx_motion_set_t set, const mmdx_animator_desc *desc, mmdx_animator_t *out_animator);
MMDX_API void mmdx_animator_destroy(mmdx_animator_t animator);
/* clips (may be NULL) receives the table as resolved: the lengths in seconds that advance uses. */
MMDX_API mmdx_status mmdx_animator_get_info(mmdx_animator_t animator, mmdx_animator_info *info, mmdx_animator_clip *clips /* [n_clips] */);
/* Fills *out with clips_a, clips_b, times_a, times_b, weights of the state, n_instances and MMDX_TIMES_ON_DEVICE |
 * MMDX_OUT_ON_DEVICE: the three blend calls take the animator's state with no glue. */
MMDX_API mmdx_status mmdx_animator_operands(mmdx_animator_t animator, mmdx_motion_blend_args *out);
/* Every device address of the state (out->struct_size set by the caller): an adopter's own behaviour kernel can write requests or
 * speeds and read `loops` (root motion, events), in stream order with the calls here. */
MMDX_API mmdx_status mmdx_animator_device_arrays(mmdx_animator_t animator, mmdx_animator_arrays *out);
/* Copy any subset of the arrays from / to host arrays (a NULL member = leave that array alone; n_instances must be the handle's),
 * in `model`'s stream order; both return when the copies are done.  set_state checks the host values before the first HIP call:
 * a clip id >= n_clips other than MMDX_CLIP_NONE in clips_a / clips_b / req_clip (where MMDX_ANIM_NO_REQUEST is valid too) is
 * MMDX_ERR_BAD_INDEX, a NaN in any time, weight, speed, fade_rate or req_fade MMDX_ERR_INVALID_ARGUMENT. */
MMDX_API mmdx_status mmdx_animator_set_state(mmdx_animator_t animator, mmdx_model_t model, const mmdx_animator_arrays *state);
MMDX_API mmdx_status mmdx_animator_get_state(mmdx_animator_t animator, mmdx_model_t model, const mmdx_animator_arrays *state);
/* Scatter n requests: instance ids[j] gets (req_clip, req_fade, req_time) = (clips[j], fades[j], start_times[j]); fades == NULL
 * means 0 (switch at once), start_times == NULL means 0.  The ids of one call must be distinct (otherwise which request an
 * instance keeps is unspecified; a host list longer than n_instances is MMDX_ERR_INVALID_ARGUMENT).  A later request replaces one that has not started yet.  flags: MMDX_TIMES_ON_DEVICE = all lists are
 * device pointers, read when the kernel runs (recordable); an id >= n_instances is then skipped on the device and clip ids are
 * used as they are (an id out of range plays the rest pose).  Host lists are checked before the first HIP call -- an id >=
 * n_instances or a clip id >= n_clips other than MMDX_CLIP_NONE: MMDX_ERR_BAD_INDEX; a NaN fade or start time:
 * MMDX_ERR_INVALID_ARGUMENT -- then copied through a scratch of the handle in stream order, and the call returns when they have
 * been consumed.  n == 0 is MMDX_OK and does nothing. */
MMDX_API mmdx_status mmdx_animator_request(mmdx_animator_t animator, mmdx_model_t model, uint32_t n, const uint32_t *ids,
                                           const uint32_t *clips, const float *fades, const double *start_times, uint32_t flags);
/* flags: MMDX_ANIM_DT_ON_DEVICE or 0; unknown bits are rejected. */
MMDX_API mmdx_status mmdx_animator_advance(mmdx_animator_t animator, mmdx_model_t model, const double *dt, uint32_t flags);

/* ---- Root motion: the animator walks its crowd through the world -----------------------------------------------------------------
 * mmdx_animator_root_motion adds, to every instance's placement (the pose form of mmdx_palette_place, in device memory), the
 * displacement the playing clips give a root bone during the step that mmdx_animator_advance is ABOUT to take: call it BEFORE
 * advance, with the same dt, on the state advance is about to step.  It reads the animator's arrays and writes only
 * placements[i][0..2]; the fourth float, the quaternion and every animator array keep their bytes.
 *
 * `set` is any bone-sided set with the animator's clip count (another count: MMDX_ERR_INVALID_ARGUMENT); it need not be the set the
 * poses come from.  The intended cheap form: bind every VMD to the single name of the root bone (mmdx_vmd_bind_bones with one
 * name) -- a one-bone bank, root_bone = 0 -- so the call reads a few keys per instance whatever the model's bone count.
 *
 * The arithmetic is part of the contract, like advance's: IEEE operations only, unfused.  R(c, t) is the translation in the row
 * that mmdx_motion_set_eval_bones_time writes for (clip c, time t, bone root_bone), {0,0,0} when c >= n_clips.  A NaN dt writes
 * nothing.  Otherwise, for every instance i, with the state as it stands before advance:
 *   1. s = double(speed) * dt                                      (step 1 of advance)
 *   2. the displacement of a side (c, t0):  raw = t0 + s;  t1 = wrap(c, raw)   (advance's wrap, above)
 *        the wrap did not fold (a HOLD / THEN clamp included):  D = R(c,t1) - R(c,t0)
 *        it folded:                                             D = (R(c,near) - R(c,t0)) + (R(c,t1) - R(c,far))
 *            with near = L(c), far = 0.0 when raw >= L(c); near = 0.0, far = L(c) otherwise (a negative step).  Further whole
 *            laps inside one step are not counted, just as `loops` counts one.
 *        Each - and + is libmmd's Vector3D operator: per component, binary32, in the order written.
 *   3. D_a = the displacement of (clips_a, times_a); D_b = that of (clips_b, times_b) when fade_rate > 0, else {+0,+0,+0}
 *   4. blend with the weight before the step, w = weights[i], by the cross-fade's rules (mmdx_motion_blend_args):
 *        !(w >= 1e-7f): D = D_a, and side b is neither evaluated nor read;  w > 1.0f - 1e-7f: D = D_b, side a is not evaluated;
 *        otherwise D.c = D_a.c * (1.0f - w) + D_b.c * w per component
 *   5. a component whose bit is absent from `axes` becomes +0.0f (a select, not a multiply)
 *   6. M = ToRotateMatrix of placements[i][4..7] as in mmdx_palette_place (the quaternion is not normalised);
 *      d = rotate(D, M) (L/util/math_impl.inl:1032-1038): d.c = D.x*M[0][c] + D.y*M[1][c] + D.z*M[2][c], left to right;
 *      placements[i][c] = placements[i][c] + d.c
 * There are no other short circuits: NaN and infinity propagate as IEEE gives them (a NaN's sign and payload are outside the
 * contract, as in mmdx_palette_place).  Clip changes advance makes in its step 4 (a request, a THEN successor, a switch at once)
 * contribute nothing: the new clip starts at its t0.  This call reads the root's translation only and leaves the heading alone;
 * mmdx_animator_root_motion_turn, below, also applies the root's rotation deltas.  (No matrix-form placements, no
 * select form: a culled character keeps walking, as its clock keeps running.)
 *
 * NULL animator / set / args / dt / placements, a struct_size mismatch, unknown flag or axes bits, a misaligned device dt (8) or
 * placements (4), a set without a bone side and a host NaN dt are MMDX_ERR_INVALID_ARGUMENT; root_bone >= the set's bone count is
 * MMDX_ERR_BAD_INDEX.  Device, stream and graph rules are advance's: asynchronous on `model`'s stream, a model of another device
 * than the animator's is refused, recordable after one unrecorded run (a host dt is frozen into the recording), and both the
 * animator and the set are pinned by a graph that holds them.
 *
 * mmdx_bone_motion_in_place (host only) is the other half: a copy of `src` in which the translation of every key of `bone` is
 * +0.0f on the axes named, everything else byte for byte the same.  The zeroed channels evaluate to zero at every time (the lerp
 * of two zeros), so a set made of such motions gives the poses whose motion has been taken out, through every existing call --
 * the one-launch blend solve included -- at no per-frame cost; the whole-model shift is what the placement then carries.  This is
 * a faithful split only when every moved bone descends from `bone` (the adopter's choice of root, such as PMX's "mother" bone); the call does
 * not check it.  NULL src / out and unknown axes bits: MMDX_ERR_INVALID_ARGUMENT; bone >= the motion's bone count: MMDX_ERR_BAD_INDEX. */
enum { MMDX_ROOT_X = 1u, MMDX_ROOT_Y = 2u, MMDX_ROOT_Z = 4u };
typedef struct mmdx_root_motion_args {
    uint32_t struct_size, flags;   /* = sizeof(mmdx_root_motion_args); flags: MMDX_ANIM_DT_ON_DEVICE or 0, other bits rejected      */
    uint32_t root_bone;            /* a bone of `set` (< its n_bones)                                                              */
    uint32_t axes;                 /* MMDX_ROOT_X | _Y | _Z; bits outside rejected; 0 allowed (nothing moves)                      */
    const double *dt;              /* as mmdx_animator_advance: a host value, or a device double with the flag                     */
    float *placements;             /* DEVICE, [NI][MMDX_POSE_FLOATS], the pose form of mmdx_palette_place; 4-byte aligned          */
} mmdx_root_motion_args;
MMDX_API mmdx_status mmdx_animator_root_motion(mmdx_animator_t animator, mmdx_motion_set_t set, mmdx_model_t model,
                                               const mmdx_root_motion_args *args);
MMDX_API mmdx_status mmdx_bone_motion_in_place(mmdx_bone_motion_t src, uint32_t bone, uint32_t axes, mmdx_bone_motion_t *out_motion);

/* ---- Root motion that turns: rotation deltas move each placement's heading ---------------------------------------------------------
 * mmdx_animator_root_motion_turn is mmdx_animator_root_motion for clips whose root also rotates (a walk along a curve, a turn on the
 * spot): the placement follows the root as a rigid frame.  If every moved bone descends from the root, the original motion is
 * S_inplace * W_root(t) * W_0 with W_root the root's "world bone" matrix, so the placement must become
 * W_p(t1) = W_root(t1) * W_root(t0)^-1 * W_p(t0); in quaternions and row vectors that is the arithmetic below (libmmd's product
 * satisfies M(a * b) = M(b) * M(a)).  The call order (BEFORE advance, same dt), the validation, the device / stream / graph rules and
 * the pinning are the plain call's, word for word.  It writes placements[i][0..2] and placements[i][4..7]; placements[i][3] and
 * every animator array keep their bytes.  A NaN dt writes nothing.
 *
 * The arithmetic is part of the contract: IEEE binary32 in the order written, unfused.  (T, Q)(c, t) is the translation and the
 * rotation {x, y, z, w} of the row mmdx_motion_set_eval_bones_time writes for (clip c, time t, bone root_bone); {0,0,0} and
 * {0,0,0,1} when c >= n_clips.  s, raw, t1, near and far are steps 1-2 of the plain call.  `*` between quaternions is
 * Quaternion::operator* (L/util/math_impl.inl:510-517), Inverse is :474-477, M(q) is q.ToRotateMatrix() (:540-563, not normalised),
 * rotate(v, M) is :1032-1038 (three-term sums left to right), - and + on vectors are per component.
 *   a side (c, t0), no fold:   qi = Q(t0).Inverse();  dq = qi * Q(t1);  D = rotate(T(t1) - T(t0), M(qi))
 *   a side (c, t0), folded:    qi = Q(t0).Inverse();   dq1 = qi * Q(near);  d1 = rotate(T(near) - T(t0), M(qi))
 *                              qf = Q(far).Inverse();  dq2 = qf * Q(t1);    d2 = rotate(T(t1) - T(far), M(qf))
 *                              D = d1 + rotate(d2, M(dq1));  dq = dq1 * dq2
 *   sides                      (D_a, dq_a) from (clips_a, times_a); (D_b, dq_b) from (clips_b, times_b) when fade_rate > 0, else
 *                              {+0,+0,+0} and {0,0,0,1}
 *   blend                      at the weight before the step, by the cross-fade's rules: !(w >= 1e-7f): side a unchanged, side b is
 *                              neither evaluated nor read;  w > 1.0f - 1e-7f: side b unchanged, side a is not evaluated;  otherwise
 *                              D.c = D_a.c * (1.0f - w) + D_b.c * w per component and dq = the middle branch of NLerp(dq_a, dq_b)[w]
 *                              (:1271-1275: the sign of the four-term dot picks a + or a -, then Vector4D::Normalize's
 *                              1 / float(sqrt(double(sum))))
 *   axes                       a component of D whose bit is absent from `axes` becomes +0.0f (a select).  D is in the ROOT'S OWN
 *                              frame at t0, not in the clip's: for a clip that starts turned, X there is not the clip's X
 *   placement {p, ., h}        p.c = p.c + rotate(D, M(h)).c with M(h) of the heading BEFORE the step;  h' = h * dq;
 *                              with MMDX_ROOT_NORMALIZE h' = (h * dq).Normalize() (:457-465: s = x*x + y*y + z*z + w*w left to
 *                              right, n = 1.0f / float(sqrt(double(s))) as math::sqrt does (L/util/math.inl:28-30), four products)
 * There are no short circuits beyond the blend's: an identity dq is still multiplied (a -0 in the heading may become +0), NaN and
 * infinity propagate as IEEE gives them.  Without MMDX_ROOT_NORMALIZE the heading's norm drifts by a rounding per step, as any
 * chained product does; mmdx_palette_place does not normalise either, so a long-lived crowd wants the flag.
 *
 * flags: MMDX_ANIM_DT_ON_DEVICE | MMDX_ROOT_NORMALIZE, other bits rejected.  Every refusal of mmdx_animator_root_motion applies with
 * the same status.  Not here: yaw-only extraction, matrix-form placements, a select form, scale.
 *
 * mmdx_bone_motion_in_place_turn (host only) is mmdx_bone_motion_in_place, and in addition every key of `bone` gets the rotation
 * {+0,+0,+0,1}.  Such a track evaluates to the identity at every time, in every bit: between two keys the weights (1 - lam) + lam
 * give exactly 1 in binary32 for lam in [0, 1], and the normalisation then multiplies by 1.  A set made of such motions gives the
 * poses with the root's motion and turning taken out; the placement carries both.  As above, the split is faithful
 * only when every moved bone descends from `bone`; the call does not check it.  Refusals as mmdx_bone_motion_in_place. */
enum { MMDX_ROOT_NORMALIZE = 1u << 14 };   /* mmdx_animator_root_motion_turn: normalise the heading after the product */
typedef struct mmdx_root_turn_args {
    uint32_t struct_size, flags;   /* = sizeof(mmdx_root_turn_args); MMDX_ANIM_DT_ON_DEVICE | MMDX_ROOT_NORMALIZE or 0             */
    uint32_t root_bone;            /* a bone of `set` (< its n_bones)                                                              */
    uint32_t axes;                 /* MMDX_ROOT_X | _Y | _Z, in the root's frame at t0; bits outside rejected; 0 allowed           */
    const double *dt;              /* as mmdx_animator_advance: a host value, or a device double with the flag                     */
    float *placements;             /* DEVICE, [NI][MMDX_POSE_FLOATS], the pose form of mmdx_palette_place; 4-byte aligned          */
} mmdx_root_turn_args;
MMDX_API mmdx_status mmdx_animator_root_motion_turn(mmdx_animator_t animator, mmdx_motion_set_t set, mmdx_model_t model,
                                                    const mmdx_root_turn_args *args);
MMDX_API mmdx_status mmdx_bone_motion_in_place_turn(mmdx_bone_motion_t src, uint32_t bone, uint32_t axes, mmdx_bone_motion_t *out_motion);

/* ---- Clip markers: which events fired during the step, per instance, on the device --------------------------------------------------
 * A marker is a time in a clip with a channel (0..31): a foot touching the ground, the hit frame of a swing, the end of a one-shot
 * clip.  mmdx_animator_events reports, for the step that mmdx_animator_advance is ABOUT to take, which channels every instance
 * passed -- a 32-bit mask per instance -- and, optionally, up to four instance lists in ascending order (mmdx_instance_select with
 * MMDX_SELECT_ON_DEVICE takes such a list as it is: the sockets of the feet that landed, the deform of those who blinked).  Like root
 * motion it is called BEFORE advance, with the same dt, on the state advance is about to step; it reads the animator's arrays
 * (clips_a, clips_b, times_a, times_b, weights, speed, fade_rate) and writes none of them.
 *
 * The marker table (mmdx_event_set_t) is made from an animator: it copies the animator's clip count and resolved lengths (the
 * animator may be destroyed afterwards), and keeps the markers sorted by (clip, time) -- markers of equal clip and time in the order
 * given -- behind an offset table first[n_clips + 1].  Markers may come in any order, duplicates are allowed, n_markers == 0 is valid
 * (nothing ever fires).  Creation is host only and refuses, before anything else happens: NULL animator / desc / out or NULL
 * markers with n_markers > 0 and a struct_size mismatch (MMDX_ERR_INVALID_ARGUMENT); clip >= n_clips (MMDX_ERR_BAD_INDEX);
 * channel >= 32, a NaN, negative or > L(clip) time, L the length mmdx_animator_get_info reports (MMDX_ERR_INVALID_ARGUMENT).  The
 * device copy is made by the first call that needs it and stays on that device.
 *
 * The arithmetic is part of the contract: comparisons of doubles only, plus the clocks stated above.  For every instance i < NI, with
 * the state as it stands before advance (L(c), wrap: advance's; near, far, folded: root motion's step 2):
 *   1. s = double(speed) * dt                                       (step 1 of advance).  A NaN s fires nothing on either side.
 *   2. a side (c, t0):  raw = t0 + s;  t1 = wrap(c, raw);  it folded: near = L(c), far = 0.0 when raw >= L(c), else near = 0.0,
 *      far = L(c).  With c >= n_clips (MMDX_CLIP_NONE, an id out of range) nothing fires.
 *   3. a leg from u to v passes the marker time m:
 *        u <= v:     (closed ? u <= m : u < m) && m <= v
 *        otherwise:  v <= m && (closed ? m <= u : m < u)
 *      The direction is that of the leg's own ends, not the sign of s.
 *   4. a side that did not fold is one leg t0 -> t1, open at t0.  A folded side is two legs: t0 -> near, open at t0, and far -> t1,
 *      closed at far: both ends of a seam count.  Further whole laps inside one step are not counted, just as `loops` counts one.
 *   5. fired(side) = the OR of 1u << channel over the markers of clip c that a leg passes
 *   6. out_fired[i] = fired(clips_a, times_a) | (fade_rate > 0 ? fired(clips_b, times_b) : 0).  With MMDX_EVENTS_DOMINANT_SIDE:
 *      fired(clips_b, times_b) alone when fade_rate > 0 && weights[i] > 0.5f, fired(clips_a, times_a) alone otherwise.
 *   7. list l < n_lists holds, in ascending order, every i with (out_fired[i] & list_mask[l]) != 0 and -- when `levels` is given --
 *      levels[i] != MMDX_CULLED.  out_counts[l] is its length, out_counts[l] = 0 for n_lists <= l < MMDX_EVENTS_MAX_LISTS; entries
 *      behind a count keep what they held; an instance may be in several lists.
 *   8. out_fired[i] is written for every i < NI, whatever `levels` says.
 *   9. a NaN step (a device NaN dt) fires nothing: out_fired is all 0 and the counts are 0.  Root motion writes nothing then; here a
 *      stale count would fire last frame's events again on a replay.  A host NaN dt is refused as everywhere.
 * Consequences:
 *   - s == 0 fires nothing (a leg from t0 to t0, open at t0).
 *   - a marker at L of a HOLD clip fires once, in the step that reaches the end: the "clip finished" event.  Sitting on L, nothing.
 *   - a marker at time 0 does not fire in the step in which a clip is started (the requester knows that event already); it fires
 *     at every loop seam.
 *   - after a promotion or a switch in advance's steps 3-4 the new clip starts at its t0: nothing of it fires in that step.
 *   - the clocks are IEEE: an infinite or NaN clock (advance never makes one from finite values) goes through the lines above as it is.
 *
 * mmdx_animator_events.  `model` gives the device, the stream and the recording, as for advance.  The masks cost one launch; with
 * lists a second one follows (per-chunk counts, then the scatter: no atomics, the order is the instance order).  NULL animator /
 * set / args / dt / out_fired, a struct_size mismatch, unknown flag bits, n_lists > MMDX_EVENTS_MAX_LISTS, n_lists > 0 with NULL
 * out_ids / out_counts or list_stride < NI, a misaligned device pointer (dt: 8 bytes, the others: 4), a set whose clip count is not
 * the animator's and a host NaN dt are MMDX_ERR_INVALID_ARGUMENT, each before the first HIP call.  Device, stream and graph rules are
 * advance's: asynchronous on `model`'s stream, a model of another device than the animator's (or than the set's copy) is refused,
 * recordable after one unrecorded run with the same set (a host dt is frozen into the recording), and the animator and the set are
 * pinned by a graph that holds them.  A set keeps a small scratch for the counts: use one set from one stream at a time. */
enum { MMDX_EVENTS_DOMINANT_SIDE = (1u << 15) }; /* mmdx_animator_events: only the side with the larger weight fires (step 6) */
#define MMDX_EVENTS_MAX_LISTS 4

typedef struct mmdx_event_set_s *mmdx_event_set_t;

typedef struct mmdx_event_marker {
    double time;                   /* seconds, 0 <= time <= L(clip)                                                                */
    uint32_t clip;                 /* < n_clips                                                                                    */
    uint32_t channel;              /* < 32: the bit of out_fired                                                                   */
} mmdx_event_marker;               /* 16 bytes */

typedef struct mmdx_event_set_desc {
    uint32_t struct_size;          /* = sizeof(mmdx_event_set_desc)                                                                */
    uint32_t n_markers;            /* 0 allowed                                                                                    */
    const mmdx_event_marker *markers; /* [n_markers] host, any order; NULL only when n_markers == 0                                */
} mmdx_event_set_desc;

typedef struct mmdx_event_set_info {
    uint32_t struct_size;
    uint32_t n_markers, n_clips;
    int32_t device_ordinal;        /* where the device copy lives, -1 = not made yet                                               */
} mmdx_event_set_info;

typedef struct mmdx_events_args {
    uint32_t struct_size, flags;   /* = sizeof(mmdx_events_args); MMDX_ANIM_DT_ON_DEVICE | MMDX_EVENTS_DOMINANT_SIDE or 0          */
    const double *dt;              /* as mmdx_animator_advance: a host value, or a device double with the flag                     */
    uint32_t *out_fired;           /* DEVICE [NI]: bit c set = a marker of channel c was passed during the step                    */
    uint32_t n_lists, list_stride; /* 0..4 lists; list l = out_ids + l * list_stride; list_stride >= NI when n_lists > 0           */
    uint32_t list_mask[MMDX_EVENTS_MAX_LISTS];   /* the channels of each list; entries >= n_lists are not read                     */
    const uint32_t *levels;        /* optional DEVICE [NI]: mmdx_cull_bounds' out_levels; MMDX_CULLED enters no list               */
    uint32_t *out_ids, *out_counts;/* DEVICE; out_counts[MMDX_EVENTS_MAX_LISTS], entries >= n_lists written 0                      */
} mmdx_events_args;

MMDX_API mmdx_status mmdx_event_set_create(mmdx_animator_t animator, const mmdx_event_set_desc *desc, mmdx_event_set_t *out_set);
MMDX_API void mmdx_event_set_destroy(mmdx_event_set_t set);
MMDX_API mmdx_status mmdx_event_set_get_info(mmdx_event_set_t set, mmdx_event_set_info *info);
MMDX_API mmdx_status mmdx_animator_events(mmdx_animator_t animator, mmdx_event_set_t set, mmdx_model_t model,
                                          const mmdx_events_args *args);

/* ---- where every instance stands: palette x world matrix ----------------------------------------------------------------------
 * Every palette the solves above write is in model space.  mmdx_palette_place multiplies each skinning matrix of instance i on the
 * right by that instance's world matrix W[i], so the deform that follows, its bounds and mmdx_cull_bounds are all in world space:
 *     out[i][b] = S[i][b] * W[i]                                  for every bone b of the model
 * This is Matrix4x4<float>::operator* (L/util/math_impl.inl:984-1003): each of the 16 elements is the left-to-right four-term sum
 * a_r1*w_1c + a_r2*w_2c + a_r3*w_3c + a_r4*w_4c in binary32, unfused (the library is built with -ffp-contract=off; models created
 * with MMDX_CREATE_FAST_MATH run the same, uncontracted kernel).  W[i] comes from placements[i] in one of two forms:
 *   pose form (default)            placements[i] is MMDX_POSE_FLOATS = 8 floats {tx, ty, tz, 0, qx, qy, qz, qw}, the layout of a local
 *                                  bone pose.  W = q.ToRotateMatrix() (L/util/math_impl.inl:540-563) with row 4 then set to
 *                                  {tx, ty, tz, 1}: exactly how libmmd builds a bone's local_matrix_ from its rotation and
 *                                  translation (L/motion/poser_impl.inl:161-162) with no local offset -- a placement is "a world
 *                                  bone".  The quaternion is NOT normalised (libmmd does not either); the fourth float is ignored.
 *   matrix form (MMDX_PLACE_MATRIX) placements[i] is 16 floats in libmmd's v[0..15] order: a11, a12, ..., translation in v[12..14].
 *                                  Byte for byte the reference viewer's g_state.model_matrix array (main.cpp:171, :1912-1930).
 *                                  Used as given: scale and shear are the caller's business, and normals come out as the deform
 *                                  makes them from such a palette.
 * There are no short circuits: an identity placement is still multiplied, so a -0 element can become +0 and an infinite element
 * times a zero of W gives NaN, as operator* does.  Results are bit-identical to libmmd's; only the sign and payload of a NaN are
 * not part of the contract (they differ between CPUs and the GPU).
 * The definition is a post-multiplication of the FINISHED skinning matrix.  It is not "the root's parent is a world bone": that
 * would associate as L_c * (L_p * (L_root * W)) and differs in the last bit. */
enum {
    MMDX_PLACE_ON_DEVICE = 1u << 8,   /* placements is a device pointer, read when the kernel RUNS (else host, copied per call)    */
    MMDX_PLACE_MATRIX = 1u << 9       /* placements[i] is a 16-float matrix (else an 8-float pose)                                 */
};
typedef struct mmdx_place_args {
    uint32_t struct_size;      /* = sizeof(mmdx_place_args)                                                                       */
    uint32_t flags;            /* MMDX_PALETTE_ON_DEVICE | MMDX_PLACE_ON_DEVICE | MMDX_OUT_ON_DEVICE | MMDX_PLACE_MATRIX; any other
                                  bit: MMDX_ERR_INVALID_ARGUMENT                                                                   */
    uint32_t n_instances;
    uint32_t reserved0;        /* must be 0                                                                                       */
    const float *palettes;     /* [NI][NB][16], NB = the model's bone count                                                       */
    const float *placements;   /* [NI][8] or, with MMDX_PLACE_MATRIX, [NI][16]                                                    */
    float *out_palettes;       /* [NI][NB][16]; may be the same pointer as palettes                                               */
} mmdx_place_args;
/* `model` supplies the bone count, the device and the stream: the call is asynchronous on it, in order with the model's solve and
 * deform calls, and records into mmdx_graph_begin / _end (every operand in device memory then; a recorded call reads palettes AND
 * placements afresh at every replay, so moving the crowd is "rewrite the placement array, launch").
 *  - out_palettes == palettes (in place) is allowed: every lane reads all it needs of a row before it writes that row.  Any other
 *    overlap of the two ranges, and placements overlapping out_palettes, are MMDX_ERR_INVALID_ARGUMENT.
 *  - An operand without its *_ON_DEVICE flag is host memory, copied per call through scratch of the model as mmdx_skeleton_solve
 *    does, and the call returns when the work is done.  The designed path is all three in device memory.
 *  - Device palettes / out_palettes must be 16-byte aligned (every device allocation is), device placements 4-byte aligned.
 *  - n_instances == 0 is MMDX_OK and launches nothing.  NULL model / args / pointers, a struct_size mismatch, an unknown flag bit and
 *    reserved0 != 0 are MMDX_ERR_INVALID_ARGUMENT; a MMDX_CREATE_HOST_ONLY model is MMDX_ERR_NO_DEVICE (after validation). */
MMDX_API mmdx_status mmdx_palette_place(mmdx_model_t model, const mmdx_place_args *args);

/* ---- bone sockets: the frames of chosen bones per instance, on the device -----------------------------------------------------
 * Where is this character's hand, head or saddle right now?  A skinning matrix is global_offset_matrix_ * local_matrix_
 * (L/motion/poser_impl.inl:320-326), and libmmd keeps global_offset_matrix_inv_ next to it (:36-37); multiplying it back gives the
 * bone's frame.  For instance i and socket s, with b = bone[s], p = rest_position[s] and S = palettes[i][b]:
 *     G   = the identity with row 4 = {p.x, p.y, p.z, 1}                                    (global_offset_matrix_inv_)
 *     B   = G * S                                                                           (Matrix4x4<float>::operator*)
 *     out = B            for a socket without an offset
 *     out = O * B        for a socket with one; O is the attachment's frame inside the bone's frame, row-vector convention
 * Every product is Matrix4x4<float>::operator* (L/util/math_impl.inl:984-1003): each of the 16 elements is the left-to-right
 * four-term sum a_r1*b_1c + a_r2*b_2c + a_r3*b_3c + a_r4*b_4c in binary32, unfused -- the rows where G is 0 and 1 included.  There
 * are no short circuits, exactly as mmdx_palette_place states for itself: a -0 can become +0 and an infinite element of S times a
 * zero of G is NaN.  O comes from 8 floats {tx, ty, tz, (ignored), qx, qy, qz, qw} exactly as the pose form of mmdx_palette_place
 * builds W (not normalised), or, with MMDX_SOCKET_OFFSET_MATRIX, is 16 floats used as given; the set expands a pose on the host at
 * creation, so a pose-form offset and the matrix it expands to give identical results.
 * What this is and is not:
 *  - on a model-space palette B is the bone's model-space frame; on a palette that went through mmdx_palette_place it is the bone's
 *    world frame, because G * (S * W);
 *  - rows 1-3 of B reproduce the rows 1-3 of libmmd's local_matrix_ bit for bit when S is finite, up to the sign of a zero;
 *  - row 4 is a recomputation and can differ from libmmd's private local_matrix_ row 4 in the last bits: the contract is the
 *    formula above, not that private field;
 *  - the sign and payload of a NaN are not part of the contract, as elsewhere.
 *
 * A socket set is created on a MODEL (a host that keeps its own bone solve has no mmdx_skeleton_t): the model supplies the bone
 * count, the device, the stream and graph recording.  mmdx_socket_set_create copies the desc's arrays.  n_sockets == 0 or above
 * 65535, a NULL model / desc / bone / rest_position / out_set, a struct_size mismatch, unknown flag bits and reserved0 != 0 are
 * MMDX_ERR_INVALID_ARGUMENT; bone[s] >= the model's bone count is MMDX_ERR_BAD_INDEX.  On a MMDX_CREATE_HOST_ONLY model the set is
 * created and validates; mmdx_palette_sockets then answers MMDX_ERR_NO_DEVICE (after validation).  Lifetime follows the graphs':
 * destroying the model first is allowed and leaves a set that refuses every call (MMDX_ERR_INVALID_ARGUMENT) and can still be
 * destroyed; a set destroyed while a graph holds its table invalidates the graph, and one destroyed during a recording that used
 * it poisons that recording. */
typedef struct mmdx_socket_set_s *mmdx_socket_set_t;
enum { MMDX_SOCKET_OFFSET_MATRIX = 1u << 0 };     /* offsets are [NS][16] matrices (else [NS][8] poses)                             */
typedef struct mmdx_socket_set_desc {
    uint32_t struct_size;            /* = sizeof(mmdx_socket_set_desc)                                                            */
    uint32_t flags;                  /* MMDX_SOCKET_OFFSET_MATRIX; any other bit: MMDX_ERR_INVALID_ARGUMENT                        */
    uint32_t n_sockets;              /* NS, 1 .. 65535                                                                            */
    uint32_t reserved0;              /* must be 0                                                                                 */
    const uint32_t *bone;            /* [NS] < the model's bone count; repeats allowed                                            */
    const float *rest_position;      /* [NS][3] the rest position of bone[s] (mmdx_pmx_get_arrays' rest_position row,
                                        Model::Bone::GetPosition)                                                                 */
    const float *offset;             /* NULL = no socket has one; else [NS][8] or [NS][16]                                        */
    const uint8_t *has_offset;       /* NULL = every socket has one when offset is given; else [NS], 0 = socket s has none (its
                                        row of offset is not read)                                                                */
} mmdx_socket_set_desc;
typedef struct mmdx_socket_set_info {
    uint32_t struct_size;            /* = sizeof(mmdx_socket_set_info), set by the caller                                         */
    uint32_t n_sockets, n_offsets;   /* sockets; how many of them have an offset                                                  */
    uint32_t n_bones;                /* the model's bone count: palettes are [NI][n_bones][16]                                    */
    int32_t device_ordinal;          /* where the table lives; -1 = a host-only model                                             */
    uint32_t reserved0;
} mmdx_socket_set_info;
MMDX_API mmdx_status mmdx_socket_set_create(mmdx_model_t model, const mmdx_socket_set_desc *desc, mmdx_socket_set_t *out_set);
MMDX_API void mmdx_socket_set_destroy(mmdx_socket_set_t set);
MMDX_API mmdx_status mmdx_socket_set_get_info(mmdx_socket_set_t set, mmdx_socket_set_info *info);

typedef struct mmdx_sockets_args {
    uint32_t struct_size;            /* = sizeof(mmdx_sockets_args)                                                               */
    uint32_t flags;                  /* MMDX_PALETTE_ON_DEVICE | MMDX_OUT_ON_DEVICE; any other bit: MMDX_ERR_INVALID_ARGUMENT      */
    uint32_t n_instances;
    uint32_t reserved0;              /* must be 0                                                                                 */
    const float *palettes;           /* [NI][NB][16], NB = the model's bone count                                                 */
    float *out_sockets;              /* [NS][NI][16], SOCKET-major                                                                */
    const mmdx_instance_select *select;   /* NULL = every instance                                                               */
} mmdx_sockets_args;
/* out_sockets[s][i] = the 16 floats of socket s of instance i, in libmmd's v[0..15] order (translation in v[12..14]).
 *  - The output is socket-major on purpose: slab s (out_sockets + s * NI * 16) is byte for byte an [NI][16] placement array for
 *    mmdx_palette_place(MMDX_PLACE_MATRIX | MMDX_PLACE_ON_DEVICE) of ANOTHER model's crowd -- characters holding props and riders
 *    on mounts are one more node in a recorded graph.
 *  - The call is asynchronous on the stream of the set's model (a borrowed one, mmdx_model_set_stream, included), in order with that
 *    model's solve, place and deform calls, and records into mmdx_graph_begin / _end of that model (both operands, and the list,
 *    in device memory then); a recorded call reads the palettes afresh at every replay.
 *  - An operand without its *_ON_DEVICE flag is host memory, copied per call through scratch of the model as mmdx_palette_place
 *    does, and the call returns when the work is done.
 *  - select follows mmdx_instance_select as mmdx_deform_batched_select states it: the first min(*count, n_ids) ids are used (count
 *    NULL: n_ids), a device id >= n_instances is skipped (a host one is MMDX_ERR_INVALID_ARGUMENT before anything is launched), an
 *    id listed twice writes the same bytes twice, and every row of an unlisted instance keeps every byte; mmdx_cull_bounds' lists go
 *    in as they are.  With a list, palettes and out_sockets must be in device memory (the staging copies of host operands move
 *    whole arrays); a host list is copied through scratch of the set and the call returns when the work is done.
 *  - out_sockets overlapping palettes is MMDX_ERR_INVALID_ARGUMENT; device palettes / out_sockets must be 16-byte aligned.
 *  - n_instances == 0 is MMDX_OK and launches nothing.  NULL set / args / pointers, a struct_size mismatch, an unknown flag bit and
 *    reserved0 != 0 are MMDX_ERR_INVALID_ARGUMENT; more than 2^23 instances or list positions is MMDX_ERR_UNSUPPORTED; a set of a
 *    MMDX_CREATE_HOST_ONLY model is MMDX_ERR_NO_DEVICE (after validation).  Models created with MMDX_CREATE_FAST_MATH run the same,
 *    uncontracted kernel. */
MMDX_API mmdx_status mmdx_palette_sockets(mmdx_socket_set_t set, const mmdx_sockets_args *args);

/* ---- spring bones: hair, skirts and ribbons swing per instance, on the device ---------------------------------------------------
 * Secondary motion for a crowd.  The reference moves such bones with Bullet on the host, once per Poser (the physics seam below
 * reproduces that for one hero model); a crowd cannot step a Bullet world per character.  A spring set is CHAINS of bones that
 * follow their parent with inertia, stiffness, drag, gravity and sphere colliders; mmdx_spring_step advances every chain of every
 * (listed) instance by one step in ONE launch and rewrites the chains' palette rows IN PLACE.  There is no libmmd counterpart
 * (Bullet is out of scope): the contract is the arithmetic below, in IEEE binary32 operations in the order written, unfused.
 *
 * The step works on palettes alone.  x . S (pt below) is where a rest-space point x carried by a bone with skinning row S stands
 * now, so the step needs no local matrices and no solver state, runs after any solve form, reads the rows of anchor and collider
 * bones and overwrites the rows of the chains' joints -- what Synchronize does at the physics seam.  Called AFTER mmdx_palette_place
 * the simulation is in world space: walking and turning drag the hair and gravity is the world's.  Called BEFORE it the simulation
 * is in model space.  The call cannot tell the difference and takes no flag for it.  mmdx_palette_bounds after it stays
 * conservative, because it reads the rewritten rows.  The frame order is solve -> place -> springs -> palette bounds -> cull ->
 * deform select.
 *  - A joint ignores its own clip pose: its target is the rigid continuation of its parent (MMD physics bones carry no keys).
 *  - Bones below a chain that are not joints keep their solved rows; post-physics bones hanging off a joint would need Fix and
 *    rigid followers, which this call does not do.  Branching chains, capsule or plane colliders, per-instance wind and reading
 *    PMX rigid-body blocks are out of scope as well.
 *
 * Notation.  pt(x, S)[c] = ((x0*S[c] + x1*S[4+c]) + x2*S[8+c]) + 1.0f*S[12+c], c = 0..2 (Matrix4x4 row-vector product, left to
 * right).  len(d) = float(sqrt(double((d0*d0 + d1*d1) + d2*d2))).  finite(x) is x - x == 0.  Vector lines are per component.
 * Per instance, chains are independent; within a chain the joints run in order, the root side first.  For the joint with bone b:
 * h = rest position of b, t = its tail rest point, P = the parent's CURRENT row (the first joint: the row of the chain's anchor, its
 * skeleton parent, read from the palette; later joints: the row just computed for the previous joint), c and p = the joint's current
 * and previous tail (3 floats each, device state owned by the set, per instance).  The chain has stiffness, drag, gravity_scale,
 * radius; the set a gravity vector g.  dt is one float for the call.
 *   1. H = pt(h, P), T0 = pt(t, P), a = T0 - H, la = len(a).  If !(la > 0) or !finite(la): row = P (all 16 floats), c = p = T0, the
 *      joint is done.
 *   2. If MMDX_SPRING_RESET, or any component of c or p is not finite: c = p = T0 (state heals itself after a NaN frame; a new set's
 *      state is NaN, so its first step is a reset).
 *   3. If dt > 0: n = c + (c - p)*(1.0f - drag); n = n + (T0 - c)*(stiffness*dt); n = n + g*(gravity_scale*dt).  Else (0, negative,
 *      NaN): n = c.
 *   4. constrain(n): if n == T0 in all three components n stays as it is (T0 is at la from H by la's own definition, and
 *      (a / la)*la need not round back to a); else d = n - H, l = len(d); if !(l > 0) or !finite(l): n = T0; else n = H + (d / l)*la.
 *   5. For each collider j in order: C = pt(centre[j], S[collider_bone[j]]), rr = r[j] + radius, d = n - C, l = len(d); if l > 0 and
 *      l < rr: n = C + (d / l)*rr, then constrain(n) again.
 *   6. p = c, c = n.
 *   7. If n == T0 in all three components: row = P, every bit (rigid following: a reset crowd equals its parents exactly).  Else
 *      u = a / la, v = (n - H) / la, k = u x v = {u1*v2 - u2*v1, u2*v0 - u0*v2, u0*v1 - u1*v0}, cs = (u0*v0 + u1*v1) + u2*v2,
 *      m = 1.0f + cs.  If !(m > 1e-6f) (antiparallel): row = P and c = p = T0.  Else, with q_ij = (k_i*k_j) / m,
 *          R = { cs + q00,  q01 + k2,  q02 - k1,
 *                q01 - k2,  cs + q11,  q12 + k0,
 *                q02 + k1,  q12 - k0,  cs + q22 }          (u . R = v in the row-vector convention)
 *      row[4i+j] = (P[4i]*R[0][j] + P[4i+1]*R[1][j]) + P[4i+2]*R[2][j] for i, j = 0..2; row[12+j] = H[j] - ((h0*row[j] + h1*row[4+j])
 *      + h2*row[8+j]); row[3] = row[7] = row[11] = 0, row[15] = 1.
 * The state of a joint is written in steps 1, 2, 6 and 7 and stored after step 7.  A float32 prototype of exactly this, its parent
 * swaying for 3 000 steps with a collider: relative length error <= 6.0e-7, |R R^T - I| <= 1.4e-6, pt(t, row) within 1 ulp of c.
 *
 * mmdx_spring_set_create validates everything on the host and touches no device.  Rest positions and parents come from the
 * skeleton.  The tail of a joint defaults to the next joint's rest position, that of a chain's last joint to h + (h - h of its
 * skeleton parent).  A bone >= the skeleton's count (joint or collider) is MMDX_ERR_BAD_INDEX.  MMDX_ERR_INVALID_ARGUMENT: a joint
 * whose skeleton parent is not the previous joint of its chain; a first joint without a parent; an anchor (the first joint's parent)
 * or collider bone that is a joint of any chain (a read after a write between lanes); a bone listed twice; a chain of 0 or more than
 * MMDX_SPRING_MAX_JOINTS joints; n_chains == 0 or above 65535; more than MMDX_SPRING_MAX_COLLIDERS colliders; NaN in chain_params,
 * gravity, joint_tail or collider_sphere; drag outside [0, 1]; max_instances == 0; NULL arrays; reserved0 != 0; a struct_size
 * mismatch. */
typedef struct mmdx_spring_set_s *mmdx_spring_set_t;
#define MMDX_SPRING_MAX_JOINTS 32
#define MMDX_SPRING_MAX_COLLIDERS 16
enum {
    MMDX_SPRING_RESET = (1u << 16),          /* mmdx_spring_step: step 2 resets every joint it steps                                */
    MMDX_SPRING_DT_ON_DEVICE = (1u << 17)    /* mmdx_spring_step: dt is a device pointer, read when the kernel RUNS                 */
};
typedef struct mmdx_spring_set_desc {
    uint32_t struct_size;            /* = sizeof(mmdx_spring_set_desc)                                                            */
    uint32_t n_chains;               /* >= 1                                                                                      */
    uint32_t n_colliders;            /* 0 .. MMDX_SPRING_MAX_COLLIDERS                                                            */
    uint32_t max_instances;          /* the state holds this many instances; >= 1                                                 */
    const uint32_t *chain_offset;    /* [n_chains + 1], chain c = joints [chain_offset[c], chain_offset[c + 1]); [0] == 0          */
    const uint32_t *joint_bone;      /* [n_joints], n_joints = chain_offset[n_chains], chain after chain, the root side first      */
    const float *joint_tail;         /* NULL = the defaults; else [n_joints][3] rest-space tail points                             */
    const float *chain_params;       /* [n_chains][4] stiffness, drag, gravity scale, radius                                       */
    const uint32_t *collider_bone;   /* [n_colliders]                                                                             */
    const float *collider_sphere;    /* [n_colliders][4] rest-space centre xyz, radius                                            */
    float gravity[3];
    uint32_t reserved0;              /* must be 0                                                                                 */
} mmdx_spring_set_desc;
typedef struct mmdx_spring_set_info {
    uint32_t struct_size;            /* = sizeof(mmdx_spring_set_info), set by the caller                                         */
    uint32_t n_chains, n_joints, n_colliders, max_instances;
    uint32_t n_bones;                /* the skeleton's bone count: palettes are [NI][n_bones][16]                                 */
    int32_t device_ordinal;          /* where the table and the state live; -1 = nowhere yet (the first step decides)             */
    uint32_t reserved0;
} mmdx_spring_set_info;
MMDX_API mmdx_status mmdx_spring_set_create(mmdx_skeleton_t skeleton, const mmdx_spring_set_desc *desc, mmdx_spring_set_t *out_set);
MMDX_API void mmdx_spring_set_destroy(mmdx_spring_set_t set);
MMDX_API mmdx_status mmdx_spring_set_get_info(mmdx_spring_set_t set, mmdx_spring_set_info *info);

typedef struct mmdx_spring_args {
    uint32_t struct_size;            /* = sizeof(mmdx_spring_args)                                                                */
    uint32_t flags;                  /* MMDX_PALETTE_ON_DEVICE (required) | MMDX_SPRING_RESET | MMDX_SPRING_DT_ON_DEVICE            */
    uint32_t n_instances;            /* NI <= the set's max_instances                                                             */
    uint32_t reserved0;              /* must be 0                                                                                 */
    float *palettes;                 /* DEVICE [NI][NB][16], 16-byte aligned, rewritten in place                                  */
    const float *dt;                 /* one float: host memory, or device memory (4-byte aligned) with MMDX_SPRING_DT_ON_DEVICE    */
    const mmdx_instance_select *select;   /* NULL = every instance                                                               */
} mmdx_spring_args;
/* One step of every chain of every instance (of the listed instances) on `model`'s stream (NULL: the selected device's default
 * stream), as the rig calls take their model.
 *   1. Only joint rows are written, of the listed instances, or of all instances without a list; every other byte of palettes
 *      stays as it is.
 *   2. The state of unlisted instances is untouched.  State belongs to the INSTANCE (ids[k]), not to the list position.
 *   3. select follows mmdx_instance_select as mmdx_deform_batched_select states it: the first min(*count, n_ids) ids are used (count
 *      NULL: n_ids); a device id >= n_instances is skipped; a host id >= n_instances is MMDX_ERR_INVALID_ARGUMENT before anything is
 *      launched.  A host list is copied through scratch of the set and the call returns when the work is done.
 *   4. The ids of one call must be distinct: an instance listed twice would be stepped by two lanes at once (undefined state, no
 *      access outside the arrays).
 *   5. The call is asynchronous on the model's stream (a borrowed one, mmdx_model_set_stream, included), in order with that model's
 *      solve, place, bounds and deform calls.  A host dt is passed by value when the call is made.
 *   6. It records into mmdx_graph_begin / _end of `model` with a device dt and a device list (or none); a host dt or a host list is
 *      MMDX_ERR_INVALID_ARGUMENT while recording, and so is a set that has not run on that device before (its table and state are
 *      uploaded by the first call).  A recorded call reads dt and the list afresh at every replay.
 *   7. The set is pinned by the graphs it took part in: destroying it invalidates them, as for every other handle.
 *   8. Unknown flag bits, a missing MMDX_PALETTE_ON_DEVICE, reserved0 != 0, NULL set / args / palettes / dt, misaligned device
 *      pointers, n_instances > max_instances and a struct_size mismatch are MMDX_ERR_INVALID_ARGUMENT; a host NaN dt is legal (step
 *      3: nothing integrates).  More than 2^24 instances or list positions in one call is MMDX_ERR_UNSUPPORTED.  n_instances == 0 is
 *      MMDX_OK and launches nothing. */
MMDX_API mmdx_status mmdx_spring_step(mmdx_spring_set_t set, mmdx_model_t model, const mmdx_spring_args *args);
/* The state of the first n_instances instances, host arrays [n_instances][n_joints][6] = {c xyz, p xyz}, in stream order behind the
 * work queued on `model`'s stream; both return when the copy is done.  For tests and save / restore.  Before the first step (or
 * set_state) on a device, get_state answers NaN everywhere.  Refused while a graph is being recorded. */
MMDX_API mmdx_status mmdx_spring_get_state(mmdx_spring_set_t set, mmdx_model_t model, uint32_t n_instances, float *out_state);
MMDX_API mmdx_status mmdx_spring_set_state(mmdx_spring_set_t set, mmdx_model_t model, uint32_t n_instances, const float *state);

/* ---- look-at: heads and eyes of a crowd turn to device-side targets --------------------------------------------------------------
 * An aim set turns chosen bones of every (listed) instance towards a per-instance target, on finished palettes, in place, in ONE
 * launch.  A target is four floats, a point and a weight; a slab of mmdx_palette_sockets ("where the hero's head is, per instance")
 * or a placement array goes in as it is.  There is no libmmd counterpart (the reference has no look-at): the contract is the
 * arithmetic below, in IEEE binary32 operations in the order written, unfused, as for the springs.
 *
 * Rotating a bone of a finished palette about its current pivot is a right-multiplication of its row by a rigid matrix M, and the
 * same right-multiplication for every skeleton descendant: the call "places" every row of a subtree by a per-instance matrix, as
 * mmdx_palette_place(MMDX_PLACE_MATRIX) places a whole palette.  The frame order is solve -> place -> aim -> springs -> palette
 * bounds -> cull -> deform select: aim runs BEFORE the springs, because hair chains anchor on the head row that aim rewrites; after
 * mmdx_palette_place the targets are world points, before it model-space points.
 *  - The hierarchy is the skeleton's parent array ONLY.  Append and IK relations are not followed: an aim on the spine moves
 *    IK-placed hands with it, which is the caller's choice.
 *  - The aim is by the eye: it is exact only when the eye lies on the pivot of the link; each later link reduces the remainder.
 *  - Damping and turn-rate limits (which need state), up vectors and roll control, and following append relations are out of scope.
 *    The weight in tgt[3] is how a caller fades a look in and out.
 *
 * An aim is L = 1 .. MMDX_AIM_MAX_LINKS link bones b_0 .. b_{L-1}, the root side first, each a strict skeleton ancestor of the next
 * (not necessarily its parent: upper body 2, neck, head); an eye bone be, which is b_{L-1} or a descendant of it; a rest-space eye
 * point e and a rest-space forward vector f, both carried by be; and per link a share in [0, 1] and a cos_limit in [-1, 1], the
 * cosine of the largest turn the link may add to its animated pose (a cosine, so that no host cos enters the contract).  The call
 * rewrites the rows of every bone in the subtree of b_0.
 *
 * Notation.  pt, len and finite as in the spring section; dir(x, S)[c] = (x0*S[c] + x1*S[4+c]) + x2*S[8+c]; mul(A, B) is
 * Matrix4x4::operator*, row r of the result = the row product of mmdx_palette_place over A's row r and B, all 16 elements, no short
 * circuit.  Vector lines are per component.  Per instance i and aim:
 *   0. tgt = the 4 floats at targets + i*target_stride (at targets when the stride is 0); g = tgt[0..2], w = tgt[3].  If !(w > 0) or
 *      any of the four is not finite: nothing of this instance is written for this aim, every byte stays.  Else w = min(w, 1.0f).
 *      The cumulative matrix C is unset.
 *   1. For each link l = 0 .. L-1: P = the row of b_l, Q = the row of be, as read from the palette; if C is set, P = mul(P, C) and
 *      Q = mul(Q, C).  H = pt(h_l, P) with h_l the rest position of b_l; E = pt(e, Q); a = dir(f, Q), la = len(a); d = g - E,
 *      ld = len(d).  The link is SKIPPED (C unchanged) if !(la > 0), !(ld > 0), or either is not finite.  u = a / la, v = d / ld; if
 *      u == v in all three components: skipped.  t = share_l*w.  If t >= 1.0f: v2 = v.  Else n = u + (v - u)*t, ln = len(n); if
 *      !(ln > 0): skipped; else v2 = n / ln.
 *      Limit.  cs = (u0*v2_0 + u1*v2_1) + u2*v2_2.  If cs < cos_limit_l: p = v2 - u*cs, lp = len(p); if !(lp > 0): skipped; else
 *      v2 = u*cos_limit_l + (p / lp)*sin_limit_l, with sin_limit_l = float(sqrt(double(1.0f - cos_limit_l*cos_limit_l))) from the
 *      set's table, and cs is computed again from the new v2 by the same line.
 *      Rotation.  R = the shortest rotation u -> v2 by the formula of spring step 7: k = u x v2, m = 1.0f + cs, q_ij = (k_i*k_j) / m;
 *      if !(m > 1e-6f) (antiparallel): skipped.
 *      Link matrix.  Rows 1-3 of M_l are {R[r][0], R[r][1], R[r][2], 0}, row 4 is {T0, T1, T2, 1} with
 *      T_j = H_j - ((H0*R[0][j] + H1*R[1][j]) + H2*R[2][j]).  C = M_l if C was unset, else C = mul(C, M_l) with its fourth column set
 *      to {0, 0, 0, 1} afterwards (which the product gives by itself unless C holds a non-finite value: the fourth column of C is a
 *      constant).  C_l = C.  A skipped link has C_l = C_{l-1}; C_l is unset while no link has been applied.
 *   2. Every bone s of the subtree has a depth k(s) = the deepest link that is s or an ancestor of s.  If C_{k(s)} is set:
 *      row'(s) = mul(row(s), C_{k(s)}); else the row is not written.  All reads of step 1 see the rows as they were before the call.
 * Sign and payload of a NaN are not part of the contract.  A float32 prototype of exactly this, evaluated in float64, over the case
 * table of the tests and 3 000 steps of a target circling a swaying 41-bone rig: with L = 1, share 1, limit -1 and e = h the new
 * forward direction is within 4.4e-7 of v per component; |R R^T - I| <= 3.7e-6 / m (u and v2 are unit vectors to a rounding error,
 * which the formula divides by m, as spring step 7 does); |pt(h_l, row'(b_l)) - H| <= 4.2e-7 * max(1, |H|).
 *
 * mmdx_aim_set_create validates everything on the host and touches no device.  Rest positions and parents come from the skeleton.
 * A bone >= the skeleton's count (link or eye) is MMDX_ERR_BAD_INDEX.  MMDX_ERR_INVALID_ARGUMENT: a link that is not a strict
 * descendant of the link before it; an eye bone outside the subtree of the last link; an aim of 0 or more than MMDX_AIM_MAX_LINKS
 * links; n_aims == 0 or above MMDX_AIM_MAX_AIMS; a share outside [0, 1]; a cos_limit outside [-1, 1]; NaN anywhere; a zero or
 * non-finite forward; subtrees of two aims that intersect (one workgroup owns a subtree: eyes under an aimed head are a second set
 * and a second call); NULL arrays; reserved0 != 0; a struct_size mismatch.  A skeleton of more than 2^20 bones is
 * MMDX_ERR_UNSUPPORTED. */
typedef struct mmdx_aim_set_s *mmdx_aim_set_t;
#define MMDX_AIM_MAX_AIMS 16
#define MMDX_AIM_MAX_LINKS 4
enum { MMDX_AIM_TARGETS_ON_DEVICE = (1u << 18) };   /* mmdx_palette_aim: targets is a device pointer, read when the kernel RUNS    */
typedef struct mmdx_aim_set_desc {
    uint32_t struct_size;            /* = sizeof(mmdx_aim_set_desc)                                                               */
    uint32_t n_aims;                 /* 1 .. MMDX_AIM_MAX_AIMS                                                                    */
    const uint32_t *link_offset;     /* [n_aims + 1], aim a = links [link_offset[a], link_offset[a + 1]); [0] == 0                 */
    const uint32_t *link_bone;       /* [n_links], n_links = link_offset[n_aims], aim after aim, the root side first               */
    const float *link_params;        /* [n_links][2] share, cos_limit                                                             */
    const uint32_t *eye_bone;        /* [n_aims]                                                                                  */
    const float *eye_point;          /* [n_aims][3] rest-space                                                                    */
    const float *forward;            /* [n_aims][3] rest-space, any length but zero                                               */
    uint32_t reserved0;              /* must be 0                                                                                 */
} mmdx_aim_set_desc;
typedef struct mmdx_aim_set_info {
    uint32_t struct_size;            /* = sizeof(mmdx_aim_set_info), set by the caller                                            */
    uint32_t n_aims, n_links;
    uint32_t n_subtree_rows;         /* palette rows one instance has rewritten when every aim applies                            */
    uint32_t n_bones;                /* the skeleton's bone count: palettes are [NI][n_bones][16]                                 */
    int32_t device_ordinal;          /* where the table lives; -1 = nowhere yet (the first call decides)                          */
} mmdx_aim_set_info;
MMDX_API mmdx_status mmdx_aim_set_create(mmdx_skeleton_t skeleton, const mmdx_aim_set_desc *desc, mmdx_aim_set_t *out_set);
MMDX_API void mmdx_aim_set_destroy(mmdx_aim_set_t set);
MMDX_API mmdx_status mmdx_aim_set_get_info(mmdx_aim_set_t set, mmdx_aim_set_info *info);

typedef struct mmdx_aim_args {
    uint32_t struct_size;            /* = sizeof(mmdx_aim_args)                                                                   */
    uint32_t flags;                  /* MMDX_PALETTE_ON_DEVICE (required) | MMDX_AIM_TARGETS_ON_DEVICE                             */
    uint32_t n_instances;            /* NI                                                                                        */
    uint32_t target_stride;          /* in floats: 0 = one target for everyone, else a multiple of 4 (>= 4)                       */
    float *palettes;                 /* DEVICE [NI][NB][16], 16-byte aligned, rewritten in place                                  */
    const float *targets;            /* {x, y, z, weight} per instance: host memory, or device memory (16-byte aligned) with
                                        MMDX_AIM_TARGETS_ON_DEVICE.  Stride 16 and targets = slab + 12: a slab of
                                        mmdx_palette_sockets as it is, its v[15] = 1 the weight                                   */
    const mmdx_instance_select *select;   /* NULL = every instance                                                               */
} mmdx_aim_args;
/* Every aim of every instance (of the listed instances) on `model`'s stream (NULL: the selected device's default stream), as the
 * rig calls and mmdx_spring_step take their model.
 *   1. Only rows of the aims' subtrees are written, of the listed instances, or of all instances without a list; every other byte of
 *      palettes stays as it is.
 *   2. select follows mmdx_instance_select as mmdx_deform_batched_select states it: the first min(*count, n_ids) ids are used (count
 *      NULL: n_ids); a device id >= n_instances is skipped; a host id >= n_instances is MMDX_ERR_INVALID_ARGUMENT before anything is
 *      launched.  A host list is copied through scratch of the set and the call returns when the work is done.  The target of a
 *      listed instance is that of the INSTANCE (ids[k]), not of the list position.
 *   3. The ids of one call must be distinct: an instance listed twice would be rewritten by two workgroups at once (undefined rows,
 *      no access outside the arrays).
 *   4. The call is asynchronous on the model's stream (a borrowed one, mmdx_model_set_stream, included), in order with that model's
 *      solve, place, spring, bounds and deform calls.  Host targets are copied through scratch of the set and the call returns when
 *      the work is done.
 *   5. It records into mmdx_graph_begin / _end of `model` with device targets and a device list (or none); host targets or a host
 *      list are MMDX_ERR_INVALID_ARGUMENT while recording, and so is a set that has not run on that device before (its table is
 *      uploaded by the first call).  A recorded call reads targets and list afresh at every replay.
 *   6. The set is pinned by the graphs it took part in: destroying it invalidates them, as for every other handle.
 *   7. Unknown flag bits, a missing MMDX_PALETTE_ON_DEVICE, a target_stride that is neither 0 nor a multiple of 4, NULL set / args /
 *      palettes / targets, misaligned device pointers and a struct_size mismatch are MMDX_ERR_INVALID_ARGUMENT.  More than 2^23
 *      instances or list positions in one call is MMDX_ERR_UNSUPPORTED.  n_instances == 0 is MMDX_OK and launches nothing.
 * MMDX_AIM_BLOCK=64 (read per call, for tests and A/B) makes a workgroup own 64 instances instead of 16. */
MMDX_API mmdx_status mmdx_palette_aim(mmdx_aim_set_t set, mmdx_model_t model, const mmdx_aim_args *args);

/* ---- reach: two-bone IK moves hands and feet of a crowd to device-side targets ---------------------------------------------------
 * A reach set puts the tip of a two-bone limb (upper arm - forearm - hand, thigh - shin - foot) of every (listed) instance on a
 * per-instance target, on finished palettes, in place, in ONE launch.  A target is four floats, a point and a weight, read as
 * mmdx_palette_aim reads it: a slab of mmdx_palette_sockets ("where the prop's handle is, per instance") or a placement array goes in
 * as it is.  The solve is analytic (the law of cosines); there is no libmmd counterpart, so the contract is the arithmetic below, in
 * IEEE binary32 operations in the order written, unfused, lengths by float(sqrt(double(s))), no trigonometry, as for the springs and
 * the aim.  The skeleton solver's CCD-IK is a different thing: its targets are bones of the clip in model space, inside the solve.
 *
 * The frame order is solve -> place -> aim -> reach -> springs -> palette bounds -> cull -> deform select: reach runs AFTER aim,
 * because an aimed spine carries the arms, and BEFORE the springs, because sleeves and ribbons anchor on rows that reach rewrites.
 *  - The hierarchy is the skeleton's parent array ONLY.  Append and IK relations are not followed.
 *  - Joint angle limits and hinge axes, twist distribution, chains longer than two bones and damping (which needs state) are out
 *    of scope.  The caller supplies the target, and the weight in tgt[3] fades a reach in and out; foot targets over a height field
 *    come from mmdx_ground_targets (the ground section below).
 *
 * A reach names three bones: a (upper arm, thigh), b (elbow, knee), c (wrist, ankle), each a strict skeleton ancestor of the next
 * (not necessarily its parent: MMD arms have twist bones in between); a rest-space tip point e carried by c; a rest-space pole
 * vector carried by a, the bend direction of a straight limb; a max_extension in (0, 1], the share of its length the limb never
 * stretches past; and flags.  The call rewrites the rows of every bone in the subtree of a.
 *
 * Notation.  pt, dir, len, mul and finite as in the aim section; dot(x, y) = (x0*y0 + x1*y1) + x2*y2; h_s the rest position of
 * bone s.  rot(u, v, H), the shortest rotation from u to v about the pivot H, is aim step 1's "Rotation" and "Link matrix": if u == v
 * in all three components the identity matrix exactly; else cs = dot(u, v), k = u x v, m = 1.0f + cs, FAILS if !(m > 1e-6f),
 * q_ij = (k_i*k_j) / m, R = {{cs + q00, q01 + k2, q02 - k1}, {q01 - k2, cs + q11, q12 + k0}, {q02 + k1, q12 - k0, cs + q22}}, rows
 * 1-3 {R[r][0], R[r][1], R[r][2], 0}, row 4 {T0, T1, T2, 1} with T_j = H_j - ((H0*R[0][j] + H1*R[1][j]) + H2*R[2][j]).  Vector lines
 * are per component.  Per instance i and reach:
 *   0. Target.  tgt = the 4 floats at targets + i*target_stride (at targets when the stride is 0); g = tgt[0..2], w = tgt[3].  If
 *      !(w > 0) or any of the four is not finite: nothing of this instance is written, every byte stays.  Else w = min(w, 1.0f).
 *   1. Points.  A = pt(h_a, row a), B = pt(h_b, row b), K = pt(h_c, row c), T = pt(e, row c).  With MMDX_REACH_KEEP_END_ROTATION the
 *      solved point is the end bone's pivot: G = g - (T - K), then T = K; otherwise G = g.  Gw = G if w >= 1.0f, else
 *      T + (G - T)*w.  l1 = len(B - A), l2 = len(T - B), dv = Gw - A, d = len(dv).  If any of l1, l2, d is not > 0 or not finite:
 *      nothing is written.
 *   2. Clamp.  s = l1 + l2, lmax = s*max_extension, lmin = fabs(l1 - l2) + (s - lmax).  If !(lmin <= lmax): nothing is written.
 *      dc = d < lmin ? lmin : d, then dc = dc > lmax ? lmax : dc.  dh = dv / d, Gc = A + dh*dc.
 *   3. Elbow.  x = ((l1*l1 - l2*l2) + dc*dc) / (2.0f*dc), y2 = l1*l1 - x*x, y = y2 > 0 ? float(sqrt(double(y2))) : 0.  Bend direction:
 *      b = B - A, p = b - dh*dot(b, dh), lp = len(p).  If !(lp > 1e-4f*l1) (a straight or target-aligned limb): b = dir(pole, row a),
 *      p and lp again by the same lines; if then !(lp > 0): nothing is written.  nb = dh*x + (p / lp)*y, v1 = nb / len(nb),
 *      u1 = (B - A) / l1.  M_a = rot(u1, v1, A).
 *   4. Forearm.  B1 = pt(h_b, mul(row b, M_a)), T1 = pt(the solved point, mul(row c, M_a)): e, or h_c with the flag.
 *      u2 = (T1 - B1) / len(T1 - B1), v2 = (Gc - B1) / len(Gc - B1); a length that is not > 0 or not finite: nothing is written.
 *      M_b = rot(u2, v2, B1).  C_0 = M_a.  C_1 = mul(M_a, M_b) with its fourth column set to {0, 0, 0, 1} afterwards (which the
 *      product gives by itself for finite values, as for the aim).
 *   5. End bone.  Without the flag C_2 = C_1.  With it C_2 is the pure translation by pt(h_c, mul(row c, C_1)) - K: rows 1-3 those
 *      of the identity exactly, so a planted foot keeps its animated orientation, its 3x3 value for value.
 *   6. Writes.  Every bone s of the subtree of a has a depth k(s) = 0, 1 or 2: the deepest of a, b, c that is s or an ancestor of
 *      s.  row'(s) = mul(row(s), C_{k(s)}).  All reads see the rows as they were before the call.  A failure in steps 1-4 (a
 *      "nothing is written", a rot that fails) writes nothing for this (instance, reach): all or nothing, unlike the aim's per-link
 *      skip.
 * Sign and payload of a NaN are not part of the contract.  A float32 prototype of exactly this, evaluated in float64, over the case
 * table of the tests and 3 000 steps of a target circling a swaying 41-bone rig (seven sets, both flag values, 30 067 applied reaches):
 * the tip (with the flag: the pivot of c) ends within 4.6e-5 * max(1, |Gc|) of Gc (2.8e-6 where both rotations have m > 0.1; the
 * worst is at m = 1.1e-3 and the error does not grow further towards m = 0); |B' - A| and |T' - B'| keep l1 and l2 to 4.6e-5 relative
 * (7.0e-6 where m > 0.1); the new elbow leaves the plane of dh and the bend direction by at most 4.4e-6 * l1.  Only the rigidity goes
 * with 1 / m (u and v of a rot are unit vectors to a rounding error, which the formula divides by m, as the aim's does):
 * |C C^T - I| <= 1.2e-6 / m for the 3x3 of C_0 (m of M_a) and of C_1 (the smaller m of M_a and M_b); the smallest m met was 6.7e-6.
 *
 * mmdx_reach_set_create validates everything on the host and touches no device.  Rest positions and parents come from the skeleton.
 * A bone >= the skeleton's count is MMDX_ERR_BAD_INDEX.  MMDX_ERR_INVALID_ARGUMENT: b not a strict descendant of a, or c not of b;
 * max_extension outside (0, 1]; NaN anywhere; a zero or non-finite pole; n_reaches == 0 or above MMDX_REACH_MAX_REACHES; unknown
 * per-reach flag bits; subtrees of two reaches that intersect (one workgroup owns a subtree: a reach under an aimed spine is a
 * different set and call); NULL arrays; reserved0 != 0; a struct_size mismatch.  A skeleton of more than 2^20 bones is
 * MMDX_ERR_UNSUPPORTED. */
typedef struct mmdx_reach_set_s *mmdx_reach_set_t;
#define MMDX_REACH_MAX_REACHES 16
enum { MMDX_REACH_TARGETS_ON_DEVICE = (1u << 19) }; /* mmdx_palette_reach: targets is a device pointer, read when the kernel RUNS  */
enum { MMDX_REACH_KEEP_END_ROTATION = 1u };         /* mmdx_reach_set_desc.flags[r]: solve for the pivot of c, translate its subtree */
typedef struct mmdx_reach_set_desc {
    uint32_t struct_size;            /* = sizeof(mmdx_reach_set_desc)                                                             */
    uint32_t n_reaches;              /* 1 .. MMDX_REACH_MAX_REACHES                                                               */
    const uint32_t *bones;           /* [n_reaches][3] a, b, c                                                                    */
    const float *tip_point;          /* [n_reaches][3] rest-space e                                                               */
    const float *pole;               /* [n_reaches][3] rest-space, any length but zero                                            */
    const float *max_extension;      /* [n_reaches] in (0, 1]                                                                     */
    const uint32_t *flags;           /* [n_reaches] 0 | MMDX_REACH_KEEP_END_ROTATION                                              */
    uint32_t reserved0;              /* must be 0                                                                                 */
} mmdx_reach_set_desc;
typedef struct mmdx_reach_set_info {
    uint32_t struct_size;            /* = sizeof(mmdx_reach_set_info), set by the caller                                          */
    uint32_t n_reaches;
    uint32_t n_subtree_rows;         /* palette rows one instance has rewritten when every reach applies                          */
    uint32_t n_bones;                /* the skeleton's bone count: palettes are [NI][n_bones][16]                                 */
    int32_t device_ordinal;          /* where the table lives; -1 = nowhere yet (the first call decides)                          */
    uint32_t reserved0;
} mmdx_reach_set_info;
MMDX_API mmdx_status mmdx_reach_set_create(mmdx_skeleton_t skeleton, const mmdx_reach_set_desc *desc, mmdx_reach_set_t *out_set);
MMDX_API void mmdx_reach_set_destroy(mmdx_reach_set_t set);
MMDX_API mmdx_status mmdx_reach_set_get_info(mmdx_reach_set_t set, mmdx_reach_set_info *info);

typedef struct mmdx_reach_args {
    uint32_t struct_size;            /* = sizeof(mmdx_reach_args)                                                                 */
    uint32_t flags;                  /* MMDX_PALETTE_ON_DEVICE (required) | MMDX_REACH_TARGETS_ON_DEVICE                           */
    uint32_t n_instances;            /* NI                                                                                        */
    uint32_t target_stride;          /* in floats: 0 = one target for everyone, else a multiple of 4 (>= 4)                       */
    float *palettes;                 /* DEVICE [NI][NB][16], 16-byte aligned, rewritten in place                                  */
    const float *targets;            /* {x, y, z, weight} per instance, for EVERY reach of the set: host memory, or device memory
                                        (16-byte aligned) with MMDX_REACH_TARGETS_ON_DEVICE.  Stride 16 and targets = slab + 12: a
                                        slab of mmdx_palette_sockets as it is, its v[15] = 1 the weight.  Two hands on two
                                        targets are two sets and two calls                                                        */
    const mmdx_instance_select *select;   /* NULL = every instance                                                               */
} mmdx_reach_args;
/* Every reach of every instance (of the listed instances) on `model`'s stream (NULL: the selected device's default stream), as
 * mmdx_palette_aim takes its model.
 *   1. Only rows of the reaches' subtrees are written, of the listed instances, or of all instances without a list; every other byte
 *      of palettes stays as it is.
 *   2. select follows mmdx_instance_select as mmdx_deform_batched_select states it: the first min(*count, n_ids) ids are used (count
 *      NULL: n_ids); a device id >= n_instances is skipped; a host id >= n_instances is MMDX_ERR_INVALID_ARGUMENT before anything is
 *      launched.  A host list is copied through scratch of the set and the call returns when the work is done.  The target of a
 *      listed instance is that of the INSTANCE (ids[k]), not of the list position.
 *   3. The ids of one call must be distinct: an instance listed twice would be rewritten by two workgroups at once (undefined rows,
 *      no access outside the arrays).
 *   4. The call is asynchronous on the model's stream (a borrowed one, mmdx_model_set_stream, included), in order with that model's
 *      solve, place, aim, spring, bounds and deform calls.  Host targets are copied through scratch of the set and the call returns
 *      when the work is done.
 *   5. It records into mmdx_graph_begin / _end of `model` with device targets and a device list (or none); host targets or a host
 *      list are MMDX_ERR_INVALID_ARGUMENT while recording, and so is a set that has not run on that device before (its table is
 *      uploaded by the first call).  A recorded call reads targets and list afresh at every replay.
 *   6. The set is pinned by the graphs it took part in: destroying it invalidates them, as for every other handle.
 *   7. Unknown flag bits, a missing MMDX_PALETTE_ON_DEVICE, a target_stride that is neither 0 nor a multiple of 4, NULL set / args /
 *      palettes / targets, misaligned device pointers and a struct_size mismatch are MMDX_ERR_INVALID_ARGUMENT.  More than 2^23
 *      instances or list positions in one call is MMDX_ERR_UNSUPPORTED.  n_instances == 0 is MMDX_OK and launches nothing.
 * A workgroup owns 16 instances (list positions) of one reach at every crowd size. */
MMDX_API mmdx_status mmdx_palette_reach(mmdx_reach_set_t set, mmdx_model_t model, const mmdx_reach_args *args);

/* ---- ground: a height field lifts placements and foot targets on the device ------------------------------------------------------
 * Root motion walks a placement through the world in x and z; a ground gives it its height and gives the reach sets of the feet
 * their targets, without the host: one call puts every (listed) placement on the ground, one call turns the feet's world positions
 * (a mmdx_palette_sockets output) into reach targets that keep each foot's animated height over the ground under that foot, and
 * writes a hip drop so that the lower foot can reach.  A ground is a regular height field in device memory.  There is no libmmd
 * counterpart, so the contract is the arithmetic below, in IEEE binary32 operations in the order written, unfused, as for the
 * springs, the aim and the reach.
 *
 * The frame order is animator -> root motion -> GROUND PLACE -> tracks -> solve -> place -> sockets -> GROUND TARGETS -> aim -> reach
 * -> springs -> palette bounds -> cull -> deform select.  With MMDX_ROOT_X | MMDX_ROOT_Z as root motion's axes the clip keeps its
 * own vertical motion and mmdx_ground_place owns placements[i][1].
 *  - Foot alignment to the slope, tilting the placement to the ground normal and geometry that is no height field are out of scope.
 *
 * The height function h(x, z) of a field of nx samples per row and nz rows, H[nz][nx], origin (origin_x, origin_z), cells
 * (cell_x, cell_z):
 *   Cell and fraction.  u = (x - origin_x) / cell_x.  If u is not finite the sample FAILS.  u = u < 0 ? 0 : u, then
 *      u = u > float(nx-1) ? float(nx-1) : u.  iu = uint32(u) (truncation); if iu > nx-2 then iu = nx-2.  fu = u - float(iu).
 *      v, iv, fv from z, origin_z, cell_z, nz by the same lines.  Outside the field the border continues flat: that is the clamp.
 *   Corners.  h00 = H[iv][iu], h10 = H[iv][iu+1], h01 = H[iv+1][iu], h11 = H[iv+1][iu+1].
 *   Interpolation.  The cell is two triangles split along the diagonal from corner 10 to corner 01, as a height-field mesh is
 *      drawn, so feet stand on the rendered surface (which is not the bilinear patch).  If fu + fv <= 1.0f:
 *         h = (h00*((1.0f - fu) - fv) + h10*fu) + h01*fv
 *      else
 *         h = (h11*((fu + fv) - 1.0f) + h10*(1.0f - fv)) + h01*(1.0f - fu)
 * At a sample point h equals the stored height exactly, up to the sign of a zero, in every cell and at the clamped borders.
 * Measured on the numpy restatement against a binary64 evaluation of the same formulas from the same binary32 x and z (200 000
 * random points in and around each field of the tests: 2 x 2, 3 x 2 and 33 x 17 samples, unequal cells, negative origins, steps
 * between neighbouring samples of up to max|H|): |h - h64| <= 5.7e-7 * max(1, max|H|) = MMDX_GROUND_H_ERROR, rounded up; and h is
 * continuous across the diagonal and across cell edges to the same bound (points a few ulps on either side).  The error is the
 * rounding of u and v, half an ulp of a number up to nx - 1, times the step between neighbouring samples: it grows with the sample
 * count and the steepness, not with the heights themselves.  Heights whose products overflow binary32 are the caller's: nothing is
 * read or written out of bounds, the values are inf or NaN.
 *
 * mmdx_ground_create validates on the host and touches no device.  MMDX_ERR_INVALID_ARGUMENT: a NULL pointer, a struct_size
 * mismatch, any flag bit, reserved0 != 0, nx or nz outside 2 .. 8192, a cell size that is not finite and > 0, a non-finite origin,
 * any non-finite height.  The heights are copied at create; the table is uploaded by the first call on a device and stays there. */
typedef struct mmdx_ground_s *mmdx_ground_t;
#define MMDX_GROUND_MAX_FEET 8
#define MMDX_GROUND_MIN_SAMPLES 2
#define MMDX_GROUND_MAX_SAMPLES 8192
#define MMDX_GROUND_H_ERROR 6e-7f   /* measured, see above; the tests assert four times it */
typedef struct mmdx_ground_desc {
    uint32_t struct_size;            /* = sizeof(mmdx_ground_desc)                                                                */
    uint32_t flags;                  /* none defined: must be 0                                                                   */
    uint32_t nx, nz;                 /* samples per row, rows: MMDX_GROUND_MIN_SAMPLES .. MMDX_GROUND_MAX_SAMPLES each            */
    float origin_x, origin_z;        /* world x, z of H[0][0]                                                                     */
    float cell_x, cell_z;            /* world distance between samples, > 0                                                       */
    const float *heights;            /* HOST [nz][nx], copied by the call                                                         */
    uint32_t reserved0;              /* must be 0                                                                                 */
} mmdx_ground_desc;
typedef struct mmdx_ground_info {
    uint32_t struct_size;            /* = sizeof(mmdx_ground_info), set by the caller                                             */
    uint32_t nx, nz;
    float origin_x, origin_z, cell_x, cell_z;
    float min_height, max_height;
    int32_t device_ordinal;          /* where the table lives; -1 = nowhere yet (the first call decides)                          */
    uint32_t reserved0;
} mmdx_ground_info;
MMDX_API mmdx_status mmdx_ground_create(const mmdx_ground_desc *desc, mmdx_ground_t *out_ground);
MMDX_API void mmdx_ground_destroy(mmdx_ground_t ground);
MMDX_API mmdx_status mmdx_ground_get_info(mmdx_ground_t ground, mmdx_ground_info *info);

typedef struct mmdx_ground_place_args {
    uint32_t struct_size;            /* = sizeof(mmdx_ground_place_args)                                                          */
    uint32_t flags;                  /* none defined: must be 0                                                                   */
    uint32_t n_instances;            /* NI                                                                                        */
    float y_offset;
    float *placements;               /* DEVICE [NI][MMDX_POSE_FLOATS], 4-byte aligned: the array root motion and
                                        mmdx_palette_place share; only placements[i][1] is ever written                           */
    const float *drop;               /* DEVICE [NI], 4-byte aligned, or NULL: last frame's mmdx_ground_targets out_drop           */
    const mmdx_instance_select *select;   /* NULL = every instance                                                               */
} mmdx_ground_place_args;
/* Per (listed) instance i, p = placements[i]: h0 = h(p[0], p[2]).  If the sample fails, or drop is given and drop[i] is not finite,
 * nothing of this instance is written.  Otherwise p[1] = (h0 + y_offset) + drop[i]; without drop p[1] = h0 + y_offset.  Called
 * after root motion and before mmdx_palette_place.  drop may not overlap placements (MMDX_ERR_INVALID_ARGUMENT).  The rules 2, 4,
 * 5, 6 and 7 below mmdx_ground_targets hold here too. */
MMDX_API mmdx_status mmdx_ground_place(mmdx_ground_t ground, mmdx_model_t model, const mmdx_ground_place_args *args);

typedef struct mmdx_ground_targets_args {
    uint32_t struct_size;            /* = sizeof(mmdx_ground_targets_args)                                                        */
    uint32_t flags;                  /* none defined: must be 0                                                                   */
    uint32_t n_instances;            /* NI                                                                                        */
    uint32_t n_feet;                 /* NF: 1 .. MMDX_GROUND_MAX_FEET                                                             */
    const float *placements;         /* DEVICE [NI][MMDX_POSE_FLOATS], 4-byte aligned, read only                                  */
    const float *points;             /* DEVICE, 4-byte aligned: foot f of instance i is the three floats at
                                        points + f*slab_stride + i*point_stride.  points = sockets + 12, point_stride = 16,
                                        slab_stride = NI*16: a mmdx_palette_sockets output as it is                               */
    uint32_t point_stride;           /* in floats, >= 3                                                                           */
    uint32_t slab_stride;            /* in floats, >= 3                                                                           */
    float *out_targets;              /* DEVICE [NF][NI][4], 16-byte aligned, foot-major: slab f is the target array of the reach
                                        set of foot f, with target_stride = 4                                                     */
    float *out_drop;                 /* DEVICE [NI], 4-byte aligned, or NULL                                                      */
    float max_step;                  /* finite, >= 0: the most a target leaves the foot's animated height, up or down             */
    float max_drop;                  /* finite, >= 0: the most the hips are lowered                                               */
    const mmdx_instance_select *select;   /* NULL = every instance                                                               */
} mmdx_ground_targets_args;
/* Per (listed) instance i, ty = placements[i][1], and per foot f with P its point:
 *   hf = h(P.x, P.z).  If that fails, or any of P.x, P.y, P.z, ty is not finite: out_targets[f][i] = {+0, +0, +0, +0} (weight 0: the
 *   reach writes nothing for that limb).  Otherwise dy = hf - ty; dy = dy < -max_step ? -max_step : dy, then
 *   dy = dy > max_step ? max_step : dy; out_targets[f][i] = {P.x, P.y + dy, P.z, 1.0f}.
 * The placement stands at ty, so the clip holds the foot at P.y - ty over it, and the target keeps that height over the ground
 * under the foot: a swing arc survives, a planted foot lands on the slope.  Use the feet's reach sets with
 * MMDX_REACH_KEEP_END_ROTATION.  If out_drop is given: h0 = h(placements[i][0], placements[i][2]); m = 0.0f; then, if h0 did not
 * fail, per foot whose SAMPLE succeeded (whatever P.y and ty are), in foot order: d = hf - h0, m = d < m ? d : m.  So m is the least
 * hf - h0 where that is below 0, and 0 otherwise, if no foot was sampled or if h0 failed; a d that is a NaN is never taken.
 * r = m < 0 ? m : 0, then out_drop[i] = r < -max_drop ? -max_drop : r.  The NEXT frame's mmdx_ground_place reads it: the latency
 * of one frame is deliberate, the call that lowers the hips runs before the solve, the call that knows by how much after it.
 *   1. Only out_targets[f][i] and out_drop[i] of the listed instances (of all without a list) are written; every other byte stays.
 *   2. select follows mmdx_instance_select as mmdx_deform_batched_select states it: the first min(*count, n_ids) ids are used (count
 *      NULL: n_ids); a device id >= n_instances is skipped; a host id >= n_instances is MMDX_ERR_INVALID_ARGUMENT before anything is
 *      launched.  A host list is copied through scratch of the ground and the call returns when the work is done.
 *   3. out_targets and out_drop may overlap neither points nor placements nor each other (MMDX_ERR_INVALID_ARGUMENT).
 *   4. The call is asynchronous on `model`'s stream (NULL: the selected device's default stream; a borrowed stream,
 *      mmdx_model_set_stream, included), in order with that model's other calls.  A MMDX_CREATE_HOST_ONLY model is
 *      MMDX_ERR_NO_DEVICE, after validation.
 *   5. It records into mmdx_graph_begin / _end of `model` with a device list (or none); a host list is MMDX_ERR_INVALID_ARGUMENT
 *      while recording, and so is a ground that has not run on that device before (its table is uploaded by the first call).  A
 *      recorded call reads every array afresh at every replay.
 *   6. The ground is pinned by the graphs it took part in: destroying it invalidates them, as for every other handle.
 *   7. NULL ground / args / pointers (drop and out_drop excepted), a struct_size mismatch, any flag bit, misaligned pointers, a
 *      stride below 3, n_feet outside 1 .. MMDX_GROUND_MAX_FEET, a negative or non-finite max_step / max_drop are
 *      MMDX_ERR_INVALID_ARGUMENT.  More than 2^23 instances or list positions in one call is MMDX_ERR_UNSUPPORTED.
 *      n_instances == 0 is MMDX_OK and launches nothing; ground, args, struct_size, flags, n_feet, the strides, max_step, max_drop
 *      and the list's header are checked before that, no pointer of the arrays is.
 * One lane per instance (list position) loops over the feet: the drop's minimum needs no atomics and is deterministic. */
MMDX_API mmdx_status mmdx_ground_targets(mmdx_ground_t ground, mmdx_model_t model, const mmdx_ground_targets_args *args);

/* ---- a box per instance BEFORE the deform: bone boxes x palette ---------------------------------------------------------------
 * mmdx_deform_batched_bounds gives the box of the vertices it wrote, so a cull that uses it tests last frame's box, and an instance
 * that is not deformed keeps an old one.  mmdx_palette_bounds gives a conservative box of the CURRENT frame from the palette alone
 * (NI x n_boxes matrices instead of NI x NV vertices), so the loop is solve -> place -> palette bounds -> cull -> select-deform.
 *
 * The table (built once by mmdx_model_create, on every model).  From the skin as mmdx_model_get_skin returns it and the base
 * positions and morph offsets as the kernels read them (binary16 widened for MMDX_CREATE_F16_POSITIONS).  Bone b is USED by vertex
 * v: BDEF1 id0; BDEF2 id0 iff w != 0 and id1 iff 1.0f - w != 0; BDEF4 id_k iff w_k != 0.  One row per used bone, ascending:
 *   lo, hi   min / max of the base positions of its vertices;
 *   reach    max over its vertices of R(v), R(v)[axis] = the sum of |offset[axis]| over the vertex-morph entries on v after group
 *            expansion (one per slot application, no rate), summed in double, rounded to float, one nextafter towards +inf.
 * max_vertex_entries = the most such entries on one vertex; weight_sum_dev = max_v |s_v - 1| with s_v the weight sum as applied, in
 * double (BDEF1 1; BDEF2 double(w) + double(1.0f - w); BDEF4 the sum of the four), rounded to float, one nextafter up;
 * eps = float((32 + max_vertex_entries) * 2^-24) + weight_sum_dev (a float addition; DESIGN.md 6.8 derives it); n_nonconvex = the
 * vertices with a negative applied weight (BDEF4 w_k < 0; BDEF2 w < 0 or w > 1).
 *
 * The arithmetic is part of the contract.  Everything is binary32, unfused, in this order (models created with
 * MMDX_CREATE_FAST_MATH run the same, uncontracted kernel), with min(a, b) = b < a ? b : a and max(a, b) = a < b ? b : a,
 * ms = morph_scale, M = palettes[i][bone] (translation in M[3][0..2]).  For every table row and output axis j:
 *   L = lo - reach*ms          H = hi + reach*ms                                  (per component)
 *   pkL = L[k]*M[k][j]         pkH = H[k]*M[k][j]                                 k = 0, 1, 2
 *   mn = ((min(p0L,p0H) + min(p1L,p1H)) + min(p2L,p2H)) + M[3][j]
 *   mx = ((max(p0L,p0H) + max(p1L,p1H)) + max(p2L,p2H)) + M[3][j]
 *   a  = ((max(|p0L|,|p0H|) + max(|p1L|,|p1H|)) + max(|p2L|,|p2H|)) + |M[3][j]|
 *   pad = a*eps                blo = mn - pad             bhi = mx + pad
 * Row i of out_bounds is the fold of blo (minimum) and bhi (maximum) over all table rows in the total order the deform bounds use
 * (-0 < +0), so it does not depend on any reduction order; each of the six components is then multiplied by pos_scale.  Layout
 * {min x, min y, min z, max x, max y, max z}, as mmdx_deform_batched_bounds writes and mmdx_cull_bounds reads.  If any blo or bhi of
 * an instance is NaN the whole row is six quiet NaNs, and so is every row when the table is empty: a broken palette stays visible
 * to the cull ("a NaN never culls").  Infinities go through the arithmetic as written (an infinite translation gives inf - inf).
 *
 * The guarantee.  If every applied weight of the model is >= 0 (n_nonconvex == 0; the call refuses other models), every slot weight
 * of instance i is <= morph_scale (slot weights are the morph rates times the group chains, mmdx_model_slot_weights; 0 when no morph
 * is in use) and the palette is finite, then row i contains every position mmdx_deform_batched* writes for instance i from the same
 * palette and pos_scale in the float32 layouts (MMDX_OUT_SOA, MMDX_OUT_VERTEX32), in the bit-exact and the fast-math build alike.
 * Limits: binary16 positions (MMDX_OUT_SOA_POS16) are rounded after the fact and can exceed the box by half a binary16 ulp -- give
 * mmdx_cull_view.margin that much.  The box is conservative, not tight: it is the union of the bones' transformed boxes (a rotated
 * box's box is larger than the rotated points' box, and a bone's box holds every vertex the bone touches at any weight), grown by
 * reach * morph_scale on every side whichever morphs are actually in use. */
typedef struct mmdx_bone_box_info {
    uint32_t struct_size, n_boxes, n_nonconvex, max_vertex_entries;
    float eps, weight_sum_dev;
    uint32_t reserved0[2];
} mmdx_bone_box_info;
/* Works on MMDX_CREATE_HOST_ONLY models.  bones [n_boxes] and boxes [n_boxes][9] = lo xyz, hi xyz, reach xyz may be NULL (call once
 * for n_boxes, then again with arrays). */
MMDX_API mmdx_status mmdx_model_get_bone_boxes(mmdx_model_t model, mmdx_bone_box_info *info, uint32_t *bones, float *boxes);

typedef struct mmdx_palette_bounds_args {
    uint32_t struct_size, flags;      /* MMDX_PALETTE_ON_DEVICE | MMDX_OUT_ON_DEVICE; any other bit is refused                  */
    uint32_t n_instances, reserved0;  /* reserved0 must be 0                                                                    */
    const float *palettes;            /* [NI][NB][16], 16-byte aligned on the device                                            */
    float *out_bounds;                /* [NI][6]                                                                                */
    float pos_scale;                  /* finite, > 0: the args.pos_scale of the deform it stands in for                         */
    float morph_scale;                /* finite, >= 0: upper bound of every slot weight; 0 = no morphs in use                   */
} mmdx_palette_bounds_args;
/* `model` supplies the table, the device and the stream: the call is asynchronous on it, in order with the model's solve, place,
 * cull and deform calls, and records into mmdx_graph_begin / _end (both operands in device memory then; a recorded call reads the
 * palettes afresh at every replay).
 *  - An operand without its *_ON_DEVICE flag is host memory, copied per call through scratch of the model in stream order, and the
 *    call returns when the work is done.
 *  - n_instances == 0 is MMDX_OK and launches nothing.  NULL model / args / pointers, a struct_size mismatch, an unknown flag bit,
 *    reserved0 != 0, a pos_scale that is not finite and > 0, a morph_scale that is not finite and >= 0, palettes overlapping
 *    out_bounds, device palettes that are not 16-byte aligned and a device out_bounds that is not 4-byte aligned are
 *    MMDX_ERR_INVALID_ARGUMENT.  Then a model with n_nonconvex > 0 is MMDX_ERR_UNSUPPORTED (the message names the count), and only
 *    then a MMDX_CREATE_HOST_ONLY model is MMDX_ERR_NO_DEVICE. */
MMDX_API mmdx_status mmdx_palette_bounds(mmdx_model_t model, const mmdx_palette_bounds_args *args);

/* The same with bone morphs applied first: morph_weights[i][n_morphs] (or one shared row with
 * MMDX_WEIGHTS_SHARED; device pointer with MMDX_WEIGHTS_ON_DEVICE) are the raw per-frame morph rates, the
 * ones mmdx_deform_batched takes.  Bone-morph rotations go through SLerp, i.e. through the device's double
 * acos / sin like the reference's through the host's.  NULL weights = mmdx_skeleton_solve. */
/* ---- the physics seam ---------------------------------------------------------------------------------
 * The reference's frame is PrePhysicsPosing -> PhysicsReactor::React -> PostPhysicsPosing (main.cpp:1801-1810):
 * after the pre-physics bone list the reactor (Bullet, on the host) overwrites the skinning matrix of every bone one
 * of its bodies moved (PoserMotionState::Synchronize, mmd-bullet_impl.inl:34-40) and re-derives local_matrix_ of
 * the "strict" ones from it -- keeping the bone's own translation -- before it recomputes their skinning matrix
 * (Fix, :42-56); the post-physics bones then hang off those local matrices.  Two calls reproduce that:
 *   mmdx_skeleton_solve_pre   reset + bone morphs + the pre-physics list; out_palettes rows of the pre-physics bones
 *                             are written (what the reactor's kinematic bodies read), the others are unspecified;
 *   (the host steps its physics)
 *   mmdx_skeleton_solve_post  Synchronize for all listed bones, then Fix for the strict ones in list order, then the
 *                             post-physics list; out_palettes (the SAME array the pre step wrote) receives the
 *                             overridden rows and the post-physics bones' rows.
 * The skeleton must have been created with MMDX_SKELETON_PHYSICS_SEAM; n_instances must match between the two
 * calls.  Fix uses Matrix4f::Inverse's Gauss-Jordan elimination step for step (L/util/math_impl.inl:822-897):
 * bit-exact against libmmd like the rest of the solve. */
typedef struct mmdx_physics_overrides {
    uint32_t struct_size;
    uint32_t n_bones;                         /* K bones physics moved (the same set for every instance)         */
    const int32_t *bone;                      /* [K] host                                                        */
    const uint8_t *strict;                    /* [K] host, non-zero: Fix() applies; NULL = none                  */
    const float *skinning;                    /* [NI][K][16] the bodies' transforms as skinning matrices; host, or
                                                 device with MMDX_OVERRIDES_ON_DEVICE                            */
} mmdx_physics_overrides;
enum { MMDX_OVERRIDES_ON_DEVICE = 1u << 5 };
MMDX_API mmdx_status mmdx_skeleton_solve_pre(mmdx_skeleton_t skeleton, mmdx_model_t model, uint32_t n_instances,
                                             const float *poses, const float *morph_weights, uint32_t flags,
                                             float *out_palettes);
MMDX_API mmdx_status mmdx_skeleton_solve_post(mmdx_skeleton_t skeleton, mmdx_model_t model, uint32_t n_instances,
                                              const mmdx_physics_overrides *overrides /* may be NULL */,
                                              uint32_t flags, float *out_palettes);
MMDX_API mmdx_status mmdx_skeleton_solve_morphed(mmdx_skeleton_t skeleton, mmdx_model_t model,
                                                 uint32_t n_instances, const float *poses,
                                                 const float *morph_weights, uint32_t flags,
                                                 float *out_palettes);
/* ---- solving a subset of a crowd: mmdx_skeleton_solve_morphed (mmdx_skeleton_solve when morph_weights == NULL) for the instances of
 * an mmdx_instance_select only -- the list type of mmdx_deform_batched_select, so mmdx_cull_bounds' out_ids / out_counts go in as they
 * are.  On rigs with CCD-IK the solve is the frame's largest step; this makes it scale with the instances in view.
 *  1. n_instances = NI is the extent of poses, morph_weights and out_palettes: instance i reads pose row i and rate row i (or the one
 *     shared row with MMDX_WEIGHTS_SHARED) and writes palette row i.  The list only says which i take part.
 *  2. For every listed i < NI the 64 * NB bytes of palette row i are identical to what mmdx_skeleton_solve_morphed writes for that
 *     instance from the same operands: the parallel-FK solver; the ordered solver with append bones, CCD-IK on one lane and on sixteen
 *     lanes per solve (MMDX_IK_COOP=0/1) and nested IK; its two-workgroups-per-CU variant; bone morphs, per instance and shared.
 *  3. Nothing else is written: palette rows of instances that are not listed keep every byte.  Pose and rate rows of unlisted
 *     instances may hold anything (NaN, uninitialised memory) and influence no written byte.
 *  4. The first min(*count, n_ids) ids are used.  *count == 0 or n_ids == 0 is a valid call that writes nothing.
 *  5. An id >= NI: in a host list the call fails with MMDX_ERR_INVALID_ARGUMENT before anything is launched; in a device list the
 *     entry is skipped on the device (nothing read or written for it).  An id that occurs twice is allowed and costs twice: the
 *     solver's per-bone state and the bone-morph state are kept per LIST POSITION, so both solves are independent and store the same
 *     bytes.  The skeleton's scratch is therefore sized by n_ids, not by NI.
 *  6. The device-resident form only: MMDX_POSES_ON_DEVICE | MMDX_OUT_ON_DEVICE are required, and MMDX_WEIGHTS_ON_DEVICE when
 *     morph_weights is given; anything else is MMDX_ERR_INVALID_ARGUMENT (the staging copies of host operands move whole arrays and
 *     cannot honour rule 3), as are unknown flag bits, select == NULL, a struct_size mismatch, unknown select->flags bits and
 *     reserved0 != 0 -- all of them, and NULL skeleton / poses / out_palettes and n_instances == 0, before the device is touched.  A
 *     host-resident list is supported: it is copied through a scratch buffer of the skeleton in stream order, and the call returns
 *     after its work has completed.
 *  7. With a device list the call is asynchronous on `model`'s stream (a borrowed stream applies; without a model, the selected
 *     device's default stream) and records into mmdx_graph_begin / mmdx_graph_end after one un-recorded run; a host list is refused
 *     while recording.  A replay reads ids and *count afresh.  The skeleton's scratch is pinned by the graph like that of the other
 *     solves: a later call whose n_ids would make it grow fails with MMDX_ERR_INVALID_ARGUMENT.  ids and count are 4-byte aligned.
 *  8. The launches are sized from n_ids: workgroups whose list positions all lie behind *count return at once.
 *  9. Only the one-step solve has a select form, the physics seam (_pre / _post) has none.  On a MMDX_SKELETON_PHYSICS_SEAM skeleton
 *     the call behaves toward a pending pre step exactly as mmdx_skeleton_solve does: the pre step is void.
 * 10. Track evaluation has a select form of its own that takes the same list: mmdx_motion_set_blend_bones_time_select writes the
 *     listed rows of `poses`, and mmdx_skeleton_solve_motion_set_blend_time_select (below) is tracks and solve in one call.  An
 *     instance that is not solved keeps its last model-space palette. */
MMDX_API mmdx_status mmdx_skeleton_solve_select(mmdx_skeleton_t skeleton, mmdx_model_t model, uint32_t n_instances, const float *poses,
                                                const float *morph_weights /* or NULL */, uint32_t flags,
                                                const mmdx_instance_select *select, float *out_palettes /* [NI][NB][16] */);
/* ---- evaluating the motion tracks of a subset of a crowd: the three cross-fade calls (mmdx_motion_set_blend_bones_time,
 * mmdx_motion_set_blend_morphs_time, mmdx_skeleton_solve_motion_set_blend_time) for the instances of an mmdx_instance_select only.  The
 * tracks are a pure function of the clocks, and the clocks stay with mmdx_animator_advance, which runs for everyone: an instance that
 * comes back into view is evaluated at its current time and nothing was skipped.  With this the frame costs what is in view from its
 * first evaluation on.
 *  1. args->n_instances = NI is the extent of the five operand arrays and of the output: instance i reads operand row i and writes
 *     output row i.  The list only says which i take part.
 *  2. For every listed i < NI the bytes of output row i are identical to what the plain call writes for that instance from the same
 *     operands: every weight class (A, B, mix, NaN), MMDX_CLIP_NONE and device ids >= n_clips.  An end-point row still reads nothing
 *     of the other clip.
 *  3. Nothing else is written: output rows of instances that are not listed keep every byte.  Operand rows of unlisted instances may
 *     hold anything (clip ids out of range, NaN times, NaN weights, uninitialised memory) and influence no written byte.
 *  4. The first min(*count, n_ids) ids are used.  *count == 0 or n_ids == 0 is a valid call that writes nothing.
 *  5. An id >= NI: in a host list the call fails with MMDX_ERR_INVALID_ARGUMENT before anything is launched; in a device list the
 *     entry is skipped on the device (nothing read or written for it).  An id that occurs twice is allowed and costs twice; both
 *     writers store the same bytes.  Output rows are addressed by id: these calls keep no state per list position.
 *  6. The device-resident form only: MMDX_TIMES_ON_DEVICE | MMDX_OUT_ON_DEVICE are required (the staging copies of host operands move
 *     whole arrays and cannot honour rule 3).  Anything else is MMDX_ERR_INVALID_ARGUMENT, as are unknown flag bits, select == NULL, a
 *     struct_size mismatch of either structure, unknown select->flags bits, reserved0 != 0, NULL handles or arrays, n_instances == 0,
 *     a set created without the side asked for and a bone count of the set that is not the skeleton's -- all of them before the
 *     device is touched.  A host-resident list is supported: it is copied through a scratch buffer of the set (on the ordered path of
 *     the palette call, of the skeleton as well) in stream order, count word first, and the call returns after its work has completed.
 *  7. With a device list the call is asynchronous on `model`'s stream (a borrowed stream applies; without a model, the selected
 *     device's default stream) and records into mmdx_graph_begin / mmdx_graph_end after one un-recorded run; a host list is refused
 *     while recording.  A replay reads ids, *count and the operands afresh.  Pinning as for the calls it is made of: the set's tables
 *     and scratch, and the skeleton's for the palette call.  ids and count are 4-byte aligned.
 *  8. The launches are sized from n_ids: workgroups whose list positions all lie behind *count return at once.
 *  9. The palette call is one launch on a parallel-FK skeleton of up to 2 048 bones (a workgroup per list position).  Otherwise (append
 *     bones / IK, or larger) the blend select goes into the set's pose scratch -- [NI] rows addressed by id, sized and pinned as for
 *     the plain call -- and mmdx_skeleton_solve_select runs with the same list; the skeleton's scratch is then sized by n_ids, as
 *     stated there.  On either path the skeleton's record of its last solve (mmdx_bench.h) is set as the plain call sets it.
 * 10. mmdx_animator_advance has no select form on purpose: clocks run for everyone.  The frame and single-motion clocks, the
 *     non-blend set calls and the physics seam get no select form either; a weight of 0 gives the set call's row, every bit. */
MMDX_API mmdx_status mmdx_motion_set_blend_bones_time_select(mmdx_motion_set_t set, mmdx_model_t model, const mmdx_motion_blend_args *args,
                                                             const mmdx_instance_select *select,
                                                             float *out_poses /* [NI][NB][MMDX_POSE_FLOATS] */);
MMDX_API mmdx_status mmdx_motion_set_blend_morphs_time_select(mmdx_motion_set_t set, mmdx_model_t model, const mmdx_motion_blend_args *args,
                                                              const mmdx_instance_select *select, float *out_weights /* [NI][NM] */);
MMDX_API mmdx_status mmdx_skeleton_solve_motion_set_blend_time_select(mmdx_skeleton_t skeleton, mmdx_motion_set_t set, mmdx_model_t model,
                                                                      const mmdx_motion_blend_args *args,
                                                                      const mmdx_instance_select *select,
                                                                      float *out_palettes /* [NI][NB][16] */);

/* ---- Layers: the masked blend of two evaluated pose or rate arrays, per bone / per morph ------------------------------------------
 * The cross-fade above applies one weight to a whole row.  A layer -- the upper body waves while the legs keep walking, the face
 * follows a talk clip while the body dances -- needs a weight per bone.  mmdx_pose_blend takes two pose arrays A and B
 * [NI][row_items][MMDX_POSE_FLOATS] that any track call wrote (a cross-fading base from one animator, a layer from another), a weight
 * per instance and a mask row per instance, and writes per item the cross-fade's blend at the effective weight weight x mask[item];
 * mmdx_rate_blend does the same for two morph-rate arrays [NI][row_items].  The result goes to mmdx_skeleton_solve / _solve_select
 * (and the deform) as poses and rates always did; calling again with a third array gives a third layer.
 *
 * For instance i and item j, with m = mask_ids ? mask_ids[i] : MMDX_MASK_NONE:
 *   mask value         mv = 1.0f for m == MMDX_MASK_NONE, masks[m][j] for m < n_masks, 0.0f for any other device id (the row is A)
 *   effective weight   e = weights[i] * mv, one binary32 multiply: without a mask e is exactly weights[i]
 *   !(e >= 1e-7f)      item j of out is A's item, every bit (the fourth translation float and NaNs copied as they are); B's item is
 *                      not read
 *   e > 1.0f - 1e-7f   item j is B's item, every bit; A's item is not read (with out == a it is simply overwritten)
 *   otherwise          the cross-fade's arithmetic above (translation, rotation, morph rate) with w = e, unfused; fourth translation
 *                      float 0.  Bit-identical to libmmd's operations; only the sign and payload of a NaN in a mixed item are not
 *                      part of the contract.
 * Two consequences callers may rely on:
 *  - B MAY BE UNINITIALISED WHERE IT IS NOT NEEDED: rows of B whose instance has weights[i] == 0 (or a device NaN weight), and items
 *    whose mask value is 0, may hold anything and influence no written byte.  The layer's tracks can therefore be evaluated with the
 *    *_select track calls for the instances that wear the layer only.
 *  - THE NO-MASK CALL EQUALS THE SET'S BLEND: with mask_ids == NULL, A the rows mmdx_motion_set_eval_bones_time writes for (clips_a,
 *    times_a) and B those for (clips_b, times_b), mmdx_pose_blend writes bit for bit what mmdx_motion_set_blend_bones_time writes for
 *    the same operands; the same holds for mmdx_rate_blend against mmdx_motion_set_blend_morphs_time.
 * `model` supplies the device, the stream, graph recording and the scratch of host operands, as for mmdx_palette_place; row_items is
 * explicit and need not be the model's bone or morph count.  The call is asynchronous on the model's stream and records into
 * mmdx_graph_begin / _end (every operand in device memory then; a replay reads a, b, weights, mask_ids, masks and the list afresh).
 *  - In place: out == a and out == b are both allowed, a lane reads its own items of A and B before it stores.  Any other overlap
 *    among a, b and out (a overlapping b included), and weights, mask_ids or masks overlapping out, are MMDX_ERR_INVALID_ARGUMENT.
 *    With out == a, a row whose weight is 0 or NaN already holds its result and is not touched at all: a crowd in which few instances
 *    wear a layer pays for those instances only.
 *  - select (NULL = every instance) follows mmdx_instance_select as mmdx_deform_batched_select states it: the first min(*count, n_ids)
 *    ids are used; a device id >= NI is skipped, a host id >= NI fails before anything is launched; an id listed twice costs twice
 *    and stores the same bytes (with a separate out; in place list an id once, a second blend of the row would start from what the
 *    first one wrote); no byte of a row that is not listed is written, and its operand rows may hold anything; a host list
 *    is copied through scratch of the model and refused while a graph is being recorded.  With a list, a, b and out must be device
 *    memory (the staging copies of host rows move whole arrays): anything else is MMDX_ERR_INVALID_ARGUMENT.
 *  - An operand without its *_ON_DEVICE flag is host memory, copied per call through scratch of the model, and the call returns when
 *    the work is done.  Host operands are checked before the first HIP call: a mask id >= n_masks other than MMDX_MASK_NONE is
 *    MMDX_ERR_BAD_INDEX, a NaN weight or mask value MMDX_ERR_INVALID_ARGUMENT; any other host mask value (negative, above 1) is used
 *    as given, like a device one.
 *  - Device pose arrays must be 16-byte aligned; device rate arrays, weights, mask_ids and masks 4-byte aligned.
 *  - n_instances == 0 or row_items == 0 is MMDX_OK and launches nothing.  NULL model / args / a / b / weights / out, masks == NULL
 *    with mask_ids and n_masks > 0, a struct_size mismatch of either structure, an unknown flag bit and reserved0 != 0 are
 *    MMDX_ERR_INVALID_ARGUMENT; a MMDX_CREATE_HOST_ONLY model is MMDX_ERR_NO_DEVICE (after validation).  Models created with
 *    MMDX_CREATE_FAST_MATH run the same, uncontracted kernels. */
#define MMDX_MASK_NONE 0xFFFFFFFFu            /* no mask: every item's mask value is 1.0f */
enum {
    MMDX_BLEND_A_ON_DEVICE = 1u << 11,        /* a is a device pointer (else host, copied per call)                                */
    MMDX_BLEND_B_ON_DEVICE = 1u << 12,        /* b is a device pointer                                                             */
    MMDX_BLEND_PARAMS_ON_DEVICE = 1u << 13    /* weights, mask_ids and masks are device pointers, read when the kernel RUNS        */
};
typedef struct mmdx_row_blend_args {
    uint32_t struct_size, flags;        /* = sizeof(mmdx_row_blend_args); the three above | MMDX_OUT_ON_DEVICE, any other bit:
                                           MMDX_ERR_INVALID_ARGUMENT                                                               */
    uint32_t n_instances, row_items;    /* NI; NB (poses) or NM (rates)                                                            */
    const float *a, *b;                 /* poses [NI][row_items][MMDX_POSE_FLOATS]; rates [NI][row_items]                          */
    const float *weights;               /* [NI]                                                                                    */
    const uint32_t *mask_ids;           /* [NI] or NULL = MMDX_MASK_NONE for everyone                                              */
    const float *masks;                 /* [n_masks][row_items]; may be NULL when n_masks == 0                                     */
    uint32_t n_masks, reserved0;        /* reserved0 must be 0                                                                     */
    float *out;                         /* same shape as a; may be == a or == b                                                    */
} mmdx_row_blend_args;
MMDX_API mmdx_status mmdx_pose_blend(mmdx_model_t model, const mmdx_row_blend_args *args,
                                     const mmdx_instance_select *select /* NULL = every instance */);
MMDX_API mmdx_status mmdx_rate_blend(mmdx_model_t model, const mmdx_row_blend_args *args,
                                     const mmdx_instance_select *select /* NULL = every instance */);

/* ---- Additive layers: a clip's offset from its reference pose, added per bone / per morph ------------------------------------------
 * The layer call above replaces: at effective weight e a bone moves from A's pose towards B's.  Breathing, a recoil, a lean into a
 * turn, a nod, "a bit more smile" add instead: the difference between a clip and that clip's reference pose goes on top of whatever
 * the base does, possibly exaggerated.  mmdx_pose_add takes the base rows A, the layer rows B and a bank of reference rows
 * refs[n_refs][row_items][MMDX_POSE_FLOATS] (one row per additive clip, chosen per instance by ref_ids), all of them rows that any
 * track call wrote, and writes A with B's difference from the reference applied at the effective weight, the way libmmd applies a
 * bone morph; mmdx_rate_add does the same for morph rates [NI][row_items] with refs[n_refs][row_items].  The reference rows need no
 * call of their own: mmdx_motion_set_eval_bones_time with n_instances = n_clips, clips[i] = i, times[i] = 0 writes refs in exactly
 * this layout (the same with _eval_morphs_time for rates).
 *
 * For instance i and item j (Quaternion and Vector3 operators as libmmd's: L/util/math_impl.inl, L/motion/poser_impl.inl):
 *  1. effective weight   e = weights[i] * mv, mv exactly as the layers block above defines it (MMDX_MASK_NONE, masks[m][j], or 0 for
 *                        any other device id): one binary32 multiply.
 *  2. reference id       r = ref_ids ? ref_ids[i] : MMDX_REF_NONE.  A device r >= n_refs other than MMDX_REF_NONE makes the whole
 *                        row A; a host one is MMDX_ERR_BAD_INDEX.
 *  3. !(e >= 1e-7f)      item j of out is A's item, every bit (the fourth translation float and NaNs as they are); neither B's item
 *                        nor the reference's is read.  This is the bone-morph walk's `rate < 1e-7f` skip (poser_impl.inl:347-353),
 *                        closed over NaN the way the layers block closes its own.
 *  4. no upper short circuit: e is used as given; e == 1 adds the whole difference, e > 1 exaggerates it.  Masks above 1 and weights
 *                        above 1 are legal in host and device memory.
 *  5. the difference     r == MMDX_REF_NONE: B's item is the difference (d.q = B.q, d.t = B.t), no arithmetic is done on it.
 *                        With R = refs[r][j]: d.q = B.q * R.q.Inverse() (operator*, Inverse, math_impl.inl:474-477, 510-517: the way
 *                        the CCD loop extracts a delta, poser_impl.inl:290), d.t = B.t - R.t per channel.
 *  6. applying it        unfused, in this order: mt = 0.0f + d.t * e per channel; mq = Identity * SLerp(Identity, d.q)[e]
 *                        (math_impl.inl:1312-1337); out.q = mq * A.q; out.t = mt + A.t; the fourth translation float is 0.
 *  7. the identity steps 0.0f + and Identity * are kept: they make the item bit for bit what Poser::UpdateMorphTransform
 *                        (poser_impl.inl:347-353) followed by UpdateBoneTransform (:144-145, morph_rotation_ * rotation_ and
 *                        morph_translation_ + translation_) computes for a bone whose morph_* received exactly one application
 *                        (d.t, d.q) at rate e.  Hence: mmdx_pose_add with B the (translation, rotation) rows of a bone morph, no
 *                        reference and the morph's rate as weight, followed by mmdx_skeleton_solve, gives the palettes of
 *                        mmdx_skeleton_solve_morphed, value for value (-0 may come out as +0, nothing else differs).
 *  8. quaternions        are never normalised.  A d.q whose |comega| exceeds 1 makes acos NaN; omega > 1e-7f is then false and
 *                        SLerp returns Identity, as in libmmd.  acos and sin go through double, as in the bone morphs.
 *  9. rates              d = (r == MMDX_REF_NONE) ? b : b - ref, then out = a + d * e (vertex_image + offset * rate,
 *                        poser_impl.inl:344), unfused.
 * Only the sign and payload of a NaN in a mixed item are not part of the contract.  Negative effective weights are A by rule 3:
 * there are no subtracting layers.
 *
 * Everything else is the layers contract above, word for word: `model`, the stream, graph recording (a replay reads a, b, weights,
 * mask_ids, masks, ref_ids, refs and the list afresh), select, host operands and their checks, zero sizes, refusals, HOST_ONLY
 * models, FAST_MATH models running the same uncontracted kernels.  The flags are the blend's; MMDX_BLEND_PARAMS_ON_DEVICE covers
 * ref_ids and refs as well.  In addition:
 *  - In place: out == a and out == b are both allowed, a lane reads its items of A, B and R before it stores; a overlapping b, and
 *    any other overlap among a, b and out, are MMDX_ERR_INVALID_ARGUMENT, and so is ref_ids or refs overlapping out.  With out == a
 *    a row whose weight is 0 or NaN is not touched, its workgroup returns after reading the weight; items that stay A are neither
 *    loaded nor stored.
 *  - B AND THE REFERENCE MAY BE UNINITIALISED wherever e fails the test of rule 3 (and B in rows whose device reference id is out of
 *    range).
 *  - ref_ids == NULL means MMDX_REF_NONE for everyone and refs / n_refs are ignored; refs == NULL with ref_ids and n_refs > 0 is
 *    MMDX_ERR_INVALID_ARGUMENT.  Host ref ids are checked before the first HIP call; host refs are not inspected.
 *  - Device refs of mmdx_pose_add must be 16-byte aligned; device refs of mmdx_rate_add and device ref_ids 4-byte aligned.
 *  - reserved0 and reserved1 must be 0. */
#define MMDX_REF_NONE 0xFFFFFFFFu             /* no reference: B already is a difference */
typedef struct mmdx_row_add_args {
    uint32_t struct_size, flags;        /* = sizeof(mmdx_row_add_args); MMDX_BLEND_A_ON_DEVICE | _B_ | _PARAMS_ | MMDX_OUT_ON_DEVICE,
                                           any other bit: MMDX_ERR_INVALID_ARGUMENT                                                */
    uint32_t n_instances, row_items;    /* NI; NB (poses) or NM (rates)                                                            */
    const float *a, *b;                 /* poses [NI][row_items][MMDX_POSE_FLOATS]; rates [NI][row_items]                          */
    const float *weights;               /* [NI]                                                                                    */
    const uint32_t *mask_ids;           /* [NI] or NULL = MMDX_MASK_NONE for everyone                                              */
    const float *masks;                 /* [n_masks][row_items]; may be NULL when n_masks == 0                                     */
    uint32_t n_masks, reserved0;        /* reserved0 must be 0                                                                     */
    float *out;                         /* same shape as a; may be == a or == b                                                    */
    const uint32_t *ref_ids;            /* [NI] or NULL = MMDX_REF_NONE for everyone                                               */
    const float *refs;                  /* poses [n_refs][row_items][MMDX_POSE_FLOATS]; rates [n_refs][row_items]                  */
    uint32_t n_refs, reserved1;         /* reserved1 must be 0                                                                     */
} mmdx_row_add_args;
MMDX_API mmdx_status mmdx_pose_add(mmdx_model_t model, const mmdx_row_add_args *args,
                                   const mmdx_instance_select *select /* NULL = every instance */);
MMDX_API mmdx_status mmdx_rate_add(mmdx_model_t model, const mmdx_row_add_args *args,
                                   const mmdx_instance_select *select /* NULL = every instance */);
/* A mask row from the hierarchy, on the host (no device needed): out_mask[b] = inside when b or any ancestor of b is in roots, else
 * outside.  Ancestors are followed through the parent array the skeleton was created from, as mmdx_skeleton_desc.parent defines it: a
 * parent outside [0, NB) ends the chain, which is followed for at most NB steps.  n_roots == 0 fills `outside`; a root >= NB is
 * MMDX_ERR_BAD_INDEX (nothing is written); NULL skeleton / out_mask, and NULL roots with n_roots > 0, are MMDX_ERR_INVALID_ARGUMENT. */
MMDX_API mmdx_status mmdx_skeleton_subtree_mask(mmdx_skeleton_t skeleton, uint32_t n_roots, const uint32_t *roots, float inside,
                                                float outside, float *out_mask /* [NB] host */);
MMDX_API void mmdx_skeleton_destroy(mmdx_skeleton_t skeleton);
/* Fills `desc` with pointers into `pmx` (valid until mmdx_pmx_destroy): rest positions, parents, transform
 * levels, flag words, append and IK tables exactly as the file states them (PmxReader,
 * L/reader/pmx_reader_impl.inl:192-264), ready for mmdx_skeleton_create(). */
MMDX_API mmdx_status mmdx_pmx_get_skeleton_desc(mmdx_pmx_t pmx, mmdx_skeleton_desc *desc);

#ifdef __cplusplus
}
#endif
#endif /* MMDX_H_INCLUDED */

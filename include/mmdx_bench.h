/* mmdx_bench.h -- measurement and A/B entry points of libmmdx.so.
 *
 * NOT part of the drop-in boundary (include/mmdx.h): nothing in the reference corresponds to these.  They exist
 * for bench.py, tools/ and the GPU tests: HIP-event timers on a model's stream, per-kernel profiling of
 * mmdx_deform_batched, the streaming copy / fill / store-pattern ceilings printed next to the roofline
 * (SURVEY.md section 8d), the re-read of the launch-shape override environment and the records of the last launch shape and the last solve shape.  Same
 * library, same status codes.
 */
#ifndef MMDX_BENCH_H_INCLUDED
#define MMDX_BENCH_H_INCLUDED

#include "mmdx.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- timing on the handle's stream (HIP events; for bench harnesses) ------------------------- */
MMDX_API mmdx_status mmdx_timer_start(mmdx_model_t model);
MMDX_API mmdx_status mmdx_timer_stop(mmdx_model_t model, float *elapsed_ms); /* syncs the stream  */
/* Per-kernel timing with no host synchronisation: while enabled, mmdx_deform_batched records HIP events on
 * the launch stream around its morph kernels and around its skinning kernel -- on every call (enabled == 1)
 * or on every N-th call (enabled == N > 1): the four event records cost the stream about 7 us per call, which a
 * throughput measurement should not pay on every step.  (Timing the skinning kernel alone is not offered: its
 * start event must follow another event record, or it is stamped with the end of the previous KERNEL and the
 * interval then includes the launch gap.)  mmdx_profile_collect waits for the recorded calls, returns how
 * many were timed and the summed milliseconds of the skinning kernel and of the morph pass, and resets
 * the recording. */
MMDX_API mmdx_status mmdx_profile_enable(mmdx_model_t model, int32_t enabled);
MMDX_API mmdx_status mmdx_profile_collect(mmdx_model_t model, uint32_t *n_calls, float *skin_ms_total,
                                          float *morph_ms_total);

/* The launch-shape overrides for A/B runs (environment variables MMDX_GROUP, MMDX_THREADS, MMDX_LDS_TARGET,
 * MMDX_INTERLEAVE; tools/ab.py) are read once per process; this re-reads them.  Not for product use. */
MMDX_API void mmdx_debug_reload_env(void);
/* Which store flavour the kernel of the model's last mmdx_deform_batched call ran with: 0 = cached non-temporal stores, 1 =
 * write-through (mmdx.h, MMDX_OUT_STORES_*; 1 only where the launched kernel has that flavour). */
MMDX_API mmdx_status mmdx_debug_last_store_policy(mmdx_model_t model, int32_t *write_through);
/* The launch shape of the model's last successfully planned mmdx_deform_batched* call, as handed to the kernel: tests read it to
 * prove that they ran the instantiation and the instances-per-workgroup they claim (small crowds plan group == 1 on their own;
 * MMDX_GROUP forces more).  Read-only host state: nothing here reaches a kernel. */
typedef enum mmdx_debug_kernel {
    MMDX_DEBUG_KERNEL_NONE = 0,      /* no call yet, or a select call with an empty list */
    MMDX_DEBUG_KERNEL_DEFORM = 1,    /* the tile kernel (deform_kernel) */
    MMDX_DEBUG_KERNEL_PACK = 2,      /* MMDX_FUSED_PACK=1 */
    MMDX_DEBUG_KERNEL_FRAME = 3,     /* one frame of one model, latency-ordered */
    MMDX_DEBUG_KERNEL_CULL = 4,      /* mmdx_cull_bounds was the model's last planned call: threads = lanes per workgroup, group =
                                        instances per chunk, ngroups = chunks, select = the form (1: one workgroup walks the chunks,
                                        2: a count launch and a scatter launch, one workgroup per chunk); every other field 0 */
    MMDX_DEBUG_KERNEL_AIM = 5,       /* mmdx_palette_aim on this model's stream was its last planned call: threads = lanes per
                                        workgroup, group = instances (list positions) per workgroup, 16, or 64 under
                                        MMDX_AIM_BLOCK=64, ngroups = workgroups per aim, lds = bytes of dynamic LDS, select = 1 with a list;
                                        every other field 0 */
    MMDX_DEBUG_KERNEL_REACH = 6      /* mmdx_palette_reach likewise: group = 16, ngroups = workgroups per reach */
} mmdx_debug_kernel;
typedef struct mmdx_debug_launch_shape {
    uint32_t struct_size;            /* sizeof(mmdx_debug_launch_shape), set by the caller */
    uint32_t kernel;                 /* mmdx_debug_kernel */
    uint32_t threads;                /* lanes per workgroup */
    uint32_t group;                  /* instances per workgroup */
    uint32_t ngroups;                /* workgroups per tile: ceil(n_instances / group), of a select call ceil(n_ids / group);
                                        0 for the frame kernel and when nothing was launched */
    uint32_t lds;                    /* bytes of dynamic LDS */
    uint32_t morph;                  /* 0 no morphs, 1 shared (separate morph pass), 2 shared (gathered in the kernel),
                                        3 per-instance weights */
    uint32_t layout;                 /* MMDX_OUT_* */
    uint32_t f16, tile_order;        /* the model's MMDX_CREATE_F16_POSITIONS / MMDX_CREATE_TILE_ORDER */
    uint32_t bounds, select;         /* the flavour of mmdx_deform_batched_bounds / _select */
    uint32_t write_through;          /* as mmdx_debug_last_store_policy */
    uint32_t interleave;             /* MMDX_INTERLEAVE as the kernel received it: instances dealt g * ngroups + grp (1) or
                                        grp * group + g (0); read by the shared-rate and no-morph modes only */
    uint32_t sel_interleave;         /* MMDX_SELECT_INTERLEAVE likewise, of a select call (0 otherwise) */
    uint32_t reserved0;
} mmdx_debug_launch_shape;
MMDX_API mmdx_status mmdx_debug_last_launch_shape(mmdx_model_t model, mmdx_debug_launch_shape *out);
/* What the skeleton's last successful solve launched (mmdx_skeleton_solve and every call that ends in it, _solve_morphed, _solve_pre,
 * _solve_post, _solve_select, _solve_motion*): tests read it to prove which compilation of the ordered bone solver they ran -- the
 * two-workgroups-per-CU one (`dense`) is chosen by crowd size on its own (more workgroups than the device has CUs) and forced or
 * forbidden by MMDX_SOLVE_DENSE=1 / 0, read per call.  Read-only host state: nothing here reaches a kernel.  A select call with an
 * empty list launches nothing and leaves the record as it was. */
typedef enum mmdx_debug_solver {
    MMDX_DEBUG_SOLVER_NONE = 0,        /* no solve yet */
    MMDX_DEBUG_SOLVER_ORDERED = 1,     /* the ordered solver (append bones, IK, physics seam): the fields below describe it */
    MMDX_DEBUG_SOLVER_PARALLEL_FK = 2  /* parallel FK (also fused with the motion evaluation): every field below is 0 */
} mmdx_debug_solver;
typedef struct mmdx_debug_solve_shape {
    uint32_t struct_size;            /* sizeof(mmdx_debug_solve_shape), set by the caller */
    uint32_t solver;                 /* mmdx_debug_solver */
    uint32_t nested;                 /* the nested-IK compilation (never dense) */
    uint32_t dense;                  /* the two-workgroups-per-CU compilation */
    uint32_t select;                 /* the select form (mmdx_skeleton_solve_select) */
    uint32_t workgroups;             /* of each ordered-segment launch: ceil(state cells / 16); the cells are the instances, of a
                                        select call the list's capacity (device list) or its ids in use (host list) */
    uint32_t lds;                    /* bytes of dynamic LDS of those launches */
    uint32_t segments;               /* ordered-segment launches of the call (1 unless ik_coop rounds cut the schedule) */
    uint32_t coop_launches;          /* ik_coop launches of the call (0 under MMDX_IK_COOP=0, on nested rigs, without window chains) */
    uint32_t reserved0;
} mmdx_debug_solve_shape;
MMDX_API mmdx_status mmdx_debug_last_solve_shape(mmdx_skeleton_t skeleton, mmdx_debug_solve_shape *out);
/* What became of the model's shared morph passes so far (mmdx.h, MMDX_MORPH_UNCHANGED): launches that walked the morph table,
 * launches whose device-side comparison found the rates unchanged and skipped the walk, and calls whose host-side comparison
 * skipped the launch altogether.  Waits for the model's stream. */
MMDX_API mmdx_status mmdx_debug_morph_pass_stats(mmdx_model_t model, uint32_t *walks, uint32_t *device_skips,
                                                 uint32_t *host_skips);
/* The revision of the sources this library was built from: SHA-1 over the translation units and headers of build.py's list,
 * in that order, embedded at build time (-DMMDX_SOURCE_SHA).  bench.py and smoke() print it next to the same hash of the files
 * in the tree and refuse to run when they differ: a timed library is provably the committed code. */
MMDX_API const char *mmdx_build_source_sha(void);
/* Device-to-device streaming copy / fill timed with HIP events: the practical HBM ceiling printed
 * next to the roofline.  bytes_moved = 2*bytes for copy, bytes for fill. */
MMDX_API mmdx_status mmdx_bench_copy(void *dst_device, const void *src_device, size_t bytes,
                                     int32_t iterations, float *avg_ms);
MMDX_API mmdx_status mmdx_bench_fill(void *dst_device, size_t bytes, int32_t iterations,
                                     float *avg_ms);
/* Store-only replay of the crowd kernel's SoA output pattern (two arrays of n_instances x
 * n_vertices x 12 bytes, 6 KiB pieces): the write ceiling of THAT pattern on this box. */
MMDX_API mmdx_status mmdx_bench_store_pattern(void *out_a_device, void *out_b_device,
                                              uint32_t n_vertices, uint32_t n_instances,
                                              int32_t iterations, float *avg_ms);

#ifdef __cplusplus
}
#endif
#endif /* MMDX_BENCH_H_INCLUDED */

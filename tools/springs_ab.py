#!/usr/bin/env python3
"""Interleaved A/B of mmdx_spring_step against the blend solve it follows, a device-to-device copy of the bytes it moves and the
existing physics seam writing the same rows from device overrides, in ONE process, median of R rounds.

    timeout -k 10 600 python tools/springs_ab.py            (AB_ROUNDS=7 AB_ITERS=200)

Shapes: 1 024 and 16 384 instances x 300 bones, 12 chains x 8 joints, 4 colliders, every operand in HBM.  Rows, in microseconds per
call:
    springs     AB_ITERS back-to-back mmdx_spring_step calls (device dt) between two synchronisations of the model's stream, host
                clock, so launch overhead is included; and the same by HIP events (mmdx_timer_*); plain and through a device list
                of every instance
    solve       mmdx_skeleton_solve_motion_set_blend_time on the same crowd (two clips over the 300 bones), host clock
    copy        mmdx_bench_copy over the bytes the step moves: per instance 96 joint rows written, 12 anchor and 4 collider rows
                read (64 bytes each) and 96 x 24 bytes of state read and written, HIP events
    seam        mmdx_skeleton_solve_pre + mmdx_skeleton_solve_post with the same 96 rows as device overrides on a skeleton created
                with MMDX_SKELETON_PHYSICS_SEAM, and mmdx_skeleton_solve_pre alone, host clock: post = the difference.  The post
                call uploads its bone list and synchronises the stream every time, and cannot be recorded.
The ratios springs / solve, springs / copy and springs / post are printed below the table.  Nothing here is a pass / fail number."""
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from simple_mmd_renderer_amd import _capi as api  # noqa: E402
from simple_mmd_renderer_amd import synth, vmd  # noqa: E402
from simple_mmd_renderer_amd.engine import DeformModel, DeviceBuffer, SpringSet  # noqa: E402

NB, N_CHAINS, N_JOINTS, N_COLLIDERS = 300, 12, 8, 4
BODY = NB - N_CHAINS * N_JOINTS


def make_rig(rng):
    """300 bones: a body of 204 (a binary tree below bone 0), then 12 chains of 8 hanging off bones 1..12."""
    parent = [-1] + [(b - 1) // 2 for b in range(1, BODY)]
    rest = [[0.0, 10.0, 0.0]] + [None] * (BODY - 1)
    for b in range(1, BODY):
        rest[b] = (np.array(rest[parent[b]]) + rng.uniform(-0.5, 0.5, 3)).tolist()
    chains = []
    for c in range(N_CHAINS):
        at, pos, chain = 1 + c, np.array(rest[1 + c]), []
        for _ in range(N_JOINTS):
            pos = pos + np.array([0.0, -0.3, 0.05]) + rng.uniform(-0.05, 0.05, 3)
            parent.append(at)
            rest.append(pos.tolist())
            at = len(parent) - 1
            chain.append(at)
        chains.append(chain)
    return np.array(parent, np.int32), np.array(rest, np.float32), chains


def main():
    rounds, iters = int(os.environ.get("AB_ROUNDS", "7")), int(os.environ.get("AB_ITERS", "200"))
    rng = np.random.default_rng(2032)
    parent, rest, chains = make_rig(rng)
    names = [f"bone{i}" for i in range(NB)]
    dm = DeformModel(synth.make_model(64, NB, 0, 0, seed=3))
    vs = [vmd.Vmd(vmd.write_vmd(synth.make_bone_keys(names[:BODY], 70 + k, keys_per=4, span=120), [])) for k in range(2)]
    bms = [v.bind_bones(names) for v in vs]
    ms = vmd.MotionSet(bms)
    sk = vmd.Skeleton(rest, parent)
    seam = vmd.Skeleton(rest, parent, physics_seam=True)
    joints = np.array([b for c in chains for b in c], np.int32)
    colliders = (np.arange(N_COLLIDERS, dtype=np.uint32), np.concatenate([rest[:N_COLLIDERS], np.full((N_COLLIDERS, 1), 0.4, np.float32)], axis=1))
    med = lambda x: float(np.median(x))                # noqa: E731
    for ni in (1024, 16384):
        sset = SpringSet(sk, chains, [20.0, 0.2, 1.0, 0.05], ni, colliders=colliders)
        d_pal, d_seam = DeviceBuffer(ni * NB * 64), DeviceBuffer(ni * NB * 64)
        d_ca, d_cb = DeviceBuffer.from_numpy((np.arange(ni) % 2).astype(np.uint32)), DeviceBuffer.from_numpy(((np.arange(ni) + 1) % 2).astype(np.uint32))
        d_ta, d_tb = DeviceBuffer.from_numpy(rng.uniform(0, 3, ni)), DeviceBuffer.from_numpy(rng.uniform(0, 3, ni))
        d_w = DeviceBuffer.from_numpy(rng.uniform(0, 1, ni).astype(np.float32))
        d_dt = DeviceBuffer.from_numpy(np.array([1 / 60], np.float32))
        d_ids = DeviceBuffer.from_numpy(np.arange(ni, dtype=np.uint32))
        sel = vmd.instance_select(d_ids.ptr, ni)
        moved = ni * ((N_CHAINS * N_JOINTS + N_CHAINS + N_COLLIDERS) * 64 + 2 * N_CHAINS * N_JOINTS * 24) // 2
        d_src, d_dst = DeviceBuffer(moved), DeviceBuffer(moved)
        solve = lambda out=d_pal: sk.solve_motion_set_blend_time_device(ms, ni, d_ca.ptr, d_ta.ptr, d_cb.ptr, d_tb.ptr, d_w.ptr, out.ptr, dm)  # noqa: E731
        solve()
        dm.sync()
        # the seam's operands: poses of the same crowd and the 96 override rows per instance, in device memory
        poses = np.zeros((ni, NB, 8), np.float32)
        poses[:, :, 7] = 1.0
        d_poses = DeviceBuffer.from_numpy(poses)
        d_over = DeviceBuffer.from_numpy(np.ascontiguousarray(d_pal.download((ni, NB, 16), np.float32)[:, joints]))
        strict = np.zeros(joints.size, np.uint8)
        ov = vmd.PhysicsOverrides(C.sizeof(vmd.PhysicsOverrides), joints.size, joints.ctypes.data, strict.ctypes.data, d_over.ptr)
        pre_flags = vmd.POSES_ON_DEVICE | api.OUT_ON_DEVICE

        def pre():
            api.check(api.lib().mmdx_skeleton_solve_pre(seam.h, dm.h, ni, d_poses.ptr, None, pre_flags, d_seam.ptr))

        def pre_post():
            pre()
            api.check(api.lib().mmdx_skeleton_solve_post(seam.h, dm.h, ni, C.byref(ov), vmd.OVERRIDES_ON_DEVICE | api.OUT_ON_DEVICE, d_seam.ptr))
        print(f"\nNI={ni} NB={NB}, {N_CHAINS} chains x {N_JOINTS} joints, {N_COLLIDERS} colliders; the step moves {2 * moved / 1e6:.1f} MB", flush=True)

        def timed(run):
            for _ in range(5):
                run()
            dm.sync()
            t0 = time.perf_counter()
            for _ in range(iters):
                run()
            dm.sync()
            return (time.perf_counter() - t0) / iters * 1e6

        def by_events(run):
            dm.sync()
            dm.timer_start()
            for _ in range(iters):
                run()
            return dm.timer_stop() / iters * 1e3
        step = lambda: sset.step(d_pal, dt_ptr=d_dt.ptr, n_instances=ni, model=dm)                      # noqa: E731
        step_sel = lambda: sset.step(d_pal, dt_ptr=d_dt.ptr, n_instances=ni, select=sel, model=dm)      # noqa: E731
        res = {}
        for r in range(rounds + 1):
            row = {}
            row["springs"], row["springs_ev"] = timed(step), by_events(step)      # every row back to back inside a round: interleaved
            row["springs_list"] = timed(step_sel)
            row["solve"] = timed(solve)
            ms_avg = C.c_float(0)
            api.check(api.lib().mmdx_bench_copy(d_dst.ptr, d_src.ptr, moved, iters, C.byref(ms_avg)))
            row["copy"] = float(ms_avg.value) * 1e3
            row["pre"], row["pre_post"] = timed(pre), timed(pre_post)
            if r >= 1:                                                          # round 0 warms every row up
                for k, us in row.items():
                    res.setdefault(k, []).append(us)
        res["post"] = [b - a for a, b in zip(res["pre"], res["pre_post"])]
        print(f"us per call, median of {rounds} rounds of {iters} calls (min-max of the rounds)")
        for k, text in (("springs", "spring step, host clock"), ("springs_ev", "spring step, HIP events"),
                        ("springs_list", "spring step through a device list of every instance, host clock"),
                        ("solve", "blend solve (mmdx_skeleton_solve_motion_set_blend_time), host clock"),
                        ("copy", "device copy of the bytes the step moves, HIP events"),
                        ("pre", "seam: solve_pre alone, host clock"), ("pre_post", "seam: solve_pre + solve_post (96 device override rows), host clock"),
                        ("post", "seam: solve_post = the difference")):
            print(f"{text:<75} {med(res[k]):9.2f} ({min(res[k]):.2f}-{max(res[k]):.2f})")
        s = med(res["springs"])
        print(f"ratios: springs / solve {s / med(res['solve']):.2f}, springs / copy {med(res['springs_ev']) / med(res['copy']):.2f} (both by HIP events), "
              f"springs / seam post {s / med(res['post']):.3f}", flush=True)
        for d in (d_pal, d_seam, d_ca, d_cb, d_ta, d_tb, d_w, d_dt, d_ids, d_src, d_dst, d_poses, d_over):
            d.free()
        sset.close()
    for x in [seam, sk, ms] + bms + vs:
        x.close()
    dm.close()


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Interleaved A/B of the cross-fade entry points (mmdx_motion_set_blend_*_time, mmdx_skeleton_solve_motion_set_blend_time)
against the motion-set calls they extend, in ONE process, on the same arrays, median of R rounds.

    timeout -k 10 600 python tools/motion_blend_ab.py            (AB_ROUNDS=7 AB_ITERS=200)

Shape: the workload of tools/motion_set_ab.py -- 1 024 x 300 bones + 200 morphs, a set of 8 clips of 20 keys per bone over 600
frames and 12 keys per morph, clip ids at random, every operand in HBM, times with sub-frame offsets.  Per entry point (the bone
track call, the morph track call, the one-launch solve) the rows are
    (a) the parent's ..._motion_set_time call on (clips_a, times_a): the yardstick
    (b) the blend call with every weight 0       (every row is A: one evaluation per row)
    (c) the blend call with every weight 0.5     (every row evaluates both clips and blends)
    (d) the blend call with 10 % of the instances at 0.5, scattered, the rest at 0
in microseconds per call (AB_ITERS back-to-back calls between two syncs, so launch overhead is included), then (b)/(a), (c)/(a)
and (d)/(a) with the min-max of the per-round ratio, next to the min-max spread of (a) itself.  Nothing here is a pass / fail
number."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from simple_mmd_renderer_amd import synth, vmd  # noqa: E402
from simple_mmd_renderer_amd.engine import DeformModel, DeviceBuffer  # noqa: E402
from tools.motion_set_ab import NCLIPS, NI, NM, make_clip  # noqa: E402


def main():
    rounds, iters = int(os.environ.get("AB_ROUNDS", "7")), int(os.environ.get("AB_ITERS", "200"))
    m = synth.make_config("config3_crowd")
    names = [f"b{i}" for i in range(m.nb)]
    mnames = [f"m{i}" for i in range(NM)]
    dm = DeformModel(m)
    sk = vmd.Skeleton(m.bone_pos, np.asarray(m.bone_parent, np.int32))
    assert sk.info["solver"] == vmd.SOLVER_PARALLEL_FK
    vs = [make_clip(303 + c, names, mnames) for c in range(NCLIPS)]
    bms, mms = [v.bind_bones(names) for v in vs], [v.bind_morphs(mnames) for v in vs]
    ms = vmd.MotionSet(bms, mms)
    print(f"NI={NI} NB={m.nb} NM={NM}; set of {NCLIPS}: {ms.info}", flush=True)
    rng = np.random.default_rng(2026)
    ta = ((np.arange(NI) * 7) % 600) / 30.0 + (np.arange(NI) % 5) / 144.0
    tb = ((np.arange(NI) * 11 + 13) % 600) / 30.0 + (np.arange(NI) % 7) / 144.0
    ca = rng.integers(0, NCLIPS, NI).astype(np.uint32)
    cb = rng.integers(0, NCLIPS, NI).astype(np.uint32)
    w10 = np.zeros(NI, np.float32)
    w10[rng.permutation(NI)[:NI // 10]] = 0.5
    weights = {"b": np.zeros(NI, np.float32), "c": np.full(NI, 0.5, np.float32), "d": w10}
    d_ca, d_ta, d_cb, d_tb = (DeviceBuffer.from_numpy(x) for x in (ca, ta, cb, tb))
    d_wt = {k: DeviceBuffer.from_numpy(v) for k, v in weights.items()}
    d_pose, d_pal, d_w = DeviceBuffer(NI * m.nb * 32), DeviceBuffer(NI * m.nb * 64), DeviceBuffer(NI * NM * 4)

    def ops(k):
        return (d_ca.ptr, d_ta.ptr, d_cb.ptr, d_tb.ptr, d_wt[k].ptr)
    rows = {
        "blend_bones_time": dict(
            {"a": lambda: ms.eval_bones_time_device(NI, d_ca.ptr, d_ta.ptr, d_pose.ptr, dm)},
            **{k: (lambda k=k: ms.blend_bones_time_device(NI, *ops(k), d_pose.ptr, dm)) for k in "bcd"}),
        "blend_morphs_time": dict(
            {"a": lambda: ms.eval_morphs_time_device(NI, d_ca.ptr, d_ta.ptr, d_w.ptr, dm)},
            **{k: (lambda k=k: ms.blend_morphs_time_device(NI, *ops(k), d_w.ptr, dm)) for k in "bcd"}),
        "solve_motion_set_blend_time": dict(
            {"a": lambda: sk.solve_motion_set_time_device(ms, NI, d_ca.ptr, d_ta.ptr, d_pal.ptr, dm)},
            **{k: (lambda k=k: sk.solve_motion_set_blend_time_device(ms, NI, *ops(k), d_pal.ptr, dm)) for k in "bcd"}),
    }

    def timed(run):
        for _ in range(5):
            run()
        dm.sync()
        t0 = time.perf_counter()
        for _ in range(iters):
            run()
        dm.sync()
        return (time.perf_counter() - t0) / iters * 1e6

    res = {}
    for r in range(rounds + 1):
        for name, variants in rows.items():
            for v, run in variants.items():            # a, b, c, d back to back inside a round: interleaved
                us = timed(run)
                if r >= 1:                             # round 0 warms every row up
                    res.setdefault((name, v), []).append(us)
    print(f"\n{'entry point':28s} {'(a) set call':>12s} {'(b) w=0':>9s} {'(c) w=.5':>9s} {'(d) 10% .5':>10s} "
          f"{'(b)/(a)':>8s} {'per round':>13s} {'(c)/(a)':>8s} {'per round':>13s} {'(d)/(a)':>8s} {'per round':>13s} {'(a) spread':>13s}"
          f"   (us per call, median of {rounds})")
    for name in rows:
        a, b, c, d = (np.array(res[(name, v)]) for v in "abcd")
        ma, mb, mc, md = (float(np.median(x)) for x in (a, b, c, d))
        print(f"{name:28s} {ma:12.2f} {mb:9.2f} {mc:9.2f} {md:10.2f} "
              f"{mb / ma:8.3f} {(b / a).min():6.3f}-{(b / a).max():5.3f} {mc / ma:8.3f} {(c / a).min():6.3f}-{(c / a).max():5.3f} "
              f"{md / ma:8.3f} {(d / a).min():6.3f}-{(d / a).max():5.3f} {a.min() / ma:6.3f}-{a.max() / ma:5.3f}", flush=True)
    for x in [ms, sk] + bms + mms + vs + [d_ca, d_ta, d_cb, d_tb, d_pose, d_pal, d_w] + list(d_wt.values()):
        x.free() if isinstance(x, DeviceBuffer) else x.close()
    dm.close()


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Interleaved A/B of the motion-set entry points against the plain single-motion calls, in ONE process, on the same arrays,
median of R rounds.

    timeout -k 10 600 python tools/motion_set_ab.py            (AB_ROUNDS=7 AB_ITERS=200)

Shape: the `tracks -> palettes, 1 024 x 300 bones` FK row of tools/rig_bench.py plus 200 morphs; clips of 20 keys per bone over 600
frames and 12 keys per morph, every operand in HBM, times with sub-frame offsets.  Per entry point (mmdx_motion_set_eval_bones_time,
mmdx_motion_set_eval_morphs_time, and mmdx_skeleton_solve_motion_set_time on the one-launch path) the rows are
    (a) the plain single-motion call (mmdx_bone_motion_eval_time / mmdx_morph_motion_eval_time / mmdx_skeleton_solve_motion_time):
        the parent's kernel, the yardstick
    (b) a set of 1 clip (all clip ids 0)
    (c) a set of 8 clips, the instances sorted by clip
    (d) the same 8 clips assigned at random
in microseconds per call (AB_ITERS back-to-back calls between two syncs, so launch overhead is included), then (b)/(a) with the
min-max of the per-round ratio next to the min-max spread of (a) itself, and (d)/(c), the price of the scattered working set."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from simple_mmd_renderer_amd import synth, vmd  # noqa: E402
from simple_mmd_renderer_amd.engine import DeformModel, DeviceBuffer  # noqa: E402

NI, NM, NCLIPS = 1024, 200, 8


def make_clip(seed, names, mnames):
    rng = np.random.RandomState(seed)
    mk = [(n, int(f), float(np.float32(rng.uniform(0, 1)))) for n in mnames for f in sorted(rng.choice(600, 12, replace=False))]
    return vmd.Vmd(vmd.write_vmd(synth.make_bone_keys(names, seed, keys_per=20, span=600), mk))


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
    set1, set8 = vmd.MotionSet(bms[:1], mms[:1]), vmd.MotionSet(bms, mms)
    print(f"NI={NI} NB={m.nb} NM={NM}; one clip: {bms[0].n_keys} bone keys, {bms[0].n_curves} curves, {mms[0].n_keys} morph keys; "
          f"set of {NCLIPS}: {set8.info}", flush=True)
    rng = np.random.default_rng(2026)
    t = ((np.arange(NI) * 7) % 600) / 30.0 + (np.arange(NI) % 5) / 144.0
    d_t = DeviceBuffer.from_numpy(t)
    clips = {"one": np.zeros(NI, np.uint32), "sorted": np.sort(rng.integers(0, NCLIPS, NI)).astype(np.uint32)}
    clips["random"] = rng.permutation(clips["sorted"])
    d_c = {k: DeviceBuffer.from_numpy(v) for k, v in clips.items()}
    d_pose, d_pal, d_w = DeviceBuffer(NI * m.nb * 32), DeviceBuffer(NI * m.nb * 64), DeviceBuffer(NI * NM * 4)
    rows = {
        "eval_bones_time": {
            "a": lambda: bms[0].eval_time_device(NI, d_t.ptr, d_pose.ptr, dm),
            "b": lambda: set1.eval_bones_time_device(NI, d_c["one"].ptr, d_t.ptr, d_pose.ptr, dm),
            "c": lambda: set8.eval_bones_time_device(NI, d_c["sorted"].ptr, d_t.ptr, d_pose.ptr, dm),
            "d": lambda: set8.eval_bones_time_device(NI, d_c["random"].ptr, d_t.ptr, d_pose.ptr, dm)},
        "eval_morphs_time": {
            "a": lambda: mms[0].eval_time_device(NI, d_t.ptr, d_w.ptr, dm),
            "b": lambda: set1.eval_morphs_time_device(NI, d_c["one"].ptr, d_t.ptr, d_w.ptr, dm),
            "c": lambda: set8.eval_morphs_time_device(NI, d_c["sorted"].ptr, d_t.ptr, d_w.ptr, dm),
            "d": lambda: set8.eval_morphs_time_device(NI, d_c["random"].ptr, d_t.ptr, d_w.ptr, dm)},
        "solve_motion_set_time": {
            "a": lambda: sk.solve_motion_time_device(bms[0], NI, d_t.ptr, d_pal.ptr, dm),
            "b": lambda: sk.solve_motion_set_time_device(set1, NI, d_c["one"].ptr, d_t.ptr, d_pal.ptr, dm),
            "c": lambda: sk.solve_motion_set_time_device(set8, NI, d_c["sorted"].ptr, d_t.ptr, d_pal.ptr, dm),
            "d": lambda: sk.solve_motion_set_time_device(set8, NI, d_c["random"].ptr, d_t.ptr, d_pal.ptr, dm)},
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
    print(f"\n{'entry point':24s} {'(a) plain':>10s} {'(b) set 1':>10s} {'(c) 8 sorted':>13s} {'(d) 8 random':>13s} "
          f"{'(b)/(a)':>8s} {'per round':>13s} {'(a) spread':>13s} {'(d)/(c)':>8s} {'per round':>13s}"
          f"   (us per call, median of {rounds})")
    for name in rows:
        a, b, c, d = (np.array(res[(name, v)]) for v in "abcd")
        ma, mb, mc, md = (float(np.median(x)) for x in (a, b, c, d))
        print(f"{name:24s} {ma:10.2f} {mb:10.2f} {mc:13.2f} {md:13.2f} {mb / ma:8.3f} {(b / a).min():6.3f}-{(b / a).max():5.3f} "
              f"{a.min() / ma:6.3f}-{a.max() / ma:5.3f} {md / mc:8.3f} {(d / c).min():6.3f}-{(d / c).max():5.3f}", flush=True)
    for x in [set1, set8, sk] + bms + mms + vs + [d_t, d_pose, d_pal, d_w] + list(d_c.values()):
        x.free() if isinstance(x, DeviceBuffer) else x.close()
    dm.close()


if __name__ == "__main__":
    main()

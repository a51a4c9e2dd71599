#!/usr/bin/env python3
"""What the crowd animator's step costs next to the solve it feeds and next to the host alternative, in ONE process, interleaved,
median of R rounds.

    timeout -k 10 600 python tools/animator_ab.py            (AB_ROUNDS=7 AB_ITERS=200)

Shape: the workload of tools/motion_set_ab.py -- 300 bones + 200 morphs, a set of 8 clips of 20 keys per bone over 600 frames --
at 1 024 and at 16 384 instances.  The animator plays a mixed crowd: every clip loops, a third of the instances are mid-fade, and
a tenth get a new request every 16th step, so the step takes every branch.  Rows, microseconds per call (AB_ITERS back-to-back
calls between two syncs, so launch overhead is included):
    advance            mmdx_animator_advance with a host dt (a kernel argument)
    advance (dev dt)   the same with MMDX_ANIM_DT_ON_DEVICE
    blend solve        mmdx_skeleton_solve_motion_set_blend_time on the animator's operands: the step advance feeds
    5 x h2d            the host alternative: the five operand arrays (28 bytes per instance) uploaded with five mmdx_memcpy_h2d
                       calls, which is what an adopter without the animator does every frame AFTER computing them on the CPU
then advance / blend solve and advance / 5 x h2d with the min-max of the per-round ratio.  Nothing here is a pass / fail number."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from simple_mmd_renderer_amd import synth, vmd  # noqa: E402
from simple_mmd_renderer_amd.engine import DeformModel, DeviceBuffer  # noqa: E402
from tools.motion_set_ab import NCLIPS, NM, make_clip  # noqa: E402

SIZES = (1024, 16384)


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
    print(f"NB={m.nb} NM={NM}; set of {NCLIPS}: {ms.info}; clip frames {ms.clip_frames().tolist()}", flush=True)
    res = {}
    for ni in SIZES:
        rng = np.random.default_rng(2026 + ni)
        an = vmd.Animator(ms, ni)
        fading = rng.random(ni) < 1 / 3
        state = dict(clips_a=rng.integers(0, NCLIPS, ni), clips_b=np.where(fading, rng.integers(0, NCLIPS, ni), vmd.CLIP_NONE),
                     times_a=rng.uniform(0, 20, ni), times_b=np.where(fading, rng.uniform(0, 20, ni), 0.0),
                     weights=np.where(fading, rng.uniform(0, 1, ni), 0.0), fade_rate=np.where(fading, 2.0, 0.0),
                     speed=rng.choice([1.0, 0.5, -1.0], ni))
        an.set_state(dm, **state)
        host = [np.ascontiguousarray(state[k], t) for k, t in (("clips_a", np.uint32), ("clips_b", np.uint32), ("times_a", np.float64),
                                                               ("times_b", np.float64), ("weights", np.float32))]
        d_host = [DeviceBuffer(a.nbytes) for a in host]
        d_dt = DeviceBuffer.from_numpy(np.array([1 / 60], np.float64))
        d_pal = DeviceBuffer(ni * m.nb * 64)
        ids = rng.permutation(ni)[:ni // 10].astype(np.uint32)
        d_req = [DeviceBuffer.from_numpy(a) for a in (ids, rng.integers(0, NCLIPS, ids.size).astype(np.uint32),
                                                      np.full(ids.size, 0.5, np.float32))]
        step = [0]

        def advance(device_dt):
            step[0] += 1
            if step[0] % 16 == 0:
                an.request_device(ids.size, *[d.ptr for d in d_req], model=dm)
            an.advance_device_dt(d_dt.ptr, dm) if device_dt else an.advance(1 / 60, dm)

        def uploads():
            for d, a in zip(d_host, host):
                d.upload(a)
        rows = {"advance": lambda: advance(False), "advance (dev dt)": lambda: advance(True),
                "blend solve": lambda: sk.solve_motion_set_blend_time_device(ms, ni, *an.operand_ptrs(), d_pal.ptr, dm),
                "5 x h2d": uploads}

        def timed(run):
            for _ in range(5):
                run()
            dm.sync()
            t0 = time.perf_counter()
            for _ in range(iters):
                run()
            dm.sync()
            return (time.perf_counter() - t0) / iters * 1e6
        for r in range(rounds + 1):
            for name, run in rows.items():                 # back to back inside a round: interleaved
                us = timed(run)
                if r >= 1:                                 # round 0 warms every row up
                    res.setdefault((ni, name), []).append(us)
        for x in [an, d_dt, d_pal] + d_host + d_req:
            x.free() if isinstance(x, DeviceBuffer) else x.close()
    print(f"\n{'NI':>6s} {'advance':>9s} {'(dev dt)':>9s} {'blend solve':>12s} {'5 x h2d':>9s} {'adv/solve':>10s} {'per round':>13s} "
          f"{'adv/h2d':>8s} {'per round':>13s} {'advance spread':>15s}   (us per call, median of {rounds})")
    for ni in SIZES:
        a, ad, s, h = (np.array(res[(ni, k)]) for k in ("advance", "advance (dev dt)", "blend solve", "5 x h2d"))
        ma, mad, msv, mh = (float(np.median(x)) for x in (a, ad, s, h))
        print(f"{ni:6d} {ma:9.2f} {mad:9.2f} {msv:12.2f} {mh:9.2f} {ma / msv:10.4f} {(a / s).min():6.4f}-{(a / s).max():6.4f} "
              f"{ma / mh:8.4f} {(a / h).min():6.4f}-{(a / h).max():6.4f} {a.min() / ma:7.3f}-{a.max() / ma:5.3f}", flush=True)
    for x in [ms, sk] + bms + mms + vs:
        x.close()
    dm.close()


if __name__ == "__main__":
    main()

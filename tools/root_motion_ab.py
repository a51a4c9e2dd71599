#!/usr/bin/env python3
"""What root motion costs next to the animator's step, next to the blend solve it precedes and next to the host alternative, in ONE
process, interleaved, median of R rounds.

    timeout -k 10 600 python tools/root_motion_ab.py            (AB_ROUNDS=7 AB_ITERS=200)

Shape: the workload of tools/animator_ab.py -- 300 bones, a set of 8 clips of 20 keys per bone over 600 frames, every clip looping,
a third of the instances mid-fade -- at 1 024 and at 16 384 instances.  The root is bone 0; the call reads a one-bone bank of it
(the intended cheap form) and, for comparison, the whole 300-bone set.  Rows, microseconds per call (AB_ITERS back-to-back calls
between two syncs, so launch overhead is included):
    root motion        mmdx_animator_root_motion on the one-bone bank, host dt
    root (dev dt)      the same with MMDX_ANIM_DT_ON_DEVICE
    root (full set)    the same call reading bone 0 of the 300-bone set
    advance            mmdx_animator_advance, the call it goes in front of (with a device request for a tenth of the crowd every
                       16th step, as in tools/animator_ab.py)
    blend solve        mmdx_skeleton_solve_motion_set_blend_time of the in-place set: the step both feed
    h2d                the host alternative: the placements (32 bytes per instance) uploaded with one mmdx_memcpy_h2d, which is what
                       an adopter without the call does every frame AFTER computing them on the CPU
then root motion / advance, / blend solve and / h2d with the min-max of the per-round ratio.  Nothing here is a pass / fail number.
`advance` steps the clocks and, over a few dozen calls, finishes every fade, so the animator's state (and the placements) are put
back with set_state before EVERY row of every round, outside the timed region, and the fraction of the crowd that is mid-fade is
asserted before the row and -- for every row but `advance`, which alone changes the state -- after it; the fractions are printed
under the table.  So every call of the root rows and of the blend solve does the same work: a third of the crowd evaluates both
sides, and whoever is within a step of its seam evaluates the fold."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from simple_mmd_renderer_amd import _capi as api  # noqa: E402
from simple_mmd_renderer_amd import synth, vmd  # noqa: E402
from simple_mmd_renderer_amd.engine import DeformModel, DeviceBuffer  # noqa: E402
from tools.motion_set_ab import NCLIPS, NM, make_clip  # noqa: E402

SIZES = (1024, 16384)
AXES = api.ROOT_X | api.ROOT_Y | api.ROOT_Z
ROWS = ("root motion", "root (dev dt)", "root (full set)", "advance", "blend solve", "h2d")


def main():
    rounds, iters = int(os.environ.get("AB_ROUNDS", "7")), int(os.environ.get("AB_ITERS", "200"))
    m = synth.make_config("config3_crowd")
    names = [f"b{i}" for i in range(m.nb)]
    mnames = [f"m{i}" for i in range(NM)]
    dm = DeformModel(m)
    sk = vmd.Skeleton(m.bone_pos, np.asarray(m.bone_parent, np.int32))
    assert sk.info["solver"] == vmd.SOLVER_PARALLEL_FK
    vs = [make_clip(303 + c, names, mnames) for c in range(NCLIPS)]
    bms = [v.bind_bones(names) for v in vs]
    still = [b.in_place(0, AXES) for b in bms]
    roots = [v.bind_bones(names[:1]) for v in vs]
    full, in_place, bank = vmd.MotionSet(bms), vmd.MotionSet(still), vmd.MotionSet(roots)
    print(f"NB={m.nb}; set of {NCLIPS}: {full.info}; root bank: {bank.info}; clip frames {full.clip_frames().tolist()}", flush=True)
    res, fades = {}, {}
    for ni in SIZES:
        rng = np.random.default_rng(2026 + ni)
        an = vmd.Animator(in_place, ni)
        fading = rng.random(ni) < 1 / 3
        state = dict(clips_a=rng.integers(0, NCLIPS, ni), clips_b=np.where(fading, rng.integers(0, NCLIPS, ni), vmd.CLIP_NONE),
                     times_a=rng.uniform(0, 20, ni), times_b=np.where(fading, rng.uniform(0, 20, ni), 0.0),
                     weights=np.where(fading, rng.uniform(0, 1, ni), 0.0), fade_rate=np.where(fading, 2.0, 0.0),
                     speed=rng.choice([1.0, 0.5, -1.0], ni))
        an.set_state(dm, **state)
        q = rng.normal(size=(ni, 4))
        place = np.concatenate([rng.uniform(-50, 50, (ni, 3)), np.zeros((ni, 1)), q / np.linalg.norm(q, axis=1, keepdims=True)], 1).astype(np.float32)
        d_place, d_up = DeviceBuffer.from_numpy(place), DeviceBuffer(place.nbytes)
        d_dt = DeviceBuffer.from_numpy(np.array([1 / 60], np.float64))
        d_pal = DeviceBuffer(ni * m.nb * 64)
        ids = rng.permutation(ni)[:ni // 10].astype(np.uint32)
        d_req = [DeviceBuffer.from_numpy(a) for a in (ids, rng.integers(0, NCLIPS, ids.size).astype(np.uint32),
                                                      np.full(ids.size, 0.5, np.float32))]
        step = [0]

        def advance():                                     # as tools/animator_ab.py: a request for a tenth every 16th step
            step[0] += 1
            if step[0] % 16 == 0:
                an.request_device(ids.size, *[d.ptr for d in d_req], model=dm)
            an.advance(1 / 60, dm)
        rows = {"root motion": lambda: an.root_motion(bank, 0, AXES, d_place.ptr, dt=1 / 60, model=dm),
                "root (dev dt)": lambda: an.root_motion(bank, 0, AXES, d_place.ptr, dt_ptr=d_dt.ptr, model=dm),
                "root (full set)": lambda: an.root_motion(full, 0, AXES, d_place.ptr, dt=1 / 60, model=dm),
                "advance": advance,
                "blend solve": lambda: sk.solve_motion_set_blend_time_device(in_place, ni, *an.operand_ptrs(), d_pal.ptr, dm),
                "h2d": lambda: d_up.upload(place)}

        def mid_fade():
            s = an.get_state(dm, names=("fade_rate", "weights"))
            return float(((s["fade_rate"] > 0) & (s["weights"] >= 1e-7) & (s["weights"] <= 1 - 1e-7)).mean())

        def timed(name):
            # `advance` steps the clocks and finishes every fade within 30 steps, so every row starts from the stated crowd, put back
            # outside the timed region; no row but `advance` changes the state, which is checked after the row as well
            an.set_state(dm, **state)
            d_place.upload(place)
            dm.sync()
            before = mid_fade()
            assert 0.28 < before < 0.39, (name, before)
            run = rows[name]
            for _ in range(5):
                run()
            dm.sync()
            t0 = time.perf_counter()
            for _ in range(iters):
                run()
            dm.sync()
            us = (time.perf_counter() - t0) / iters * 1e6
            after = mid_fade()
            assert name == "advance" or after == before, (name, before, after)
            fades[(ni, name)] = (before, after)
            return us
        for r in range(rounds + 1):
            for name in ROWS:                              # back to back inside a round: interleaved
                us = timed(name)
                if r >= 1:                                 # round 0 warms every row up
                    res.setdefault((ni, name), []).append(us)
        for x in [an, d_place, d_up, d_dt, d_pal] + d_req:
            x.free() if isinstance(x, DeviceBuffer) else x.close()
    print(f"\n{'NI':>6s} " + " ".join(f"{k:>15s}" for k in ROWS) + f" {'root/advance':>13s} {'per round':>13s} {'root/solve':>11s} "
          f"{'per round':>13s} {'root/h2d':>9s} {'per round':>13s}   (us per call, median of {rounds})")
    for ni in SIZES:
        t = {k: np.array(res[(ni, k)]) for k in ROWS}
        med = {k: float(np.median(v)) for k, v in t.items()}
        line = f"{ni:6d} " + " ".join(f"{med[k]:15.2f}" for k in ROWS)
        for other in ("advance", "blend solve", "h2d"):
            ratio = t["root motion"] / t[other]
            line += f" {med['root motion'] / med[other]:{13 if other == 'advance' else 11 if other == 'blend solve' else 9}.4f} {ratio.min():6.4f}-{ratio.max():6.4f}"
        print(line, flush=True)
    print("\nfraction of the crowd mid-fade (a running fade and a weight that blends) before -> after the last round of a row:")
    for ni in SIZES:
        print(f"{ni:6d} " + "  ".join(f"{k}: {fades[(ni, k)][0]:.3f} -> {fades[(ni, k)][1]:.3f}" for k in ROWS), flush=True)
    for x in [full, in_place, bank, sk] + bms + still + roots + vs:
        x.close()
    dm.close()


if __name__ == "__main__":
    main()

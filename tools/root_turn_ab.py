#!/usr/bin/env python3
"""What root motion that turns costs next to the plain root-motion call and next to the blend solve it precedes, in ONE process,
interleaved, median of R rounds.

    timeout -k 10 600 python tools/root_turn_ab.py            (AB_ROUNDS=7 AB_ITERS=200)

Shape: the workload of tools/root_motion_ab.py -- 300 bones, a set of 8 clips of 20 keys per bone over 600 frames, every clip
looping, a third of the instances mid-fade -- at 1 024 and at 16 384 instances.  The root is bone 0; the calls read a one-bone bank
of it.  Rows, microseconds per call (AB_ITERS back-to-back calls between two syncs, so launch overhead is included):
    root motion        (a) mmdx_animator_root_motion, host dt
    root turn          (b) mmdx_animator_root_motion_turn, host dt
    turn + normalize   (c) the same with MMDX_ROOT_NORMALIZE
    blend solve        mmdx_skeleton_solve_motion_set_blend_time of the in-place-turn set: the step they feed
then (b) / (a) and (c) / (a) with the min-max of the per-round ratio.  Nothing here is a pass / fail number.
No row changes the animator's state; the placements, which every root row moves and the turn rows also turn, are put back before
EVERY row of every round, outside the timed region, so that no row starts from headings another row's 200 products have drifted.
The fraction of the crowd that is mid-fade is asserted before and after every row and printed under the table."""
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
ROWS = ("root motion", "root turn", "turn + normalize", "blend solve")


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
    still = [b.in_place_turn(0, AXES) for b in bms]
    roots = [v.bind_bones(names[:1]) for v in vs]
    in_place, bank = vmd.MotionSet(still), vmd.MotionSet(roots)
    print(f"NB={m.nb}; in-place-turn set of {NCLIPS}: {in_place.info}; root bank: {bank.info}", flush=True)
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
        d_place = DeviceBuffer.from_numpy(place)
        d_pal = DeviceBuffer(ni * m.nb * 64)
        rows = {"root motion": lambda: an.root_motion(bank, 0, AXES, d_place.ptr, dt=1 / 60, model=dm),
                "root turn": lambda: an.root_turn(bank, 0, AXES, d_place.ptr, dt=1 / 60, model=dm),
                "turn + normalize": lambda: an.root_turn(bank, 0, AXES, d_place.ptr, dt=1 / 60, model=dm, normalize=True),
                "blend solve": lambda: sk.solve_motion_set_blend_time_device(in_place, ni, *an.operand_ptrs(), d_pal.ptr, dm)}

        def mid_fade():
            s = an.get_state(dm, names=("fade_rate", "weights"))
            return float(((s["fade_rate"] > 0) & (s["weights"] >= 1e-7) & (s["weights"] <= 1 - 1e-7)).mean())

        def timed(name):
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
            assert after == before, (name, before, after)
            fades[(ni, name)] = (before, after)
            return us
        for r in range(rounds + 1):
            for name in ROWS:                              # back to back inside a round: interleaved
                us = timed(name)
                if r >= 1:                                 # round 0 warms every row up
                    res.setdefault((ni, name), []).append(us)
        for x in [an, d_place, d_pal]:
            x.free() if isinstance(x, DeviceBuffer) else x.close()
    print(f"\n{'NI':>6s} " + " ".join(f"{k:>17s}" for k in ROWS) + f" {'turn/plain':>11s} {'per round':>13s} {'norm/plain':>11s} "
          f"{'per round':>13s} {'turn/solve':>11s}   (us per call, median of {rounds})")
    for ni in SIZES:
        t = {k: np.array(res[(ni, k)]) for k in ROWS}
        med = {k: float(np.median(v)) for k, v in t.items()}
        line = f"{ni:6d} " + " ".join(f"{med[k]:17.2f}" for k in ROWS)
        for row in ("root turn", "turn + normalize"):
            ratio = t[row] / t["root motion"]
            line += f" {med[row] / med['root motion']:11.4f} {ratio.min():6.4f}-{ratio.max():6.4f}"
        line += f" {med['root turn'] / med['blend solve']:11.4f}"
        print(line, flush=True)
    print("\nfraction of the crowd mid-fade (a running fade and a weight that blends) before -> after the last round of a row:")
    for ni in SIZES:
        print(f"{ni:6d} " + "  ".join(f"{k}: {fades[(ni, k)][0]:.3f} -> {fades[(ni, k)][1]:.3f}" for k in ROWS), flush=True)
    for x in [in_place, bank, sk] + bms + still + roots + vs:
        x.close()
    dm.close()


if __name__ == "__main__":
    main()

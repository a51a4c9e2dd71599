"""Generate tests/golden/root_q8.vmd and tests/golden/root_turn_expect.npz: mmdx_animator_root_motion_turn (include/mmdx.h) as the
real libmmd computes it.

The clips are the six of tests/root_motion_ref (root_curved has rotating root keys) and root_q8, written by the project's own
vmd.write_vmd (tests/root_turn_ref.write_q8).  Rows: every weight of motion_blend_ref.WEIGHTS, with and without a running fade,
over the scenarios below -- plain steps, folds forwards and backwards on either side, steps of several laps, clamps under HOLD and
THEN, dt = 0 and NaN, speeds 1, 0.5, -1 and 0, MMDX_CLIP_NONE and ids out of range on either side, the track-less clip, the clip of
length 0, root_q8 across its seam -- with the axes, MMDX_ROOT_NORMALIZE and the headings cycling underneath; then the 45 rows of a
walk along root_curved, one per step of 1/30 s, whose (T, Q) the general closure test chains in float64.

Every number comes from tests/root_turn_driver.cpp: (T, Q) by Motion::GetBonePose(name, double), the combination by Quaternionf's
and Vector3f's operators, ToRotateMatrix, rotate and NLerp, the clocks by a host build of csrc/anim_math.hpp.  Needs the reference's
headers:
    python -m tests.gen_root_turn_golden
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import motion_blend_ref as mb  # noqa: E402
from tests import root_motion_ref as rm  # noqa: E402
from tests import root_turn_ref as rt  # noqa: E402

F = np.float32
NONE, OUT = rt.NONE, 77
NAN = float("nan")
# (speed, dt, clip a, time a, clip b, time b)
SCENARIOS = (
    (1.0, 1 / 60, 0, 0.3, 1, 0.2),                  # a plain step
    (1.0, 1 / 30, 0, 1.49, 4, 0.5),                 # a folds forwards, b turns under HOLD
    (1.0, 1 / 30, 1, 0.5, 0, 1.49),                 # b folds forwards
    (-1.0, 1 / 30, 0, 0.01, 1, 0.02),               # both fold backwards
    (1.0, 7.0, 0, 0.4, rt.Q8, 0.3),                 # several laps forwards
    (-1.0, 7.0, rt.Q8, 0.4, 0, 0.3),                # several laps backwards
    (1.0, 1 / 30, 4, 1.49, 5, 0.99),                # HOLD and THEN clamp at the end
    (-1.0, 1 / 60, 4, 0.005, 5, 0.01),              # ... and at the start
    (1.0, 0.0, 0, 0.7, rt.Q8, 0.5),                 # a step of 0
    (0.5, 1 / 60, 0, 1.0, 2, 0.3),                  # half speed; b has no root keys
    (0.5, 1 / 30, rt.Q8, 1.99, 0, 1.495),           # half speed across the seam, both sides
    (0.0, 1 / 60, 0, 1.0, rt.Q8, 0.3),              # speed 0
    (1.0, 1 / 60, NONE, 0.5, 0, 0.3),
    (1.0, 1 / 60, 0, 0.5, NONE, 0.3),
    (1.0, 1 / 60, OUT, 0.5, rt.Q8, 0.3),
    (1.0, 1 / 60, rt.Q8, 0.5, OUT, 0.3),
    (1.0, 1 / 60, 3, 0.3, 0, 1.2),                  # a clip of length 0
    (1.0, NAN, 0, 0.3, 1, 0.2),                     # a NaN step writes nothing
    (1.0, 0.5, rt.Q8, 1.5, 0, 0.75),                # root_q8 lands on its last key: a fold of exact values
    (-1.0, 1 / 144, 0, 0.002, rt.Q8, 0.004),        # a short backward fold on both sides
)
WALK_STEPS, WALK_DT = 45, 1 / 30


def heading(rng, r):
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    kind = r % 3                                     # identity, a unit quaternion, an unnormalised one
    return (0.0, 0.0, 0.0, 1.0) if kind == 0 else q if kind == 1 else q * rng.uniform(0.4, 1.7)


def cases():
    rng = np.random.RandomState(20262)
    cols = {k: [] for k, _ in rt.ROW_ARRAYS}
    r = 0
    for weight in mb.WEIGHTS:
        for fade_rate in (0.0, 3.0):
            for speed, dt, ca, ta, cb, tb in SCENARIOS:
                place = np.concatenate([rng.uniform(-20, 20, 3), [rng.uniform(-1, 1)], heading(rng, r)]).astype(F)
                axes = 7 if r % 5 < 3 else (r // 5) % 8
                flags = rt.ROOT_NORMALIZE if rng.rand() < 0.5 else 0
                for k, v in zip(cols, (ca, cb, ta, tb, weight, speed, fade_rate, dt, axes, place, flags)):
                    cols[k].append(v)
                r += 1
    # the walk along root_curved: the clocks of 45 steps of 1/30 s from t = 0 (a row per step; the headings are the rows' own)
    tab = rt.table()
    t = 0.0
    for k in range(WALK_STEPS):
        place = np.concatenate([rng.uniform(-20, 20, 3), [rng.uniform(-1, 1)], heading(rng, 1)]).astype(F)
        for key, v in zip(cols, (0, NONE, t, 0.0, 0.0, 1.0, 0.0, WALK_DT, 7, place, rt.ROOT_NORMALIZE if k % 2 else 0)):
            cols[key].append(v)
        t = float(rm.ar.wrap(tab, np.array([0], np.uint32), np.array([t + 1.0 * WALK_DT]))[0][0])
    return {k: np.array(cols[k], t) for k, t in rt.ROW_ARRAYS}


def main():
    rt.write_q8()
    rows = cases()
    got = rt.run_libmmd_driver(rt.table(), rows)
    z = dict(rows, times=got["times"], folded=got["folded"], t=got["t"], q=got["q"], expect=got["expect"],
             walk=np.arange(rows["dt"].size - WALK_STEPS, rows["dt"].size, dtype=np.uint32))
    print(rt.check_coverage(z))
    np.savez_compressed(rt.FIXTURE, **z)
    print("%s: %d rows, %.1f KB" % (os.path.basename(rt.FIXTURE), rows["dt"].size, os.path.getsize(rt.FIXTURE) / 1024))
    print("%s: %.1f KB" % (os.path.basename(rt.Q8_VMD), os.path.getsize(rt.Q8_VMD) / 1024))


if __name__ == "__main__":
    main()

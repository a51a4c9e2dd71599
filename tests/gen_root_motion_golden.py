"""Generate tests/golden/root_*.vmd and tests/golden/root_motion_expect.npz: mmdx_animator_root_motion (include/mmdx.h) as the real
libmmd computes it.

The clips are written by the project's own vmd.write_vmd (tests/root_motion_ref.write_clips): a curved root track that does not
close, a linear one, a clip without root keys and a clip of length 0, on a parentless root name next to a few bones of rig_small.
Rows: every weight of motion_blend_ref.WEIGHTS, with and without a running fade, over the scenarios below -- plain steps, folds
forwards and backwards, steps of several laps, clamps under HOLD and THEN, dt = 0 and NaN, speeds 1, 0.5, -1 and 0, MMDX_CLIP_NONE
and ids out of range on either side -- with the axes and the headings cycling underneath.

Every number comes from tests/root_motion_driver.cpp: R by Motion::GetBonePose(name, double), the combination by Vector3f's
operators, Quaternion::ToRotateMatrix and rotate, the clocks by a host build of csrc/anim_math.hpp.  Needs the reference's headers:
    python -m tests.gen_root_motion_golden
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import motion_blend_ref as mb  # noqa: E402
from tests import root_motion_ref as rm  # noqa: E402

F = np.float32
NONE, OUT = rm.NONE, 77
NAN = float("nan")
# (speed, dt, clip a, time a, clip b, time b)
SCENARIOS = (
    (1.0, 1 / 60, 0, 0.3, 1, 0.2),                  # a plain step
    (1.0, 1 / 30, 0, 1.49, 1, 0.99),                # both sides fold forwards
    (-1.0, 1 / 30, 0, 0.01, 1, 0.02),               # both fold backwards
    (1.0, 7.0, 0, 0.4, 1, 0.3),                     # several laps forwards
    (-1.0, 7.0, 1, 0.4, 0, 0.3),                    # several laps backwards
    (1.0, 1 / 30, 4, 1.49, 5, 0.99),                # HOLD and THEN clamp at the end
    (-1.0, 1 / 60, 4, 0.005, 5, 0.01),              # ... and at the start
    (1.0, 0.0, 0, 0.7, 1, 0.5),                     # a step of 0
    (0.5, 1 / 60, 0, 1.0, 2, 0.3),                  # half speed; b has no root keys
    (0.5, 1 / 30, 1, 0.99, 0, 1.495),               # half speed across the seam
    (0.0, 1 / 60, 0, 1.0, 1, 0.3),                  # speed 0
    (1.0, 1 / 60, NONE, 0.5, 1, 0.3),
    (1.0, 1 / 60, 0, 0.5, NONE, 0.3),
    (1.0, 1 / 60, OUT, 0.5, 1, 0.3),
    (1.0, 1 / 60, 1, 0.5, OUT, 0.3),
    (1.0, 1 / 60, 3, 0.3, 0, 1.2),                  # a clip of length 0
    (1.0, NAN, 0, 0.3, 1, 0.2),                     # a NaN step writes nothing
    (1.0, 1 / 144, 2, 0.5, 4, 0.75),
)


def cases():
    rng = np.random.RandomState(20261)
    cols = {k: [] for k, _ in rm.ROW_ARRAYS}
    r = 0
    for weight in mb.WEIGHTS:
        for fade_rate in (0.0, 3.0):
            for speed, dt, ca, ta, cb, tb in SCENARIOS:
                q = rng.normal(size=4)
                q /= np.linalg.norm(q)
                kind = r % 3                         # identity, a unit quaternion, an unnormalised one
                q = (0.0, 0.0, 0.0, 1.0) if kind == 0 else q if kind == 1 else q * rng.uniform(0.4, 1.7)
                place = np.concatenate([rng.uniform(-20, 20, 3), [rng.uniform(-1, 1)], q]).astype(F)
                for k, v in zip(cols, (ca, cb, ta, tb, weight, speed, fade_rate, dt, 7 if r % 5 < 3 else (r // 5) % 8, place)):
                    cols[k].append(v)
                r += 1
    return {k: np.array(cols[k], t) for k, t in rm.ROW_ARRAYS}


def main():
    rm.write_clips()
    rows = cases()
    got = rm.run_libmmd_driver(rm.table(), rows)
    z = dict(rows, times=got["times"], folded=got["folded"], r=got["r"], expect=got["expect"])
    print(rm.check_coverage(z))
    np.savez_compressed(rm.FIXTURE, **z)
    print("%s: %d rows, %.1f KB" % (os.path.basename(rm.FIXTURE), rows["dt"].size, os.path.getsize(rm.FIXTURE) / 1024))
    for p in rm.VMDS.values():
        print("%s: %.1f KB" % (os.path.basename(p), os.path.getsize(p) / 1024))


if __name__ == "__main__":
    main()

"""Generate tests/golden/pose_add_expect.npz: additive layers (include/mmdx.h, mmdx_pose_add / mmdx_rate_add) as the real libmmd
computes them.

A rows and B rows are the cross-fade fixture's two clips (tests/gen_motion_blend_golden.py) at times of its time table, evaluated
by libmmd through tests/motion_blend_driver.cpp as it is (clip 0 for A, clip 1 for B); reference row 0 is clip 1 at time 0.  Rows:
every weight of pose_add_ref.WEIGHTS under each of the four mask rows of row_blend_ref and under MMDX_MASK_NONE, without a
reference (MMDX_REF_NONE) and with reference 0, three (time a, time b) pairs each; then pose_add_ref.synthetic_rows, what the clips
cannot reach, once without and once with reference row 1.  The expected rows come from tests/pose_add_driver.cpp: libmmd's own
Quaternionf / Vector3f operators.  Needs the reference's headers:
    python -m tests.gen_pose_add_golden
"""
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import gen_motion_blend_golden as gmb  # noqa: E402
from tests import golden_util as gu  # noqa: E402
from tests import pose_add_ref as pa  # noqa: E402
from tests import row_blend_ref as rb  # noqa: E402


def cases():
    t = gmb.fixture_times()
    t = t[np.isfinite(t)]
    sa, sb = (next(s for s in range(s0, s0 + t.size) if math.gcd(s, t.size) == 1) for s0 in (5, 11))
    ta, tb, w, ids, refs = [], [], [], [], []
    r = 0
    for weight in pa.WEIGHTS:
        for m in list(range(rb.N_MASKS)) + [rb.MASK_NONE]:
            for ref in (pa.REF_NONE, 0):
                for _ in range(pa.TIMES_PER_CASE):
                    w.append(weight); ids.append(m); refs.append(ref)
                    ta.append(t[(r * sa + 1) % t.size])
                    tb.append(t[(r * sb + 4) % t.size])
                    r += 1
    return np.array(ta, np.float64), np.array(tb, np.float64), np.array(w, np.float32), np.array(ids, np.uint32), np.array(refs, np.uint32)


def build():
    zr = np.load(os.path.join(gu.GOLDEN_DIR, "rig_small_expect.npz"))
    zv = np.load(os.path.join(gu.GOLDEN_DIR, "vmd_small_expect.npz"))
    bone_names = [str(n) for n in zr["model_bone_names"]]
    morph_names = [str(n) for n in zv["model_morph_names"]]
    nb, nm = len(bone_names), len(morph_names)
    ta, tb, w, ids, rids = cases()
    n = w.size
    clip_a, clip_b = np.zeros(n, np.uint32), np.ones(n, np.uint32)
    ops = (bone_names, morph_names, clip_a, ta, clip_b, tb)
    a_poses, a_rates = rb.driver_expect(*ops, np.zeros((n, nb), np.float32), np.zeros((n, nm), np.float32))
    b_poses, b_rates = rb.driver_expect(*ops, np.ones((n, nb), np.float32), np.ones((n, nm), np.float32))
    one, zero = np.ones(1, np.uint32), np.zeros(1, np.float64)
    ref_pose, ref_rate = rb.driver_expect(bone_names, morph_names, one, zero, one, zero, np.zeros((1, nb), np.float32),
                                          np.zeros((1, nm), np.float32))
    sap, sbp, srp, sar, sbr, srr, sw = pa.synthetic_rows(nb, nm)
    ns = sw.size
    z = dict(weights=np.r_[w, sw, sw], mask_ids=np.r_[ids, np.full(2 * ns, rb.MASK_NONE, np.uint32)],
             ref_ids=np.r_[rids, np.full(ns, pa.REF_NONE, np.uint32), np.ones(ns, np.uint32)],
             times_a=np.r_[ta, np.full(2 * ns, np.nan)], times_b=np.r_[tb, np.full(2 * ns, np.nan)],
             synthetic=np.r_[np.zeros(n, bool), np.ones(2 * ns, bool)],
             bone_masks=rb.mask_rows(nb, 31), morph_masks=rb.mask_rows(nm, 32),
             pose_refs=np.stack([ref_pose[0], srp]), rate_refs=np.stack([ref_rate[0], srr]),
             a_poses=np.concatenate([a_poses, sap, sap]), b_poses=np.concatenate([b_poses, sbp, sbp]),
             a_rates=np.concatenate([a_rates, sar, sar]), b_rates=np.concatenate([b_rates, sbr, sbr]))
    z["expect_poses"], z["expect_rates"] = pa.driver_expect(z["a_poses"], z["b_poses"], z["a_rates"], z["b_rates"], z["weights"],
                                                            z["bone_masks"], z["morph_masks"], z["mask_ids"], z["pose_refs"],
                                                            z["rate_refs"], z["ref_ids"])
    pa.check_coverage(z)
    return z


def main():
    z = build()
    np.savez_compressed(pa.FIXTURE, **z)
    print("%s: %d rows, %.1f KB" % (os.path.basename(pa.FIXTURE), z["weights"].size, os.path.getsize(pa.FIXTURE) / 1024))


if __name__ == "__main__":
    main()

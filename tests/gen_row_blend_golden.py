"""Generate tests/golden/row_blend_expect.npz: the masked blend of two evaluated rows (include/mmdx.h, mmdx_pose_blend /
mmdx_rate_blend) as the real libmmd computes it.

The two clips and the rig_small names are the cross-fade fixture's (tests/gen_motion_blend_golden.py).  Rows: every weight of
motion_blend_ref.WEIGHTS for every pair of motion_blend_ref.PAIRS under each of four mask rows (values from {0, 0.25, 0.5, 1}) and
under MMDX_MASK_NONE, one (time a, time b) each from the cross-fade fixture's time table.  tests/motion_blend_driver.cpp is used
as it is, once per bone or morph, with that item's effective weights float32(w) * float32(mask[m][j]); the A and B rows are its
output at weight 0 and weight 1.  Needs the reference's headers:
    python -m tests.gen_row_blend_golden
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
from tests import motion_blend_ref as mb  # noqa: E402
from tests import row_blend_ref as rb  # noqa: E402


def cases():
    t = gmb.fixture_times()
    # both strides coprime to the table size: each side walks the whole table before it repeats a time
    sa, sb = (next(s for s in range(s0, s0 + t.size) if math.gcd(s, t.size) == 1) for s0 in (7, 13))
    ca, cb, ta, tb, w, ids = [], [], [], [], [], []
    r = 0
    for weight in mb.WEIGHTS:
        for a, b in mb.PAIRS:
            for m in list(range(rb.N_MASKS)) + [rb.MASK_NONE]:
                ca.append(a); cb.append(b); w.append(weight); ids.append(m)
                ta.append(t[(r * sa + 2) % t.size])
                tb.append(t[(r * sb + 5) % t.size])
                r += 1
    return (np.array(ca, np.uint32), np.array(ta, np.float64), np.array(cb, np.uint32), np.array(tb, np.float64),
            np.array(w, np.float32), np.array(ids, np.uint32))


def main():
    zr = np.load(os.path.join(gu.GOLDEN_DIR, "rig_small_expect.npz"))
    zv = np.load(os.path.join(gu.GOLDEN_DIR, "vmd_small_expect.npz"))
    bone_names = [str(n) for n in zr["model_bone_names"]]
    morph_names = [str(n) for n in zv["model_morph_names"]]
    nb, nm = len(bone_names), len(morph_names)
    ca, ta, cb, tb, w, ids = cases()
    bone_masks, morph_masks = rb.mask_rows(nb, 31), rb.mask_rows(nm, 32)
    e_bones = rb.effective_weights(w, nb, bone_masks, ids)
    e_morphs = rb.effective_weights(w, nm, morph_masks, ids)
    poses, rates = rb.driver_expect(bone_names, morph_names, ca, ta, cb, tb, e_bones, e_morphs)
    a_poses, a_rates = rb.driver_expect(bone_names, morph_names, ca, ta, cb, tb, np.zeros_like(e_bones), np.zeros_like(e_morphs))
    b_poses, b_rates = rb.driver_expect(bone_names, morph_names, ca, ta, cb, tb, np.ones_like(e_bones), np.ones_like(e_morphs))
    z = dict(clips_a=ca, clips_b=cb, times_a=ta, times_b=tb, weights=w, mask_ids=ids, bone_masks=bone_masks, morph_masks=morph_masks,
             bone_names=np.array(bone_names), morph_names=np.array(morph_names), a_poses=a_poses, b_poses=b_poses, a_rates=a_rates,
             b_rates=b_rates, expect_poses=poses, expect_rates=rates)
    rb.check_coverage(z)
    np.savez_compressed(rb.FIXTURE, **z)
    print("%s: %d rows, %.1f KB" % (os.path.basename(rb.FIXTURE), w.size, os.path.getsize(rb.FIXTURE) / 1024))


if __name__ == "__main__":
    main()

"""Generate tests/golden/motion_time_expect.npz: what the real libmmd's MotionPlayer::SeekTime computes for the committed
motions tests/golden/vmd_small.vmd (morph tracks) and rig_small.vmd (bone tracks), at times chosen to cover the time path's
corners (include/mmdx.h, mmdx_morph_motion_eval_time, points 1-6):

  * -1, -0, 0, -inf, +inf, 1e300;
  * n/60 and n/144 seconds across the whole span and past its end (display-rate loops);
  * k/30 for every key frame k of every track, and the neighbouring doubles on both sides (k/30 * 30 lands on either side
    of k, or on it: an exact hit that still interpolates at bary 0), and for every third key three ulps below k/30 (bary
    rounding up to 1.0f);
  * halves of a second, where time * 30 is an exact integer (1.5 s -> frame 45).

Local poses and morph rates come from libmmd's Motion::GetBonePose / GetMorphPose(name, double time)
(tests/motion_time_driver.cpp); palettes from those poses through libmmd's own bone solve on the rig_small skeleton
(oracle.pyoracle.Reference.skeleton).  Needs the reference's headers and oracle/_ref (built by oracle/Makefile):
    python -m tests.gen_motion_time_golden
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle.pyoracle import Reference  # noqa: E402
from simple_mmd_renderer_amd import vmd  # noqa: E402
from tests import golden_util as gu  # noqa: E402
from tests import motion_time_ref as mt  # noqa: E402


def key_frames():
    """Every key frame of every track of the two motions, ascending."""
    ks = set()
    bv, mv = vmd.Vmd(mt.BONE_VMD), vmd.Vmd(mt.MORPH_VMD)
    for fr, _, _, _ in mt.tracks_of(bv).values():
        ks.update(int(f) for f in fr)
    for i in range(len(mv.morph_track_names)):
        ks.update(int(f) for f in mv.morph_track(i)[0])
    bv.close(); mv.close()
    return sorted(ks)


def fixture_times():
    keys = key_frames()
    span_s = (max(keys) + 12) / 30.0                            # the whole span and a bit past its end
    t = [-1.0, -0.0, 0.0, -np.inf, np.inf, 1e300]
    t += [n / 60.0 for n in range(0, int(span_s * 60) + 1, 5)]
    t += [n / 144.0 for n in range(0, int(span_s * 144) + 1, 13)]
    for j, k in enumerate(keys):
        x = k / 30.0
        t += [x, np.nextafter(x, -np.inf), np.nextafter(x, np.inf)]
        if j % 3 == 0:
            y = x
            for _ in range(3):
                y = np.nextafter(y, -np.inf)
            t.append(y)                                         # three ulps below: bary rounds to 1.0f
    t += [h / 2.0 for h in range(0, int(span_s * 2) + 1)]      # time * 30 exact: 1.5 -> 45
    out = []
    for x in t:                                                 # keep the first occurrence, bit for bit (-0.0 != 0.0)
        if not any(np.float64(x).tobytes() == np.float64(y).tobytes() for y in out):
            out.append(x)
    return np.array(out, np.float64)


def main():
    zr = np.load(os.path.join(gu.GOLDEN_DIR, "rig_small_expect.npz"))
    zv = np.load(os.path.join(gu.GOLDEN_DIR, "vmd_small_expect.npz"))
    bone_names = [str(n) for n in zr["model_bone_names"]]
    morph_names = [str(n) for n in zv["model_morph_names"]]
    times = fixture_times()
    poses, rates = mt.driver_expect(mt.BONE_VMD, bone_names, mt.MORPH_VMD, morph_names, times)
    rsk = Reference.skeleton(zr["rest"], zr["parent"], zr["level"], zr["flags"])
    pals = np.stack([rsk.solve(poses[i]) for i in range(times.size)])
    rsk.close()
    np.savez_compressed(mt.FIXTURE, times=times, bone_names=np.array(bone_names), morph_names=np.array(morph_names),
                        rest=zr["rest"], parent=zr["parent"], level=zr["level"], flags=zr["flags"],
                        expect_rates=rates, expect_poses=poses, expect_palettes=pals)
    print("%s: %d times, %.1f KB" % (os.path.basename(mt.FIXTURE), times.size, os.path.getsize(mt.FIXTURE) / 1024))


if __name__ == "__main__":
    main()

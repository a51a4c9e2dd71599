"""Generate tests/golden/rig_blend_b.vmd and tests/golden/motion_blend_expect.npz: the cross-fade between two clips (include/mmdx.h,
mmdx_motion_blend_args) as the real libmmd computes it.

Clip 0 is the committed rig_small.vmd (bone tracks) / vmd_small.vmd (morph tracks); clip 1, rig_blend_b.vmd, is a second motion
over the same bone and morph names written by the project's own vmd.write_vmd (several keys per track, other frames, other
curves, rotations from both hemispheres).  Rows: every weight of motion_blend_ref.WEIGHTS for every pair of
motion_blend_ref.PAIRS, four (time a, time b) each, the times spanning both clips and past their ends, with key frames k/30 of
both clips and their neighbouring doubles among them.

Local poses and rates come from tests/motion_blend_driver.cpp (libmmd's GetBonePose / GetMorphPose, NLerp and lerp expressions);
palettes from those poses through libmmd's own bone solve on the rig_small skeleton (oracle.pyoracle.Reference.skeleton).  Needs
the reference's headers and oracle/_ref (built by oracle/Makefile):
    python -m tests.gen_motion_blend_golden
"""
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle.pyoracle import Reference  # noqa: E402
from simple_mmd_renderer_amd import synth, vmd  # noqa: E402
from tests import golden_util as gu  # noqa: E402
from tests import motion_blend_ref as mb  # noqa: E402
from tests import motion_time_ref as mt  # noqa: E402

ROWS_PER_CASE = 4


def write_clip_b(bone_tracks, morph_tracks):
    """The second clip: 5 keys per bone over 150 frames, 4 keys per morph; every other key of every third bone negated -- the same
    rotation, the other hemisphere -- so that both signs of A.q . B.q occur whatever the writer's random rotations do."""
    keys = synth.make_bone_keys(bone_tracks, 2026, keys_per=5, span=150)
    flipped = []
    for j, (name, frame, t, q, interp) in enumerate(keys):
        if bone_tracks.index(name) % 3 == 0 and j % 2 == 0:
            q = tuple(-float(x) for x in q)
        flipped.append((name, frame, t, q, interp))
    rng = np.random.RandomState(2027)
    morphs = [(n, int(f), float(np.float32(rng.uniform(0, 1)))) for n in morph_tracks for f in (0, 17, 61, 140)]
    data = vmd.write_vmd(flipped, morphs)
    with open(mb.CLIP_B_VMD, "wb") as f:
        f.write(data)
    return data


def key_frames():
    ks = []
    for path in (mt.BONE_VMD, mb.CLIP_B_VMD):
        v = vmd.Vmd(path)
        s = set()
        for fr, _, _, _ in mt.tracks_of(v).values():
            s.update(int(f) for f in fr)
        for i in range(len(v.morph_track_names)):
            s.update(int(f) for f in v.morph_track(i)[0])
        v.close()
        ks.append(sorted(s))
    return ks


def fixture_times():
    """Times spanning both clips: before the start, display-rate instants, past the end, and for a few key frames k of either
    clip k/30 with the doubles on both sides."""
    ka, kb = key_frames()
    span = (max(ka + kb) + 12) / 30.0
    t = [-1.0, 0.0, np.inf]
    t += [n / 60.0 for n in range(1, int(span * 60), 23)]
    t += [n / 144.0 for n in range(1, int(span * 144), 61)]
    for k in ka[1:-1][::max(1, len(ka) // 4)][:4] + kb[1:-1][::max(1, len(kb) // 4)][:4]:
        x = k / 30.0
        t += [x, np.nextafter(x, -np.inf), np.nextafter(x, np.inf)]
    return np.array(t, np.float64)


def cases():
    t = fixture_times()
    # both strides coprime to the table size: each side walks the whole table before it repeats a time
    sa, sb = (next(s for s in range(s0, s0 + t.size) if math.gcd(s, t.size) == 1) for s0 in (5, 11))
    ca, cb, ta, tb, w = [], [], [], [], []
    r = 0
    for weight in mb.WEIGHTS:
        for a, b in mb.PAIRS:
            for _ in range(ROWS_PER_CASE):
                ca.append(a); cb.append(b); w.append(weight)
                ta.append(t[(r * sa + 1) % t.size])
                tb.append(t[(r * sb + 3) % t.size])
                r += 1
    return (np.array(ca, np.uint32), np.array(ta, np.float64), np.array(cb, np.uint32), np.array(tb, np.float64),
            np.array(w, np.float32))


def main():
    zr = np.load(os.path.join(gu.GOLDEN_DIR, "rig_small_expect.npz"))
    zv = np.load(os.path.join(gu.GOLDEN_DIR, "vmd_small_expect.npz"))
    bone_names = [str(n) for n in zr["model_bone_names"]]
    morph_names = [str(n) for n in zv["model_morph_names"]]
    v0, m0 = vmd.Vmd(mt.BONE_VMD), vmd.Vmd(mt.MORPH_VMD)
    write_clip_b(list(v0.bone_track_names), list(m0.morph_track_names))
    v0.close(); m0.close()
    ca, ta, cb, tb, w = cases()
    poses, rates = mb.driver_expect(mb.BONE_VMDS, bone_names, mb.MORPH_VMDS, morph_names, ca, ta, cb, tb, w)
    rsk = Reference.skeleton(zr["rest"], zr["parent"], zr["level"], zr["flags"])
    pals = np.stack([rsk.solve(poses[i]) for i in range(w.size)])
    rsk.close()
    z = dict(clips_a=ca, clips_b=cb, times_a=ta, times_b=tb, weights=w, bone_names=np.array(bone_names),
             morph_names=np.array(morph_names), expect_poses=poses, expect_rates=rates, expect_palettes=pals)
    # the unblended rows of both sides, from libmmd as well (weight 0: the row is A): what the coverage is counted on
    zero = np.zeros_like(w)
    a_rows, _ = mb.driver_expect(mb.BONE_VMDS, bone_names, mb.MORPH_VMDS, morph_names, ca, ta, ca, ta, zero)
    b_rows, _ = mb.driver_expect(mb.BONE_VMDS, bone_names, mb.MORPH_VMDS, morph_names, cb, tb, cb, tb, zero)
    mb.check_coverage(z, a_rows, b_rows)
    np.savez_compressed(mb.FIXTURE, **z)
    print("%s: %d rows, %.1f KB; %s: %.1f KB" % (os.path.basename(mb.FIXTURE), w.size, os.path.getsize(mb.FIXTURE) / 1024,
                                                 os.path.basename(mb.CLIP_B_VMD), os.path.getsize(mb.CLIP_B_VMD) / 1024))


if __name__ == "__main__":
    main()

"""Time-based motion evaluation (MotionPlayer::SeekTime): the checkers the tests and the fixture generator share.

  * the REAL libmmd, Motion::GetBonePose / GetMorphPose(name, double time), through tests/motion_time_driver.cpp --
    compiled with g++ where the reference's headers are present (they are not on the GPU machines);
  * a from-scratch restatement of the same (tests/motion_time_restate.c, gcc at test time), for randomized tests
    anywhere;
  * the fixture tests/golden/motion_time_expect.npz (tests/gen_motion_time_golden.py) and its inputs.
Nothing compiled here is committed: both libraries are built by tests/host_program.py.
"""
import ctypes as C
import os

import numpy as np

from tests import golden_util as gu
from tests import host_program as hp

HERE, REF_INC, driver_available = hp.TESTS, hp.REF_INC, hp.reference_available          # what callers took from here before
FIXTURE = os.path.join(gu.GOLDEN_DIR, "motion_time_expect.npz")
MORPH_VMD = os.path.join(gu.GOLDEN_DIR, "vmd_small.vmd")
BONE_VMD = os.path.join(gu.GOLDEN_DIR, "rig_small.vmd")


def ptr(a, t):
    return a.ctypes.data_as(C.POINTER(t))


# ---- the real libmmd ------------------------------------------------------------------------------
def build_driver() -> str:
    return hp.build("motion_time_driver", [os.path.join(HERE, "motion_time_driver.cpp")], strict=False, shared=True, include=[REF_INC])


class Driver:
    """libmmd's VmdReader + Motion of one .vmd, evaluated at times in seconds."""

    def __init__(self, vmd_path: str):
        self.lib = C.CDLL(build_driver())
        self.lib.mtd_load.restype = C.c_void_p
        h = self.lib.mtd_load(str(vmd_path).encode())
        if not h:
            raise RuntimeError("libmmd VmdReader failed on " + str(vmd_path))
        self.h = C.c_void_p(h)

    def bone_poses(self, name: str, times):
        """GetBonePose(name, t) for every t -> f32 [T, 8], or None without such a track."""
        t = np.ascontiguousarray(times, np.float64).reshape(-1)
        out = np.zeros((t.size, 8), np.float32)
        try:
            sj = name.encode("shift_jis")
        except UnicodeEncodeError:
            return None
        ok = self.lib.mtd_bone_poses_time(self.h, sj, C.c_uint32(t.size), ptr(t, C.c_double), ptr(out, C.c_float))
        return out if ok else None

    def morph_weights(self, name: str, times):
        """GetMorphPose(name, t) for every t -> f32 [T], or None without such a track."""
        t = np.ascontiguousarray(times, np.float64).reshape(-1)
        out = np.zeros(t.size, np.float32)
        try:
            sj = name.encode("shift_jis")
        except UnicodeEncodeError:
            return None
        ok = self.lib.mtd_morph_weights_time(self.h, sj, C.c_uint32(t.size), ptr(t, C.c_double), ptr(out, C.c_float))
        return out if ok else None

    def close(self):
        if self.h:
            self.lib.mtd_destroy(self.h)
            self.h = None


def driver_expect(bone_vmd, bone_names, morph_vmd, morph_names, times):
    """What MotionPlayer::SeekTime leaves in the poser, per model bone / morph: poses f32 [T, NB, 8] (untracked bones:
    ResetPosing's zero translation and identity rotation) and rates f32 [T, NM] (untracked morphs: 0)."""
    t = np.ascontiguousarray(times, np.float64).reshape(-1)
    poses = np.zeros((t.size, len(bone_names), 8), np.float32)
    poses[:, :, 7] = 1.0
    d = Driver(bone_vmd)
    for j, n in enumerate(bone_names):
        p = d.bone_poses(n, t)
        if p is not None:
            poses[:, j] = p
    d.close()
    rates = np.zeros((t.size, len(morph_names)), np.float32)
    d = Driver(morph_vmd)
    for j, n in enumerate(morph_names):
        w = d.morph_weights(n, t)
        if w is not None:
            rates[:, j] = w
    d.close()
    return poses, rates


# ---- the restatement ------------------------------------------------------------------------------
def restatement():
    return C.CDLL(hp.build("motion_time_restate", [os.path.join(HERE, "motion_time_restate.c")], cxx=False, c_std="gnu11", strict=False,
                           shared=True, link=["-lm"]))


def tracks_of(v):
    """name -> (frames u32[K], tr f32[K,3], rot f32[K,4], interp i8[K,64]) of a parsed simple_mmd_renderer_amd.vmd.Vmd."""
    out = {}
    for i, n in enumerate(v.bone_track_names):
        ks = v.bone_track(i)
        out[n] = (np.array([k["frame"] for k in ks], np.uint32),
                  np.array([k["translation"] for k in ks], np.float32).reshape(-1, 3),
                  np.array([k["rotation"] for k in ks], np.float32).reshape(-1, 4),
                  np.frombuffer(b"".join(k["interpolation"] for k in ks), np.uint8).view(np.int8).reshape(-1, 64))
    return out


def morph_keys_of(v, model_names):
    """(key_off, frames, weights) in model-morph order, as mmdx_vmd_bind_morphs builds them."""
    tracks = {n: v.morph_track(i) for i, n in enumerate(v.morph_track_names)}
    off, fr, w = [0], [], []
    for n in model_names:
        if n in tracks:
            fr += list(tracks[n][0])
            w += list(tracks[n][1])
        off.append(len(fr))
    return np.asarray(off, np.uint32), np.asarray(fr, np.uint32), np.asarray(w, np.float32)


def restate_poses(v, bone_names, times):
    """The restatement of GetBonePose(name, t) per model bone -> f32 [T, NB, 8]."""
    lib = restatement()
    tr = tracks_of(v)
    t = np.ascontiguousarray(times, np.float64).reshape(-1)
    out = np.zeros((t.size, len(bone_names), 8), np.float32)
    one = np.zeros(8, np.float32)
    dummy = (np.zeros(1, np.uint32), np.zeros((1, 3), np.float32), np.zeros((1, 4), np.float32), np.zeros((1, 64), np.int8))
    for j, n in enumerate(bone_names):
        k = tr.get(n)
        nk = 0 if k is None else k[0].size
        fr, tt, rot, ip = [np.ascontiguousarray(a) for a in (k if nk else dummy)]
        for i, x in enumerate(t):
            lib.mt_bone_pose_time(C.c_uint32(nk), ptr(fr, C.c_uint32), ptr(tt, C.c_float), ptr(rot, C.c_float), ptr(ip, C.c_int8),
                                  C.c_double(float(x)), ptr(one, C.c_float))
            out[i, j] = one
    return out


def restate_rates(v, morph_names, times):
    """The restatement of GetMorphPose(name, t) per model morph -> f32 [T, NM]."""
    lib = restatement()
    off, fr, w = morph_keys_of(v, morph_names)
    if fr.size == 0:
        fr, w = np.zeros(1, np.uint32), np.zeros(1, np.float32)
    t = np.ascontiguousarray(times, np.float64).reshape(-1)
    out = np.zeros((t.size, len(morph_names)), np.float32)
    lib.mt_morph_tracks_time(C.c_uint32(len(morph_names)), ptr(off, C.c_uint32), ptr(fr, C.c_uint32), ptr(w, C.c_float),
                             C.c_uint32(t.size), ptr(t, C.c_double), ptr(out, C.c_float))
    return out


# ---- the fixture ----------------------------------------------------------------------------------
def fixture():
    """dict: times f64 [T], bone_names [NB], morph_names [NM], rest / parent / level / flags (the rig_small skeleton),
    expect_rates f32 [T, NM], expect_poses f32 [T, NB, 8], expect_palettes f32 [T, NB, 16]."""
    z = np.load(FIXTURE)
    out = {k: z[k] for k in z.files}
    out["bone_names"] = [str(n) for n in z["bone_names"]]
    out["morph_names"] = [str(n) for n in z["morph_names"]]
    return out

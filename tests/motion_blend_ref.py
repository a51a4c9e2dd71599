"""Cross-fade between two clips of a motion set (include/mmdx.h, mmdx_motion_blend_args): the checkers the tests and the fixture
generator share.

  * a numpy float32 restatement of the blend (blend_poses / blend_rates): the row-level short circuits, the per-channel
    l*(1-w) + r*w and NLerp's middle branch, one rounding per operation, the normalisation through double;
  * the REAL libmmd through tests/motion_blend_driver.cpp -- compiled with g++ where the reference's headers are present (they
    are not on the GPU machines);
  * the fixture tests/golden/motion_blend_expect.npz (tests/gen_motion_blend_golden.py) and its inputs.
Nothing compiled here is committed.
"""
import ctypes as C
import os

import numpy as np

from tests import golden_util as gu
from tests import host_program as hp
from tests import motion_time_ref as mt

FIXTURE = os.path.join(gu.GOLDEN_DIR, "motion_blend_expect.npz")
CLIP_B_VMD = os.path.join(gu.GOLDEN_DIR, "rig_blend_b.vmd")          # clip 1: bone and morph tracks in one file
BONE_VMDS = (mt.BONE_VMD, CLIP_B_VMD)                                 # clip 0, clip 1
MORPH_VMDS = (mt.MORPH_VMD, CLIP_B_VMD)
NONE = 0xFFFFFFFF                                                     # MMDX_CLIP_NONE
REST_POSE = np.array([0, 0, 0, 0, 0, 0, 0, 1], np.float32)           # Poser::ResetPosing
EPS = np.float32(1e-7)
ONE = np.float32(1.0)
# the weights the issue sets, as the float32 the entry points take; classes by NLerp's short circuits
WEIGHTS = np.array([0.0, 5e-8, 1e-7, 0.25, 0.5, np.float32(1.0) - np.float32(1e-7), 1 - 5e-8, 1.0, -1.0, 2.0], np.float32)
PAIRS = ((0, 1), (1, 0), (0, 0), (NONE, 1), (0, NONE))


def side_of(w):
    """0: the row is A (anything that is not >= 1e-7f, NaN included), 1: the row is B (> 1.0f - 1e-7f), 2: blended."""
    w = np.asarray(w, np.float32)
    with np.errstate(invalid="ignore"):
        return np.where(~(w >= EPS), 0, np.where(w > ONE - EPS, 1, 2)).astype(np.uint32)


def blend_rates(a, b, w):
    """a, b f32 [N, NM], w f32 [N] -> [N, NM]."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    w = np.asarray(w, np.float32).reshape(-1, 1)
    side = side_of(w)
    with np.errstate(all="ignore"):
        mix = a * (ONE - w) + b * w
    return np.where(side == 0, a, np.where(side == 1, b, mix)).astype(np.float32)


def blend_poses(a, b, w):
    """a, b f32 [N, NB, 8] (t.xyz, 0, q.xyzw), w f32 [N] -> [N, NB, 8]."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    w = np.asarray(w, np.float32).reshape(-1, 1, 1)
    side = side_of(w)
    with np.errstate(all="ignore"):
        out = np.zeros_like(a)
        out[..., :3] = a[..., :3] * (ONE - w) + b[..., :3] * w
        qa, qb = a[..., 4:], b[..., 4:]
        dot = qa[..., 0] * qb[..., 0] + qa[..., 1] * qb[..., 1] + qa[..., 2] * qb[..., 2] + qa[..., 3] * qb[..., 3]   # left to right
        k = ONE - w
        v = np.where((dot < 0)[..., None], k * qa - w * qb, k * qa + w * qb)
        s = v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1] + v[..., 2] * v[..., 2] + v[..., 3] * v[..., 3]
        n = ONE / np.sqrt(s.astype(np.float64)).astype(np.float32)                                                    # Vector4D::Normalize
        out[..., 4:] = v * n[..., None]
    return np.where(side == 0, a, np.where(side == 1, b, out)).astype(np.float32)


def quaternion_dots(a, b):
    """A.q . B.q per (row, bone), the float32 sum the blend takes its sign from."""
    qa, qb = np.asarray(a, np.float32)[..., 4:], np.asarray(b, np.float32)[..., 4:]
    return qa[..., 0] * qb[..., 0] + qa[..., 1] * qb[..., 1] + qa[..., 2] * qb[..., 2] + qa[..., 3] * qb[..., 3]


def pick(rows_per_clip, clips, rest):
    """rows_per_clip [n_clips][N, ...] -> the row of clips[i] for every i, `rest` for ids outside the bank."""
    rows = np.stack(rows_per_clip)
    clips = np.asarray(clips, np.uint32)
    n = clips.size
    valid = clips < rows.shape[0]
    got = rows[np.where(valid, clips, 0), np.arange(n)]
    return np.where(valid.reshape((n,) + (1,) * (got.ndim - 1)), got, rest).astype(np.float32)


def check_coverage(z, a_rows, b_rows):
    """Among the blended (row, bone) pairs both signs of A.q . B.q occur at least 8 times, and every weight occurs."""
    mix = side_of(z["weights"]) == 2
    dots = quaternion_dots(a_rows, b_rows)[mix]
    assert (dots < 0).sum() >= 8 and (dots >= 0).sum() >= 8, ((dots < 0).sum(), (dots >= 0).sum())
    for weight in WEIGHTS:
        assert (z["weights"].view(np.uint32) == np.float32(weight).view(np.uint32)).sum() >= len(PAIRS), weight
    assert {(int(a), int(b)) for a, b in zip(z["clips_a"], z["clips_b"])} == set(PAIRS)


# ---- the real libmmd ------------------------------------------------------------------------------
def build_driver() -> str:
    return hp.build("motion_blend_driver", [os.path.join(hp.TESTS, "motion_blend_driver.cpp")], strict=False, shared=True,
                    include=[hp.REF_INC])


def driver_expect(bone_vmds, bone_names, morph_vmds, morph_names, clips_a, times_a, clips_b, times_b, weights):
    """The blended rows by libmmd's own GetBonePose / GetMorphPose, NLerp and lerp expressions -> poses f32 [N, NB, 8] and rates
    f32 [N, NM].  bone_vmds / morph_vmds: one .vmd path per clip."""
    lib = C.CDLL(build_driver())
    lib.mbd_load.restype = C.c_void_p
    ca, cb = np.ascontiguousarray(clips_a, np.uint32), np.ascontiguousarray(clips_b, np.uint32)
    ta, tb = np.ascontiguousarray(times_a, np.float64), np.ascontiguousarray(times_b, np.float64)
    w = np.ascontiguousarray(weights, np.float32)
    n = w.size

    def run(fn, paths, names, width):
        hs = [lib.mbd_load(str(p).encode()) for p in paths]
        if not all(hs):
            raise RuntimeError("libmmd VmdReader failed on one of " + repr(paths))
        arr = (C.c_void_p * len(hs))(*hs)
        out = np.zeros((n, len(names)) + ((width,) if width > 1 else ()), np.float32)
        one = np.zeros((n, width), np.float32)
        for j, name in enumerate(names):
            fn(arr, C.c_uint32(len(hs)), name.encode("shift_jis"), C.c_uint32(n), mt.ptr(ca, C.c_uint32), mt.ptr(ta, C.c_double),
               mt.ptr(cb, C.c_uint32), mt.ptr(tb, C.c_double), mt.ptr(w, C.c_float), mt.ptr(one, C.c_float))
            out[:, j] = one if width > 1 else one[:, 0]
        for h in hs:
            lib.mbd_destroy(C.c_void_p(h))
        return out
    return run(lib.mbd_blend_bone, bone_vmds, bone_names, 8), run(lib.mbd_blend_morph, morph_vmds, morph_names, 1)


# ---- the fixture ----------------------------------------------------------------------------------
def fixture():
    """dict: clips_a / clips_b u32 [N], times_a / times_b f64 [N], weights f32 [N], bone_names [NB], morph_names [NM],
    expect_poses f32 [N, NB, 8], expect_rates f32 [N, NM], expect_palettes f32 [N, NB, 16] (the rig_small skeleton of
    tests/golden/rig_small_expect.npz)."""
    z = np.load(FIXTURE)
    out = {k: z[k] for k in z.files}
    out["bone_names"] = [str(n) for n in z["bone_names"]]
    out["morph_names"] = [str(n) for n in z["morph_names"]]
    return out

"""Motion sets: mmdx_motion_set_* and mmdx_skeleton_solve_motion_set* -- every instance of a crowd plays its own clip
(in the reference every Poser has its own MotionPlayer over whichever Motion it likes, L/motion/poser_impl.inl:522-555).

The result for instance i is, bit for bit, what the single-motion entry point returns for clip clips[i] at frames[i] / times[i]:
the checkers are the single-motion entry points themselves (pinned against libmmd elsewhere), the restatement
tests/motion_time_ref.py and oracle.pyoracle.  CPU tests cover the symbols, the host-side concatenation (mmdx_motion_set_get_info)
and every argument check that needs no device; GPU tests compare through the C ABI with no tolerance.
"""
import os
import subprocess

import numpy as np
import pytest

from simple_mmd_renderer_amd import _capi as api
from simple_mmd_renderer_amd import synth, vmd
from simple_mmd_renderer_amd.engine import DeformModel, DeviceBuffer
from tests import golden_util as gu
from tests import motion_time_ref as mt
from tests.test_capi_symbols import declared_symbols
from tests.test_motion_time import key_frames_of, random_motion, random_times

SET_ENTRY_POINTS = ("mmdx_motion_set_create", "mmdx_motion_set_get_info", "mmdx_motion_set_destroy",
                    "mmdx_motion_set_eval_bones", "mmdx_motion_set_eval_bones_time", "mmdx_motion_set_eval_morphs",
                    "mmdx_motion_set_eval_morphs_time", "mmdx_skeleton_solve_motion_set", "mmdx_skeleton_solve_motion_set_time")
NONE = vmd.CLIP_NONE
REST_POSE = np.array([0, 0, 0, 0, 0, 0, 0, 1], np.float32)          # Poser::ResetPosing


@pytest.fixture(autouse=True)
def _lib(hip_lib):
    return hip_lib


# ---------------------------------------------------------------------------------------- CPU ----
def test_set_entry_points_are_declared_exported_and_bound(hip_lib):
    syms = declared_symbols()
    for name in SET_ENTRY_POINTS:
        assert name in syms and hasattr(hip_lib, name) and name in api.SIGNATURES, name
    hdr = open(os.path.join(os.path.dirname(mt.HERE), "include", "mmdx.h")).read()
    assert "MMDX_CLIP_NONE = 0xFFFFFFFFu" in hdr and "#define MMDX_ABI_VERSION 3u" in hdr
    assert hip_lib.mmdx_abi_version() == 3
    assert vmd.CLIP_NONE == 0xFFFFFFFF


def _handles(ms):
    import ctypes as C
    return (C.c_void_p * len(ms))(*[m.h if m is not None else None for m in ms])


def test_create_refuses_bad_clip_lists_and_reports_the_sums():
    import ctypes as C
    lib = api.lib()
    names = [f"bone{i}" for i in range(41)]
    mnames = ["m0", "m1", "m2"]
    vs = [vmd.Vmd(random_motion(seed, names[:30 + seed], mnames)) for seed in range(3)]
    bms = [v.bind_bones(names[:40]) for v in vs]
    mms = [v.bind_morphs(mnames) for v in vs]
    bm41 = vs[0].bind_bones(names)
    mm2 = vs[0].bind_morphs(mnames[:2])
    h = C.c_void_p()
    assert lib.mmdx_motion_set_create(0, _handles(bms), _handles(mms), C.byref(h)) == 1                 # no clips
    assert lib.mmdx_motion_set_create(3, None, None, C.byref(h)) == 1                                   # neither side
    assert lib.mmdx_motion_set_create(3, _handles(bms), _handles(mms), None) == 1                       # nowhere to put it
    assert lib.mmdx_motion_set_create(3, _handles([bms[0], None, bms[2]]), None, C.byref(h)) == 1       # a NULL element
    assert "NULL" in lib.mmdx_last_error_string().decode()
    assert lib.mmdx_motion_set_create(3, None, _handles([mms[0], mms[1], None]), C.byref(h)) == 1
    assert lib.mmdx_motion_set_create(3, _handles([bms[0], bm41, bms[2]]), None, C.byref(h)) == 1       # 40 vs 41 bones
    assert "40" in lib.mmdx_last_error_string().decode() and "41" in lib.mmdx_last_error_string().decode()
    assert lib.mmdx_motion_set_create(3, None, _handles([mms[0], mm2, mms[2]]), C.byref(h)) == 1        # 3 vs 2 morphs
    assert not h.value
    with pytest.raises(api.MmdxError):
        vmd.MotionSet()
    ms = vmd.MotionSet(bms, mms)
    assert ms.info["n_clips"] == 3 and ms.info["n_bones"] == 40 and ms.info["n_morphs"] == 3
    assert ms.info["n_bone_keys"] == sum(b.n_keys for b in bms) > 0
    assert ms.info["n_morph_keys"] == sum(m.n_keys for m in mms) > 0
    assert 0 < max(b.n_curves for b in bms) <= ms.info["n_curves"] <= sum(b.n_curves for b in bms)
    # the same clip three times: every curve table is byte-identical to the first clip's, so it is stored once
    same = vmd.MotionSet([bms[1]] * 3)
    assert same.info["n_curves"] == bms[1].n_curves and same.info["n_bone_keys"] == 3 * bms[1].n_keys
    assert same.info["n_morphs"] == 0 and same.info["n_morph_keys"] == 0
    only_morphs = vmd.MotionSet(morph_motions=mms)
    assert only_morphs.info["n_bones"] == 0 and only_morphs.info["n_bone_keys"] == 0 and only_morphs.info["n_curves"] == 0
    bad = vmd.MotionSetInfo()
    assert lib.mmdx_motion_set_get_info(ms.h, C.byref(bad)) == 1 and lib.mmdx_motion_set_get_info(None, C.byref(bad)) == 1
    for x in [ms, same, only_morphs, bm41, mm2] + bms + mms + vs:
        x.close()
    lib.mmdx_motion_set_destroy(None)


def test_set_entry_points_refuse_bad_arguments():
    """Everything that needs no device is decided before the first HIP call, so it is checked here without a GPU."""
    lib = api.lib()
    names = ["センター", "首"]
    v = vmd.Vmd(vmd.write_vmd(synth.make_bone_keys(names, 1, keys_per=3), [("あ", 0, 0.5), ("あ", 9, 1.0)]))
    bm, mm = v.bind_bones(names), v.bind_morphs(["あ"])
    both = vmd.MotionSet([bm, bm], [mm, mm])
    bones_only, morphs_only = vmd.MotionSet([bm, bm]), vmd.MotionSet(morph_motions=[mm, mm])
    sk = vmd.Skeleton(*synth.make_skeleton(2, 1))
    sk3 = vmd.Skeleton(*synth.make_skeleton(3, 1))
    c = np.array([0, NONE], np.uint32)
    c_bad = np.array([1, 2], np.uint32)                     # 2 == n_clips
    fr = np.array([3, 4], np.uint32)
    t = np.array([0.5, 1.0], np.float64)
    tn = np.array([0.5, np.nan], np.float64)
    out = np.zeros((2, 2, 16), np.float32)
    o = out.ctypes.data

    def entry(fn, skeleton=None):
        if skeleton is None:
            return lambda s, cp, kp, f, op=o, n=2: fn(s, None, n, cp, kp, f, op)
        return lambda s, cp, kp, f, op=o, n=2, k=skeleton: fn(k, s, None, n, cp, kp, f, op)
    calls = {   # name -> (call, host clock, is the time form, set lacking the side)
        "bones": (entry(lib.mmdx_motion_set_eval_bones), fr, False, morphs_only),
        "bones_time": (entry(lib.mmdx_motion_set_eval_bones_time), t, True, morphs_only),
        "morphs": (entry(lib.mmdx_motion_set_eval_morphs), fr, False, bones_only),
        "morphs_time": (entry(lib.mmdx_motion_set_eval_morphs_time), t, True, bones_only),
        "solve": (entry(lib.mmdx_skeleton_solve_motion_set, sk.h), fr, False, morphs_only),
        "solve_time": (entry(lib.mmdx_skeleton_solve_motion_set_time, sk.h), t, True, morphs_only),
    }
    err = lambda: lib.mmdx_last_error_string().decode()          # noqa: E731
    for what, (call, clock, is_time, lacking) in calls.items():
        cp, kp = c.ctypes.data, clock.ctypes.data
        assert call(None, cp, kp, 0) == 1, what                                     # NULL set
        assert call(both.h, None, kp, 0) == 1, what                                 # NULL clips
        assert call(both.h, cp, None, 0) == 1, what                                 # NULL frames / times
        assert call(both.h, cp, kp, 0, op=None) == 1, what                          # NULL output
        assert call(both.h, cp, kp, 0, n=0) == 1, what                              # no instances
        for bad in (1 << 1, 1 << 3, 1 << 4, 1 << 31):
            assert call(both.h, cp, kp, bad) == 1 and "unknown flag" in err(), (what, bad)
        assert call(both.h, c_bad.ctypes.data, kp, 0) == 2 and "clips[1]" in err(), what          # MMDX_ERR_BAD_INDEX
        assert call(both.h, c_bad.ctypes.data, kp, api.OUT_ON_DEVICE) == 2, what
        assert call(lacking.h, cp, kp, 0) == 1 and "created without" in err(), what
        if is_time:
            assert call(both.h, cp, tn.ctypes.data, 0) == 1 and "NaN" in err(), what
            assert call(both.h, cp, tn.ctypes.data, api.OUT_ON_DEVICE) == 1, what
    for fn, clock in ((lib.mmdx_skeleton_solve_motion_set, fr), (lib.mmdx_skeleton_solve_motion_set_time, t)):
        assert fn(None, both.h, None, 2, c.ctypes.data, clock.ctypes.data, 0, o) == 1                     # NULL skeleton
        assert fn(sk3.h, both.h, None, 2, c.ctypes.data, clock.ctypes.data, 0, o) == 1 and "3" in err()  # another bone count
    with pytest.raises(api.MmdxError) as e:
        both.eval_bones_time([0, 1], [0.0, float("nan")])
    assert e.value.status == 1
    with pytest.raises(api.MmdxError) as e:
        sk.solve_motion_set(both, [0, 7], [1, 2])
    assert e.value.status == 2
    for x in (both, bones_only, morphs_only, sk, sk3, bm, mm, v):
        x.close()


# ---------------------------------------------------------------------------------------- GPU ----
NB = 40
NAMES = [f"bone{i}" for i in range(NB)]
MNAMES = [f"m{i}" for i in range(5)] + ["none"]
_cache = {}


def _mixed_crowd():
    """Four clips over 40 bones (a wave of the track kernels holds two instances with different clips) and 5 morphs plus one
    unbound: seeds 0-2 bound to different bone subsets (different key counts, bones keyed in one clip only), the fourth without
    a single record.  ~250 instances at corner times, the keys' exact and adjacent times and a NaN; clip ids cycle through the
    four clips, MMDX_CLIP_NONE and n_clips + 5.  Computed once: the restated poses / rates of every clip at every time."""
    if "mixed" in _cache:
        return _cache["mixed"]
    subsets = [NAMES[:33], NAMES[5:], NAMES[::2]]
    data = [random_motion(seed, sub, MNAMES[:5]) for seed, sub in enumerate(subsets)] + [vmd.write_vmd([], [])]
    vs = [vmd.Vmd(d) for d in data]
    keys = sorted({k for v in vs for k in key_frames_of(v)})
    t = np.r_[random_times(100, keys[::3][:40], n=100), np.nan]
    n = t.size
    frames = np.clip(np.nan_to_num(t * 30.0, nan=0.0, posinf=2.0 ** 32 - 1, neginf=0.0), 0, 2.0 ** 32 - 1).astype(np.uint32)
    frames[20:20 + 60] = np.array(keys[:60], np.uint32)                     # exact key hits of the frame path
    cycle = np.array([0, 1, 2, 3, NONE, 4 + 5], np.uint32)
    clips = cycle[np.arange(n) % cycle.size]
    clips[-1] = 1                                                           # the NaN plays a clip with keys
    poses = np.stack([mt.restate_poses(v, NAMES, t) for v in vs])           # [clip][instance][bone][8]
    rates = np.stack([mt.restate_rates(v, MNAMES, t) for v in vs])
    for v in vs:
        v.close()
    valid = clips < 4
    want_pose = np.where(valid[:, None, None], poses[np.minimum(clips, 3), np.arange(n)], REST_POSE)
    want_rate = np.where(valid[:, None], rates[np.minimum(clips, 3), np.arange(n)], np.float32(0))
    assert 200 <= n <= 270 and len({len(key_frames_of(vmd.Vmd(d))) for d in data}) == 4
    _cache["mixed"] = dict(data=data, t=t, frames=frames, clips=clips, valid=valid, want_pose=want_pose.astype(np.float32),
                           want_rate=want_rate.astype(np.float32), n=n)
    return _cache["mixed"]


def _open_clips(data):
    vs = [vmd.Vmd(d) for d in data]
    return vs, [v.bind_bones(NAMES) for v in vs], [v.bind_morphs(MNAMES) for v in vs]


def _close(*xs):
    for x in xs:
        for y in (x if isinstance(x, (list, tuple)) else [x]):
            y.free() if isinstance(y, DeviceBuffer) else y.close()


@pytest.mark.gpu
def test_gpu_set_equals_the_single_clip_calls_and_the_restatement():
    z = _mixed_crowd()
    n, t, frames, clips, valid = z["n"], z["t"], z["frames"], z["clips"], z["valid"]
    vs, bms, mms = _open_clips(z["data"])
    d_t, d_f, d_c = DeviceBuffer.from_numpy(t), DeviceBuffer.from_numpy(frames), DeviceBuffer.from_numpy(clips)
    d_pose, d_w = DeviceBuffer(n * NB * 32), DeviceBuffer(n * 6 * 4)
    # the single-clip device calls of every clip, time and frame forms: the rows the set has to reproduce
    single = {k: [] for k in ("pose_t", "pose_f", "rate_t", "rate_f")}
    for bm, mm in zip(bms, mms):
        bm.eval_time_device(n, d_t.ptr, d_pose.ptr)
        single["pose_t"].append(d_pose.download((n, NB, 8), np.float32))
        bm.eval_device(n, d_f.ptr, d_pose.ptr)
        single["pose_f"].append(d_pose.download((n, NB, 8), np.float32))
        mm.eval_time_device(n, d_t.ptr, d_w.ptr)
        single["rate_t"].append(d_w.download((n, 6), np.float32))
        mm.eval_device(n, d_f.ptr, d_w.ptr)
        single["rate_f"].append(d_w.download((n, 6), np.float32))
    ms = vmd.MotionSet(bms, mms)
    _close(bms, mms, vs)                                   # the set copied the tables: the clips and their files are gone
    assert ms.info["n_clips"] == 4 and ms.nb == NB and ms.nm == 6

    def pick(rows, rest):
        rows = np.stack(rows)[np.minimum(clips, 3), np.arange(n)]
        return np.where(valid.reshape((n,) + (1,) * (rows.ndim - 1)), rows, rest).astype(np.float32)
    got = {}
    for d in (d_pose, d_w):
        d.memset(0xFF)                                     # an unwritten row would show
    ms.eval_bones_time_device(n, d_c.ptr, d_t.ptr, d_pose.ptr)
    got["pose_t"] = d_pose.download((n, NB, 8), np.float32)
    ms.eval_morphs_time_device(n, d_c.ptr, d_t.ptr, d_w.ptr)
    got["rate_t"] = d_w.download((n, 6), np.float32)
    for d in (d_pose, d_w):
        d.memset(0xFF)
    ms.eval_bones_device(n, d_c.ptr, d_f.ptr, d_pose.ptr)
    got["pose_f"] = d_pose.download((n, NB, 8), np.float32)
    ms.eval_morphs_device(n, d_c.ptr, d_f.ptr, d_w.ptr)
    got["rate_f"] = d_w.download((n, 6), np.float32)
    for k in ("pose_t", "pose_f"):
        gu.assert_bits_equal(got[k], pick(single[k], REST_POSE), f"{k}: set vs the single-clip device calls")
        gu.assert_bits_equal(got[k][~valid], np.broadcast_to(REST_POSE, ((~valid).sum(), NB, 8)), f"{k}: NONE / out-of-range rows")
    for k in ("rate_t", "rate_f"):
        gu.assert_bits_equal(got[k], pick(single[k], np.float32(0)), f"{k}: set vs the single-clip device calls")
        gu.assert_bits_equal(got[k][~valid], np.zeros(((~valid).sum(), 6), np.float32), f"{k}: NONE / out-of-range rows")
    gu.assert_bits_equal(got["pose_t"], z["want_pose"], "poses vs the restatement")
    gu.assert_bits_equal(got["rate_t"], z["want_rate"], "rates vs the restatement")
    assert (~valid).sum() > 60 and valid.sum() > 120
    # host operands (valid ids and MMDX_CLIP_NONE; no NaN time) equal the device result
    host = np.flatnonzero((valid | (clips == NONE)) & ~np.isnan(t))
    gu.assert_bits_equal(ms.eval_bones_time(clips[host], t[host]), got["pose_t"][host], "poses (host operands, times)")
    gu.assert_bits_equal(ms.eval_bones(clips[host], frames[host]), got["pose_f"][host], "poses (host operands, frames)")
    gu.assert_bits_equal(ms.eval_morphs_time(clips[host], t[host]), got["rate_t"][host], "rates (host operands, times)")
    gu.assert_bits_equal(ms.eval_morphs(clips[host], frames[host]), got["rate_f"][host], "rates (host operands, frames)")
    _close(ms, d_t, d_f, d_c, d_pose, d_w)


@pytest.mark.gpu
def test_gpu_set_palettes_one_launch_and_two_launches(oracle):
    """The same instances through solve_motion_set_time_device on a parallel-FK skeleton (one launch) and on an IK / append rig
    (two launches): every third instance against the oracle solve of the restated poses, NONE rows against the solve of the rest
    pose, one frame-form run against solve_motion_device of every clip."""
    z = _mixed_crowd()
    n, t, frames, clips, valid = z["n"], z["t"], z["frames"], z["clips"], z["valid"]
    vs, bms, mms = _open_clips(z["data"])
    rest, parent, level, flags = synth.make_skeleton(NB, 3, 5, 0.25, 3)
    fk = vmd.Skeleton(rest, parent, level, flags)
    rig = synth.make_ik_rig(NB, 3, n_ik=3, n_append=4)
    ik = vmd.Skeleton(*rig)
    assert fk.info["solver"] == vmd.SOLVER_PARALLEL_FK and ik.info["solver"] == vmd.SOLVER_SERIAL
    d_t, d_f, d_c = DeviceBuffer.from_numpy(t), DeviceBuffer.from_numpy(frames), DeviceBuffer.from_numpy(clips)
    d_pal = DeviceBuffer(n * NB * 64)
    single = {"fk": [], "ik": []}
    for bm in bms:
        for name, sk in (("fk", fk), ("ik", ik)):
            sk.solve_motion_device(bm, n, d_f.ptr, d_pal.ptr)
            single[name].append(d_pal.download((n, NB, 16), np.float32))
    ms = vmd.MotionSet(bms)
    _close(bms, mms, vs)
    rest_pose = np.broadcast_to(REST_POSE, (NB, 8)).copy()
    want_rest = {"fk": oracle.bone_solve(rest, parent, rest_pose, level, flags),
                 "ik": oracle.bone_solve_full(rig[0], rig[1], rest_pose, rig[2], rig[3], rig[4], rig[5], rig[6])}
    for name, sk in (("fk", fk), ("ik", ik)):
        d_pal.memset(0xFF)
        sk.solve_motion_set_time_device(ms, n, d_c.ptr, d_t.ptr, d_pal.ptr)
        got = d_pal.download((n, NB, 16), np.float32)
        for i in list(range(0, n, 3)) + list(np.flatnonzero(~valid)[:8]):
            pose = z["want_pose"][i]
            want = (oracle.bone_solve(rest, parent, pose, level, flags) if name == "fk" else
                    oracle.bone_solve_full(rig[0], rig[1], pose, rig[2], rig[3], rig[4], rig[5], rig[6]))
            gu.assert_bits_equal(got[i], want, f"{name} palette of instance {i} (clip {clips[i]}, t={t[i]!r})")
            if not valid[i]:
                gu.assert_bits_equal(got[i], want_rest[name], f"{name} palette of the rest pose, instance {i}")
        d_pal.memset(0xFF)
        sk.solve_motion_set_device(ms, n, d_c.ptr, d_f.ptr, d_pal.ptr)
        got_f = d_pal.download((n, NB, 16), np.float32)
        want_f = np.stack(single[name])[np.minimum(clips, 3), np.arange(n)]
        want_f[~valid] = want_rest[name]
        gu.assert_bits_equal(got_f, want_f, f"{name} palettes, frame form vs solve_motion_device per clip")
        host = np.flatnonzero(valid & ~np.isnan(t))[::5]
        gu.assert_bits_equal(sk.solve_motion_set_time(ms, clips[host], t[host]), got[host], f"{name} palettes (host operands)")
    _close(ms, fk, ik, d_t, d_f, d_c, d_pal)


@pytest.mark.gpu
def test_gpu_set_of_one_clip_gives_the_bytes_of_the_plain_call():
    z = _mixed_crowd()
    n, t, frames = z["n"], z["t"], z["frames"]
    v = vmd.Vmd(z["data"][0])
    bm, mm = v.bind_bones(NAMES), v.bind_morphs(MNAMES)
    fk = vmd.Skeleton(*synth.make_skeleton(NB, 3, 5, 0.25, 3))
    ms = vmd.MotionSet([bm], [mm])
    d_t, d_f, d_c = DeviceBuffer.from_numpy(t), DeviceBuffer.from_numpy(frames), DeviceBuffer.from_numpy(np.zeros(n, np.uint32))
    d_a, d_b = DeviceBuffer(n * NB * 64), DeviceBuffer(n * NB * 64)
    runs = [("poses, times", (n, NB, 8), lambda o: bm.eval_time_device(n, d_t.ptr, o), lambda o: ms.eval_bones_time_device(n, d_c.ptr, d_t.ptr, o)),
            ("poses, frames", (n, NB, 8), lambda o: bm.eval_device(n, d_f.ptr, o), lambda o: ms.eval_bones_device(n, d_c.ptr, d_f.ptr, o)),
            ("rates, times", (n, 6), lambda o: mm.eval_time_device(n, d_t.ptr, o), lambda o: ms.eval_morphs_time_device(n, d_c.ptr, d_t.ptr, o)),
            ("rates, frames", (n, 6), lambda o: mm.eval_device(n, d_f.ptr, o), lambda o: ms.eval_morphs_device(n, d_c.ptr, d_f.ptr, o)),
            ("palettes, times", (n, NB, 16), lambda o: fk.solve_motion_time_device(bm, n, d_t.ptr, o),
             lambda o: fk.solve_motion_set_time_device(ms, n, d_c.ptr, d_t.ptr, o)),
            ("palettes, frames", (n, NB, 16), lambda o: fk.solve_motion_device(bm, n, d_f.ptr, o),
             lambda o: fk.solve_motion_set_device(ms, n, d_c.ptr, d_f.ptr, o))]
    for what, shape, plain, as_set in runs:
        d_a.memset(0xFF); d_b.memset(0xEE)
        plain(d_a.ptr)
        as_set(d_b.ptr)
        gu.assert_bits_equal(d_b.download(shape, np.float32), d_a.download(shape, np.float32), what)
    _close(ms, fk, bm, mm, v, d_t, d_f, d_c, d_a, d_b)


def _crowd_clips(m, seeds):
    """One clip per seed over the model's bones and morphs: different bone subsets, key counts and spans."""
    names = [f"b{i}" for i in range(m.nb)]
    mnames = [f"m{i}" for i in range(m.nm)]
    data = []
    for k, seed in enumerate(seeds):
        rng = np.random.RandomState(seed)
        mk = [(n, int(f), float(np.float32(rng.uniform(0, 1)))) for n in mnames[k % 2:] for f in (0, 31 + k, 80, 119)]
        data.append(vmd.write_vmd(synth.make_bone_keys(names[k:40 + 2 * k], seed, keys_per=4 + k, span=120), mk))
    return names, mnames, data


@pytest.mark.gpu
def test_gpu_mixed_crowd_end_to_end(oracle):
    """256 instances, a random clip each, sub-frame times: set -> palettes (one launch) and rates -> crowd deform, all in HBM;
    sampled instances (every clip among them) bit for bit against the oracle deform of the restated inputs."""
    m = synth.make_model(1500, 48, 6, 200, seed=51)
    names, mnames, data = _crowd_clips(m, (61, 62, 63, 64))
    ni = 256
    rng = np.random.RandomState(7)
    clips = rng.randint(0, 4, ni).astype(np.uint32)
    t = 0.25 + np.arange(ni) / 300.0 + (np.arange(ni) % 7) * (1.0 / 210.0)
    parent = np.asarray(m.bone_parent, np.int32)
    sk = vmd.Skeleton(m.bone_pos, parent)
    assert sk.info["solver"] == vmd.SOLVER_PARALLEL_FK
    vs = [vmd.Vmd(d) for d in data]
    bms, mms = [v.bind_bones(names) for v in vs], [v.bind_morphs(mnames) for v in vs]
    ms = vmd.MotionSet(bms, mms)
    _close(bms, mms)
    with DeformModel(m) as dm:
        d_t, d_c = DeviceBuffer.from_numpy(t), DeviceBuffer.from_numpy(clips)
        d_pal, d_w = DeviceBuffer(ni * m.nb * 64), DeviceBuffer(ni * m.nm * 4)
        sa, sb = dm.out_sizes(api.OUT_SOA, ni)
        d_a, d_b = DeviceBuffer(sa), DeviceBuffer(sb)
        sk.solve_motion_set_time_device(ms, ni, d_c.ptr, d_t.ptr, d_pal.ptr, dm)
        ms.eval_morphs_time_device(ni, d_c.ptr, d_t.ptr, d_w.ptr, dm)
        dm.deform_batched_raw(ni, d_w.ptr, d_pal.ptr, d_a.ptr, d_b.ptr, api.OUT_SOA,
                              api.PALETTE_ON_DEVICE | api.WEIGHTS_ON_DEVICE | api.OUT_ON_DEVICE)
        dm.sync()
        pos = d_a.download((ni, m.nv, 3), np.float32)
        nrm = d_b.download((ni, m.nv, 3), np.float32)
        sample = sorted({int(np.flatnonzero(clips == c)[k]) for c in range(4) for k in (0, -1)} | {0, 255})
        assert 8 <= len(sample) <= 10 and set(clips[sample]) == {0, 1, 2, 3}
        for i in sample:
            v = vs[clips[i]]
            pose = mt.restate_poses(v, names, t[i:i + 1])[0]
            rate = mt.restate_rates(v, mnames, t[i:i + 1])[0]
            pal = oracle.bone_solve(m.bone_pos, parent.astype(np.int64), pose)
            want_p, want_n = oracle.deform(m, rate, pal)
            gu.assert_bits_equal(pos[i], want_p, f"positions of instance {i} (clip {clips[i]})")
            gu.assert_bits_equal(nrm[i], want_n, f"normals of instance {i} (clip {clips[i]})")
        _close(d_t, d_c, d_pal, d_w, d_a, d_b)
    _close(ms, sk, vs)


@pytest.mark.gpu
def test_gpu_graph_of_the_set_calls(oracle):
    """The three calls of the end-to-end test recorded once (a linear chain); clip ids AND times rewritten in place; one replay
    equals the eager calls and the restatement.  Destroying the set while the graph lives invalidates the graph, as destroying a
    motion does."""
    m = synth.make_model(1500, 48, 6, 200, seed=53)
    names, mnames, data = _crowd_clips(m, (71, 72, 73, 74))
    ni = 16
    parent = np.asarray(m.bone_parent, np.int32)
    sk = vmd.Skeleton(m.bone_pos, parent)
    vs = [vmd.Vmd(d) for d in data]
    bms, mms = [v.bind_bones(names) for v in vs], [v.bind_morphs(mnames) for v in vs]
    ms = vmd.MotionSet(bms, mms)
    _close(bms, mms)
    flags = api.PALETTE_ON_DEVICE | api.WEIGHTS_ON_DEVICE | api.OUT_ON_DEVICE
    with DeformModel(m) as dm:
        d_t = DeviceBuffer.from_numpy(np.arange(ni) / 60.0)
        d_c = DeviceBuffer.from_numpy((np.arange(ni) % 4).astype(np.uint32))
        d_pal, d_w = DeviceBuffer(ni * m.nb * 64), DeviceBuffer(ni * m.nm * 4)
        sa, sb = dm.out_sizes(api.OUT_SOA, ni)
        d_a, d_b = DeviceBuffer(sa), DeviceBuffer(sb)

        def frame():
            sk.solve_motion_set_time_device(ms, ni, d_c.ptr, d_t.ptr, d_pal.ptr, dm)
            ms.eval_morphs_time_device(ni, d_c.ptr, d_t.ptr, d_w.ptr, dm)
            dm.deform_batched_raw(ni, d_w.ptr, d_pal.ptr, d_a.ptr, d_b.ptr, api.OUT_SOA, flags)
        frame()
        dm.sync()
        dm.graph_begin()
        frame()
        g = dm.graph_end()
        t = 2.0 + np.arange(ni) / 144.0 + 1.0 / 7.0
        clips = np.array([3, 3, 2, NONE, 1, 0, 0, 2, 1, 3, NONE, 0, 2, 2, 1, 9], np.uint32)
        d_t.upload(t)
        d_c.upload(clips)
        frame()
        dm.sync()
        want_a, want_b = d_a.download((ni, m.nv, 3), np.float32), d_b.download((ni, m.nv, 3), np.float32)
        want_pal, want_w = d_pal.download((ni, m.nb, 16), np.float32), d_w.download((ni, m.nm), np.float32)
        d_a.memset(0); d_b.memset(0); d_pal.memset(0); d_w.memset(0xFF)
        g.launch()
        dm.sync()
        gu.assert_bits_equal(d_a.download((ni, m.nv, 3), np.float32), want_a, "replay pos")
        gu.assert_bits_equal(d_b.download((ni, m.nv, 3), np.float32), want_b, "replay nrm")
        got_pal, got_w = d_pal.download((ni, m.nb, 16), np.float32), d_w.download((ni, m.nm), np.float32)
        gu.assert_bits_equal(got_pal, want_pal, "replay palettes")
        gu.assert_bits_equal(got_w, want_w, "replay rates")
        rest_pose = np.broadcast_to(REST_POSE, (m.nb, 8)).copy()
        for i in (0, 2, 3, 4, 5, 15):
            playing = clips[i] < 4
            pose = mt.restate_poses(vs[clips[i]], names, t[i:i + 1])[0] if playing else rest_pose
            rate = mt.restate_rates(vs[clips[i]], mnames, t[i:i + 1])[0] if playing else np.zeros(m.nm, np.float32)
            gu.assert_bits_equal(got_pal[i], oracle.bone_solve(m.bone_pos, parent.astype(np.int64), pose), f"palette {i}")
            gu.assert_bits_equal(got_w[i], rate, f"rates {i}")
        ms.close()                                        # the set took part in the recording
        with pytest.raises(api.MmdxError, match="destroyed"):
            g.launch()
        g.close()
        _close(d_t, d_c, d_pal, d_w, d_a, d_b)
    _close(sk, vs)


@pytest.mark.gpu
def test_cpp_motion_set_matches_python_path(tmp_path):
    """host/motion_example.cpp in crowd mode (mmdx::MotionSet: several .vmd files, instance i plays clip i % n_clips at its
    own time) against the same crowd driven from Python: identical palette and rate checksums."""
    from simple_mmd_renderer_amd import build, pmx
    nb = 40
    rig = synth.make_ik_rig(nb, 11, n_ik=3, n_append=4)
    m = synth.make_model(600, nb, 5, 60, seed=12)
    m.bone_pos, m.bone_parent = rig[0].copy(), rig[1].astype(m.bone_parent.dtype)
    bnames = ["骨%d" % b for b in range(nb)]
    mnames = ["表情%d" % k for k in range(m.nm)]
    (tmp_path / "m.pmx").write_bytes(pmx.write_pmx(m, pmx.PmxWriteOptions(rig=rig, bone_names=bnames, morph_names=mnames)))
    paths = []
    for k in range(3):
        rng = np.random.RandomState(5 + k)
        mk = [(n, int(f), float(np.float32(rng.uniform(0, 1)))) for n in mnames[:3 + k] for f in (0, 7 + k, 19)]
        p = tmp_path / ("c%d.vmd" % k)
        p.write_bytes(vmd.write_vmd(synth.make_bone_keys(bnames[k:30 + k], 13 + k, keys_per=4, span=24), mk))
        paths.append(str(p))
    ni, hz = 37, 144.0
    exe = build.build_host_example(name="motion_example")
    r = subprocess.run([exe, "--crowd", str(ni), str(hz), str(tmp_path / "m.pmx")] + paths, capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0 and "checksum=" in r.stdout, r.stdout + r.stderr
    pm = pmx.load_pmx(str(tmp_path / "m.pmx"))
    vs = [vmd.Vmd(p) for p in paths]
    bms, mms = [v.bind_bones(pm.bone_names) for v in vs], [v.bind_morphs(pm.morph_names) for v in vs]
    ms, sk = vmd.MotionSet(bms, mms), pm.skeleton()
    clips = (np.arange(ni) % 3).astype(np.uint32)
    t = np.arange(ni) / hz

    def fnv(a):
        h = 1469598103934665603
        for byte in np.ascontiguousarray(a).view(np.uint8).ravel().tolist():
            h = ((h ^ byte) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
        return h
    pal = sk.solve_motion_set_time(ms, clips, t)
    rates = ms.eval_morphs_time(clips, t)
    want = "crowd=%d clips=3 nb=%d nm=%d checksum=%016x" % (ni, nb, m.nm, (fnv(pal) * 31 + fnv(rates)) & 0xFFFFFFFFFFFFFFFF)
    assert r.stdout.strip() == want
    _close(ms, sk, bms, mms, vs)

"""Cross-fade between two clips of a motion set, per instance: mmdx_motion_set_blend_bones_time, _blend_morphs_time and
mmdx_skeleton_solve_motion_set_blend_time (include/mmdx.h, mmdx_motion_blend_args).

The blend is libmmd's own between-two-keys code applied between two clips -- l*(1-w) + r*w per channel
(L/motion/motion_impl.inl:364-372, :462) and NLerp(l, r)[w] (L/util/math_impl.inl:1260-1282) with NLerp's short circuits taken
for the whole row -- so everything here is compared as bit patterns, with no tolerance:
  * tests/golden/motion_blend_expect.npz comes from the real libmmd (tests/motion_blend_driver.cpp, tests/gen_motion_blend_golden.py);
  * tests/motion_blend_ref.py restates the blend in numpy float32 and reproduces that fixture on the CPU;
  * on the GPU the end-point rows are the rows of the existing set calls, the blended rows the restatement applied to them, and
    the one-launch palette call equals the blended poses followed by mmdx_skeleton_solve.
"""
import ctypes as C
import os

import numpy as np
import pytest

from simple_mmd_renderer_amd import _capi as api
from simple_mmd_renderer_amd import synth, vmd
from simple_mmd_renderer_amd.engine import DeformModel, DeviceBuffer
from tests import golden_util as gu
from tests import motion_blend_ref as mb
from tests import motion_time_ref as mt
from tests.test_capi_symbols import declared_symbols

BLEND_ENTRY_POINTS = ("mmdx_motion_set_blend_bones_time", "mmdx_motion_set_blend_morphs_time",
                      "mmdx_skeleton_solve_motion_set_blend_time")
NONE = vmd.CLIP_NONE
needs_driver = pytest.mark.skipif(not mt.driver_available(), reason="the reference's libmmd headers are not present")


@pytest.fixture(autouse=True)
def _lib(hip_lib):
    return hip_lib


def _close(*xs):
    for x in xs:
        for y in (x if isinstance(x, (list, tuple)) else [x]):
            y.free() if isinstance(y, DeviceBuffer) else y.close()


# ---------------------------------------------------------------------------------------- CPU ----
def test_blend_entry_points_are_declared_exported_and_bound(hip_lib):
    syms = declared_symbols()
    for name in BLEND_ENTRY_POINTS:
        assert name in syms and hasattr(hip_lib, name) and name in api.SIGNATURES, name
    hdr = open(os.path.join(os.path.dirname(mt.HERE), "include", "mmdx.h")).read()
    assert "typedef struct mmdx_motion_blend_args {" in hdr and "#define MMDX_ABI_VERSION 3u" in hdr
    assert hip_lib.mmdx_abi_version() == 3
    assert C.sizeof(vmd.MotionBlendArgs) == 2 * 4 + 5 * 8 + 4 + 4          # two u32, five pointers, flags, tail padding
    for name in ("blend_bones_time", "blend_morphs_time", "blend_bones_time_device", "blend_morphs_time_device"):
        assert callable(getattr(vmd.MotionSet, name))
    assert callable(vmd.Skeleton.solve_motion_set_blend_time) and callable(vmd.Skeleton.solve_motion_set_blend_time_device)
    poser = open(os.path.join(os.path.dirname(mt.HERE), "simple_mmd_renderer_amd", "host", "mmdx_poser.hpp")).read()
    assert "mmdx_skeleton_solve_motion_set_blend_time(" in poser


def _restated_sides(z):
    """The A and B rows of every fixture row from the restatement of the single clips (tests/motion_time_restate.c): poses
    [N, NB, 8] x 2, rates [N, NM] x 2."""
    bvs, mvs = [vmd.Vmd(p) for p in mb.BONE_VMDS], [vmd.Vmd(p) for p in mb.MORPH_VMDS]
    out = []
    for clips, times in ((z["clips_a"], z["times_a"]), (z["clips_b"], z["times_b"])):
        out.append(mb.pick([mt.restate_poses(v, z["bone_names"], times) for v in bvs], clips, mb.REST_POSE))
        out.append(mb.pick([mt.restate_rates(v, z["morph_names"], times) for v in mvs], clips, np.float32(0)))
    _close(bvs, mvs)
    return out[0], out[2], out[1], out[3]


def test_numpy_restatement_reproduces_the_libmmd_fixture(oracle):
    z = mb.fixture()
    n = z["weights"].size
    assert 180 <= n <= 220 and os.path.getsize(mb.FIXTURE) <= os.path.getsize(mt.FIXTURE)
    assert os.path.getsize(mb.CLIP_B_VMD) < 64 * 1024
    pose_a, pose_b, rate_a, rate_b = _restated_sides(z)
    gu.assert_bits_equal(mb.blend_poses(pose_a, pose_b, z["weights"]), z["expect_poses"], "poses")
    gu.assert_bits_equal(mb.blend_rates(rate_a, rate_b, z["weights"]), z["expect_rates"], "rates")
    zr = np.load(os.path.join(gu.GOLDEN_DIR, "rig_small_expect.npz"))
    for i in range(0, n, 5):
        pal = oracle.bone_solve(zr["rest"], zr["parent"], z["expect_poses"][i], zr["level"], zr["flags"])
        gu.assert_bits_equal(pal, z["expect_palettes"][i], f"palette of row {i}")
    # end-point rows are the single clip's rows, every bit
    side = mb.side_of(z["weights"])
    gu.assert_bits_equal(z["expect_poses"][side == 0], pose_a[side == 0], "A rows")
    gu.assert_bits_equal(z["expect_poses"][side == 1], pose_b[side == 1], "B rows")
    gu.assert_bits_equal(z["expect_rates"][side == 0], rate_a[side == 0], "A rates")
    gu.assert_bits_equal(z["expect_rates"][side == 1], rate_b[side == 1], "B rates")


def test_fixture_covers_both_hemispheres_and_every_weight_class():
    z = mb.fixture()
    pose_a, pose_b, _, _ = _restated_sides(z)
    mb.check_coverage(z, pose_a, pose_b)
    side = mb.side_of(z["weights"])
    assert [int((side == s).sum()) for s in (0, 1, 2)] == [60, 60, 80]     # 0, 5e-8, -1 | 1-5e-8, 1, 2 | 1e-7, .25, .5, 1-1e-7
    v = vmd.Vmd(mb.CLIP_B_VMD)
    assert min(len(v.bone_track(i)) for i in range(len(v.bone_track_names))) > 1          # more than one key per track
    assert min(len(v.morph_track(i)[0]) for i in range(len(v.morph_track_names))) > 1
    v.close()


@needs_driver
def test_fixture_equals_a_fresh_run_of_libmmd():
    z = mb.fixture()
    poses, rates = mb.driver_expect(mb.BONE_VMDS, z["bone_names"], mb.MORPH_VMDS, z["morph_names"], z["clips_a"], z["times_a"],
                                    z["clips_b"], z["times_b"], z["weights"])
    gu.assert_bits_equal(poses, z["expect_poses"], "poses")
    gu.assert_bits_equal(rates, z["expect_rates"], "rates")


def test_blend_entry_points_refuse_bad_arguments():
    """Everything that needs no device is decided before the first HIP call, so it is checked here without a GPU."""
    lib = api.lib()
    names = ["センター", "首"]
    v = vmd.Vmd(vmd.write_vmd(synth.make_bone_keys(names, 1, keys_per=3), [("あ", 0, 0.5), ("あ", 9, 1.0)]))
    bm, mm = v.bind_bones(names), v.bind_morphs(["あ"])
    both = vmd.MotionSet([bm, bm], [mm, mm])
    bones_only, morphs_only = vmd.MotionSet([bm, bm]), vmd.MotionSet(morph_motions=[mm, mm])
    sk = vmd.Skeleton(*synth.make_skeleton(2, 1))
    sk3 = vmd.Skeleton(*synth.make_skeleton(3, 1))
    good = dict(clips_a=np.array([0, NONE], np.uint32), clips_b=np.array([1, 0], np.uint32), times_a=np.array([0.5, 1.0]),
                times_b=np.array([0.0, 0.25]), weights=np.array([0.5, 0.0], np.float32))
    out = np.zeros((2, 2, 16), np.float32)
    err = lambda: lib.mmdx_last_error_string().decode()          # noqa: E731

    def args(n=2, flags=0, struct_size=None, **replace):
        arrays = dict(good, **replace)
        a = vmd.MotionBlendArgs(C.sizeof(vmd.MotionBlendArgs) if struct_size is None else struct_size, n,
                                *[arrays[k].ctypes.data if arrays[k] is not None else None
                                  for k in ("clips_a", "clips_b", "times_a", "times_b", "weights")], flags)
        a.keep = arrays
        return a
    calls = {   # name -> (call(set, args*, out), the set that lacks the side)
        "bones": (lambda s, a, o: lib.mmdx_motion_set_blend_bones_time(s, None, a, o), morphs_only),
        "morphs": (lambda s, a, o: lib.mmdx_motion_set_blend_morphs_time(s, None, a, o), bones_only),
        "solve": (lambda s, a, o: lib.mmdx_skeleton_solve_motion_set_blend_time(sk.h, s, None, a, o), morphs_only),
    }
    o = out.ctypes.data
    nan64, nan32 = np.array([0.5, np.nan]), np.array([0.5, np.nan], np.float32)
    for what, (call, lacking) in calls.items():
        assert call(None, C.byref(args()), o) == 1, what                                        # NULL set
        assert call(both.h, None, o) == 1, what                                                 # NULL args
        assert call(both.h, C.byref(args()), None) == 1, what                                   # NULL output
        for k in ("clips_a", "clips_b", "times_a", "times_b", "weights"):
            assert call(both.h, C.byref(args(**{k: None})), o) == 1 and "NULL" in err(), (what, k)
        assert call(both.h, C.byref(args(n=0)), o) == 1, what                                   # no instances
        for size in (0, C.sizeof(vmd.MotionBlendArgs) - 8, C.sizeof(vmd.MotionBlendArgs) + 8):
            assert call(both.h, C.byref(args(struct_size=size)), o) == 1 and "struct_size" in err(), (what, size)
        for bad in (1 << 1, 1 << 3, 1 << 4, 1 << 31):
            assert call(both.h, C.byref(args(flags=bad)), o) == 1 and "unknown flag" in err(), (what, bad)
        bad_b = np.array([1, 2], np.uint32)                                                     # 2 == n_clips, in clips_b only
        assert call(both.h, C.byref(args(clips_b=bad_b)), o) == 2 and "clips_b[1]" in err(), what          # MMDX_ERR_BAD_INDEX
        assert call(both.h, C.byref(args(clips_b=bad_b, flags=api.OUT_ON_DEVICE)), o) == 2, what
        assert call(both.h, C.byref(args(clips_a=bad_b)), o) == 2 and "clips_a[1]" in err(), what
        assert call(both.h, C.byref(args(times_a=nan64)), o) == 1 and "times_a[1] is NaN" in err(), what
        assert call(both.h, C.byref(args(times_b=nan64)), o) == 1 and "times_b[1] is NaN" in err(), what
        assert call(both.h, C.byref(args(weights=nan32)), o) == 1 and "weights[1] is NaN" in err(), what
        assert call(both.h, C.byref(args(weights=nan32, flags=api.OUT_ON_DEVICE)), o) == 1 and "NaN" in err(), what
        assert call(lacking.h, C.byref(args()), o) == 1 and "created without" in err(), what
    fn = lib.mmdx_skeleton_solve_motion_set_blend_time
    assert fn(None, both.h, None, C.byref(args()), o) == 1                                      # NULL skeleton
    assert fn(sk3.h, both.h, None, C.byref(args()), o) == 1 and "3" in err()                    # another bone count
    with pytest.raises(api.MmdxError) as e:
        both.blend_bones_time([0, 1], [0.0, 0.0], [1, 0], [0.0, 0.0], [0.5, float("nan")])
    assert e.value.status == 1
    with pytest.raises(api.MmdxError) as e:
        sk.solve_motion_set_blend_time(both, [0, 1], [0.0, 0.0], [1, 7], [0.0, 0.0], [0.5, 0.5])
    assert e.value.status == 2
    with pytest.raises(ValueError):
        both.blend_morphs_time([0, 1], [0.0, 0.0], [1], [0.0, 0.0], [0.5, 0.5])
    for x in (both, bones_only, morphs_only, sk, sk3, bm, mm, v):
        x.close()


# ---------------------------------------------------------------------------------------- GPU ----
def _device_operands(ca, ta, cb, tb, w):
    return [DeviceBuffer.from_numpy(np.ascontiguousarray(a, t)) for a, t in
            ((ca, np.uint32), (ta, np.float64), (cb, np.uint32), (tb, np.float64), (w, np.float32))]


def _ptrs(ds):
    return [d.ptr for d in ds]


@pytest.mark.gpu
def test_gpu_fixture_through_all_three_calls():
    """tests/golden/motion_blend_expect.npz (the real libmmd) with host operands and again with device operands."""
    z = mb.fixture()
    zr = np.load(os.path.join(gu.GOLDEN_DIR, "rig_small_expect.npz"))
    n, nb, nm = z["weights"].size, len(z["bone_names"]), len(z["morph_names"])
    bvs, mvs = [vmd.Vmd(p) for p in mb.BONE_VMDS], [vmd.Vmd(p) for p in mb.MORPH_VMDS]
    bms, mms = [v.bind_bones(z["bone_names"]) for v in bvs], [v.bind_morphs(z["morph_names"]) for v in mvs]
    ms = vmd.MotionSet(bms, mms)
    sk = vmd.Skeleton(zr["rest"], zr["parent"], zr["level"], zr["flags"])
    assert sk.info["solver"] == vmd.SOLVER_PARALLEL_FK
    ops = (z["clips_a"], z["times_a"], z["clips_b"], z["times_b"], z["weights"])
    gu.assert_bits_equal(ms.blend_bones_time(*ops), z["expect_poses"], "poses (host operands)")
    gu.assert_bits_equal(ms.blend_morphs_time(*ops), z["expect_rates"], "rates (host operands)")
    gu.assert_bits_equal(sk.solve_motion_set_blend_time(ms, *ops), z["expect_palettes"], "palettes (host operands)")
    ds = _device_operands(*ops)
    d_pose, d_w, d_pal = DeviceBuffer(n * nb * 32), DeviceBuffer(n * nm * 4), DeviceBuffer(n * nb * 64)
    for d in (d_pose, d_w, d_pal):
        d.memset(0xFF)
    ms.blend_bones_time_device(n, *_ptrs(ds), d_pose.ptr)
    ms.blend_morphs_time_device(n, *_ptrs(ds), d_w.ptr)
    sk.solve_motion_set_blend_time_device(ms, n, *_ptrs(ds), d_pal.ptr)
    gu.assert_bits_equal(d_pose.download((n, nb, 8), np.float32), z["expect_poses"], "poses (device operands)")
    gu.assert_bits_equal(d_w.download((n, nm), np.float32), z["expect_rates"], "rates (device operands)")
    gu.assert_bits_equal(d_pal.download((n, nb, 16), np.float32), z["expect_palettes"], "palettes (device operands)")
    _close(ms, sk, bms, mms, bvs, mvs, ds, d_pose, d_w, d_pal)


NI, NB, NM, NCLIPS = 67, 41, 7, 3                    # 41 bones / 7 morphs: a wave of the track kernels spans several instances
NAMES = [f"bone{i}" for i in range(NB)]
MNAMES = [f"m{i}" for i in range(NM)]
_cache = {}


def _crowd():
    """Three clips over 41 bones (different subsets) and 7 morphs, 67 instances, random clip ids and times on both sides, and the
    A and B rows of every instance from the EXISTING set calls on the device.  Computed once; nothing in it is modified."""
    if "crowd" in _cache:
        return _cache["crowd"]
    rng = np.random.RandomState(41)
    data = []
    for seed, sub in enumerate((NAMES[:35], NAMES[4:], NAMES[::2])):
        mk = [(n, int(f), float(np.float32(rng.uniform(-0.2, 1.2)))) for n in MNAMES[:5 + seed] for f in sorted(rng.choice(150, 5, replace=False))]
        data.append(vmd.write_vmd(synth.make_bone_keys(sub, 30 + seed, keys_per=4 + seed, span=150), mk))
    ca, cb = rng.randint(0, NCLIPS, NI).astype(np.uint32), rng.randint(0, NCLIPS, NI).astype(np.uint32)
    ca[5], cb[6], ca[7], cb[7] = NONE, NONE, NCLIPS + 5, NONE
    ta, tb = rng.uniform(-0.2, 5.5, NI), rng.uniform(-0.2, 5.5, NI)
    vs = [vmd.Vmd(d) for d in data]
    bms, mms = [v.bind_bones(NAMES) for v in vs], [v.bind_morphs(MNAMES) for v in vs]
    ms = vmd.MotionSet(bms, mms)
    _close(bms, mms, vs)
    d_pose, d_w = DeviceBuffer(NI * NB * 32), DeviceBuffer(NI * NM * 4)
    rows = {}
    for side, c, t in (("a", ca, ta), ("b", cb, tb)):
        d_c, d_t = DeviceBuffer.from_numpy(c), DeviceBuffer.from_numpy(t)
        ms.eval_bones_time_device(NI, d_c.ptr, d_t.ptr, d_pose.ptr)
        rows["pose_" + side] = d_pose.download((NI, NB, 8), np.float32)
        ms.eval_morphs_time_device(NI, d_c.ptr, d_t.ptr, d_w.ptr)
        rows["rate_" + side] = d_w.download((NI, NM), np.float32)
        _close(d_c, d_t)
    _close(ms, d_pose, d_w)
    _cache["crowd"] = dict(data=data, ca=ca, cb=cb, ta=ta, tb=tb, **rows)
    return _cache["crowd"]


def _crowd_set(z):
    vs = [vmd.Vmd(d) for d in z["data"]]
    bms, mms = [v.bind_bones(NAMES) for v in vs], [v.bind_morphs(MNAMES) for v in vs]
    ms = vmd.MotionSet(bms, mms)
    _close(bms, mms, vs)
    return ms


def _run_blend(ms, ca, ta, cb, tb, w):
    """Both track calls with device operands into pattern-filled outputs -> poses [NI, NB, 8], rates [NI, NM]."""
    ds = _device_operands(ca, ta, cb, tb, w)
    d_pose, d_w = DeviceBuffer(NI * NB * 32), DeviceBuffer(NI * NM * 4)
    d_pose.memset(0xFF); d_w.memset(0xFF)
    ms.blend_bones_time_device(NI, *_ptrs(ds), d_pose.ptr)
    ms.blend_morphs_time_device(NI, *_ptrs(ds), d_w.ptr)
    poses, rates = d_pose.download((NI, NB, 8), np.float32), d_w.download((NI, NM), np.float32)
    _close(ds, d_pose, d_w)
    return poses, rates


@pytest.mark.gpu
def test_gpu_end_point_rows_are_the_rows_of_the_set_calls():
    """w in {0, 5e-8, -1, NaN}: the row of (clips_a, times_a), with clips_b out of range and times_b NaN on those rows;
    w in {1, 1-5e-8, 2}: the row of (clips_b, times_b), with side a poisoned the same way.  This shows that nothing of the
    unused side reaches the row; that the kernels do not evaluate it at all is their code's property (the second
    eval_clip_pose / eval_clip_rate sits behind `side == kBlendMix`), which no output can show."""
    z = _crowd()
    ms = _crowd_set(z)
    ends = np.array([0.0, 5e-8, -1.0, np.nan, 1.0, 1 - 5e-8, 2.0], np.float32)
    w = ends[np.arange(NI) % ends.size]
    side = mb.side_of(w)
    assert set(side) == {0, 1} and (side == 0).sum() > 30 and (side == 1).sum() > 25
    ca, cb, ta, tb = z["ca"].copy(), z["cb"].copy(), z["ta"].copy(), z["tb"].copy()
    cb[side == 0], tb[side == 0] = NCLIPS + 5, np.nan
    ca[side == 1], ta[side == 1] = NCLIPS + 5, np.nan
    poses, rates = _run_blend(ms, ca, ta, cb, tb, w)
    is_a = (side == 0)
    gu.assert_bits_equal(poses[is_a], z["pose_a"][is_a], "A rows: poses")
    gu.assert_bits_equal(poses[~is_a], z["pose_b"][~is_a], "B rows: poses")
    gu.assert_bits_equal(rates[is_a], z["rate_a"][is_a], "A rows: rates")
    gu.assert_bits_equal(rates[~is_a], z["rate_b"][~is_a], "B rows: rates")
    _close(ms)


@pytest.mark.gpu
def test_gpu_mixed_crowd_equals_the_restatement_of_the_set_calls():
    """Weights of every class, different from lane to lane inside a wave (41 bones / 7 morphs per instance): every row equals
    motion_blend_ref applied to the rows of the two existing set calls, and every row of the pattern-filled output is written."""
    z = _crowd()
    ms = _crowd_set(z)
    rng = np.random.RandomState(43)
    # every weight the issue names twice (3 of them are A, 3 are B, 4 blend), a NaN, and the rest drawn from (0, 1)
    w = np.r_[mb.WEIGHTS, mb.WEIGHTS, np.float32(np.nan), rng.uniform(0, 1, NI - 2 * mb.WEIGHTS.size - 1).astype(np.float32)].astype(np.float32)
    w = w[rng.permutation(NI)]
    side = mb.side_of(w)
    assert all((side == s).sum() >= 4 for s in (0, 1, 2)) and (side == 2).sum() > 40
    poses, rates = _run_blend(ms, z["ca"], z["ta"], z["cb"], z["tb"], w)
    want_pose, want_rate = mb.blend_poses(z["pose_a"], z["pose_b"], w), mb.blend_rates(z["rate_a"], z["rate_b"], w)
    gu.assert_bits_equal(poses, want_pose, "poses")
    gu.assert_bits_equal(rates, want_rate, "rates")
    assert not (poses.view(np.uint32) == 0xFFFFFFFF).any() and not (rates.view(np.uint32) == 0xFFFFFFFF).any()
    dots = mb.quaternion_dots(z["pose_a"], z["pose_b"])[side == 2]
    assert (dots < 0).sum() > 100 and (dots >= 0).sum() > 100                     # both NLerp branches, many times
    # host operands give the device result (valid ids and MMDX_CLIP_NONE only, no NaN weight)
    host = np.flatnonzero(((z["ca"] < NCLIPS) | (z["ca"] == NONE)) & ((z["cb"] < NCLIPS) | (z["cb"] == NONE)) & ~np.isnan(w))
    ops = (z["ca"][host], z["ta"][host], z["cb"][host], z["tb"][host], w[host])
    gu.assert_bits_equal(ms.blend_bones_time(*ops), poses[host], "poses (host operands)")
    gu.assert_bits_equal(ms.blend_morphs_time(*ops), rates[host], "rates (host operands)")
    _close(ms)


def _solve_cases(name):
    if name == "ik":
        z = np.load(os.path.join(gu.GOLDEN_DIR, "rig_ik_expect.npz"))
        ik = {k[3:]: z[k] for k in z.files if k.startswith("ik_")}
        return vmd.Skeleton(z["rest"], z["parent"], z["level"], z["flags"], z["append_parent"], z["append_ratio"], ik), vmd.SOLVER_SERIAL
    nb = {"fk41": 41, "fk1030": 1030}[name]
    return vmd.Skeleton(*synth.make_skeleton(nb, 3, 5, 0.25, 3)), vmd.SOLVER_PARALLEL_FK


@pytest.mark.gpu
@pytest.mark.parametrize("rig", ["fk41", "fk1030", "ik"])
def test_gpu_one_launch_equals_blend_then_solve(rig):
    """mmdx_skeleton_solve_motion_set_blend_time against blend_bones_time followed by mmdx_skeleton_solve: a parallel-FK rig of
    41 bones, one of 1 030 (two bones per thread in the one-launch kernel) and the IK / append rig of rig_ik_expect.npz (the
    ordered solver: two launches)."""
    sk, solver = _solve_cases(rig)
    assert sk.info["solver"] == solver
    nb, ni = sk.nb, 5
    names = [f"b{i}" for i in range(nb)]
    vs = [vmd.Vmd(vmd.write_vmd(synth.make_bone_keys(names[k::1 + k], 80 + k, keys_per=3 + k, span=90), [])) for k in range(3)]
    bms = [v.bind_bones(names) for v in vs]
    ms = vmd.MotionSet(bms)
    _close(bms, vs)
    ca, cb = np.array([0, 1, 2, NONE, 1], np.uint32), np.array([1, 2, 0, 2, 9], np.uint32)
    ta, tb = np.array([0.1, 0.7, 1.3, 2.0, 2.9]), np.array([2.5, 0.2, 1.0, 0.5, 1.1])
    w = np.array([0.0, 0.3, 1.0, 0.5, 1e-7], np.float32)
    ds = _device_operands(ca, ta, cb, tb, w)
    d_pose, d_two, d_one = DeviceBuffer(ni * nb * 32), DeviceBuffer(ni * nb * 64), DeviceBuffer(ni * nb * 64)
    d_two.memset(0xEE); d_one.memset(0xFF)
    ms.blend_bones_time_device(ni, *_ptrs(ds), d_pose.ptr)
    sk.solve_device(ni, d_pose.ptr, d_two.ptr)
    sk.solve_motion_set_blend_time_device(ms, ni, *_ptrs(ds), d_one.ptr)
    two = d_two.download((ni, nb, 16), np.float32)
    gu.assert_bits_equal(d_one.download((ni, nb, 16), np.float32), two, f"{rig}: one call vs blend + solve")
    gu.assert_bits_equal(sk.solve_motion_set_blend_time(ms, ca[:4], ta[:4], cb[:4], tb[:4], w[:4]), two[:4], f"{rig}: host operands")
    assert len({two[i].tobytes() for i in range(ni)}) == ni                       # five different poses went through
    _close(ms, sk, ds, d_pose, d_two, d_one)


@pytest.mark.gpu
def test_gpu_graph_of_blend_solve_and_deform():
    """blend-solve -> blend-morphs -> mmdx_deform_batched recorded once with every operand on the device (after one eager run);
    replayed; weights and clips_b rewritten in place; replayed again.  Each replay's vertices equal the direct calls'."""
    from tests.test_motion_set import _crowd_clips
    m = synth.make_model(2048, 64, 8, 200, 112)                                   # the size of g12_mini_model
    names, mnames, data = _crowd_clips(m, (91, 92, 93, 94))
    ni = 4
    sk = vmd.Skeleton(m.bone_pos, np.asarray(m.bone_parent, np.int32))
    vs = [vmd.Vmd(d) for d in data]
    bms, mms = [v.bind_bones(names) for v in vs], [v.bind_morphs(mnames) for v in vs]
    ms = vmd.MotionSet(bms, mms)
    _close(bms, mms, vs)
    flags = api.PALETTE_ON_DEVICE | api.WEIGHTS_ON_DEVICE | api.OUT_ON_DEVICE
    with DeformModel(m) as dm:
        ds = _device_operands(np.array([0, 1, 2, 3], np.uint32), np.array([0.5, 1.25, 2.0, 3.1]),
                              np.array([1, 1, 0, NONE], np.uint32), np.array([1.5, 0.3, 2.2, 0.0]), np.array([0.0, 0.5, 0.25, 1.0], np.float32))
        d_cb, d_wt = ds[2], ds[4]
        d_pal, d_w = DeviceBuffer(ni * m.nb * 64), DeviceBuffer(ni * m.nm * 4)
        sa, sb = dm.out_sizes(api.OUT_SOA, ni)
        d_a, d_b = DeviceBuffer(sa), DeviceBuffer(sb)

        def frame():
            sk.solve_motion_set_blend_time_device(ms, ni, *_ptrs(ds), d_pal.ptr, dm)
            ms.blend_morphs_time_device(ni, *_ptrs(ds), d_w.ptr, dm)
            dm.deform_batched_raw(ni, d_w.ptr, d_pal.ptr, d_a.ptr, d_b.ptr, api.OUT_SOA, flags)

        def direct():
            frame()
            dm.sync()
            return d_a.download((ni, m.nv, 3), np.float32), d_b.download((ni, m.nv, 3), np.float32)

        def replay(g):
            d_a.memset(0); d_b.memset(0); d_pal.memset(0); d_w.memset(0xFF)
            g.launch()
            dm.sync()
            return d_a.download((ni, m.nv, 3), np.float32), d_b.download((ni, m.nv, 3), np.float32)
        first = direct()                                      # the run before recording, as the header requires
        dm.graph_begin()
        frame()
        g = dm.graph_end()
        got = replay(g)
        gu.assert_bits_equal(got[0], first[0], "replay 1 pos")
        gu.assert_bits_equal(got[1], first[1], "replay 1 nrm")
        d_wt.upload(np.array([0.75, 1.0, 5e-8, 0.5], np.float32))
        d_cb.upload(np.array([3, 2, 9, 0], np.uint32))
        got = replay(g)
        second = direct()
        gu.assert_bits_equal(got[0], second[0], "replay 2 pos")
        gu.assert_bits_equal(got[1], second[1], "replay 2 nrm")
        assert not np.array_equal(first[0].view(np.uint32), second[0].view(np.uint32))
        g.close()
        _close(ds, d_pal, d_w, d_a, d_b)
    _close(ms, sk)

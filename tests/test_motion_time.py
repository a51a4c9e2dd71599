"""Time-based motion evaluation: mmdx_morph_motion_eval_time, mmdx_bone_motion_eval_time, mmdx_skeleton_solve_motion_time
(MotionPlayer::SeekTime, L/motion/poser_impl.inl:548-555; Motion::GetBonePose / GetMorphPose(name, double time),
L/motion/motion_impl.inl:321-380, :426-465).

CPU tests pin the fixture tests/golden/motion_time_expect.npz and the restatement tests/motion_time_restate.c against the
real libmmd (tests/motion_time_driver.cpp, where the reference's headers are present), show that the fixture exercises the
places where the time path differs from the frame path, and check the new entry points' symbols and argument checks.  GPU
tests compare the HIP kernels with the fixture and the restatement through the C ABI: bit-exact, no tolerance.
"""
import os
import subprocess

import numpy as np
import pytest

from oracle.pyoracle import Reference, ReferenceMotion, reference_available
from simple_mmd_renderer_amd import _capi as api
from simple_mmd_renderer_amd import synth, vmd
from simple_mmd_renderer_amd.engine import DeformModel, DeviceBuffer
from tests import golden_util as gu
from tests import motion_time_ref as mt
from tests.test_capi_symbols import declared_symbols

TIME_ENTRY_POINTS = ("mmdx_morph_motion_eval_time", "mmdx_bone_motion_eval_time", "mmdx_skeleton_solve_motion_time")
needs_driver = pytest.mark.skipif(not mt.driver_available(), reason="the reference's libmmd headers are not present")


@pytest.fixture(autouse=True)
def _lib(hip_lib):
    return hip_lib


def random_motion(seed, names, morph_names=()):
    """Random bone tracks (curved and linear keys, one key beyond 2^24) and morph tracks (one infinite weight next to a key)."""
    keys = synth.make_bone_keys(names, seed, keys_per=4 + seed, span=150)
    keys.append((names[0], 2 ** 24 + 9, (0, 1, 0), (0, 0.6, 0, 0.8), bytes([64] * 64)))    # beyond float's exact range
    rng = np.random.RandomState(seed)
    mk = []
    for n in morph_names:
        for f in sorted(rng.choice(150, 5, replace=False)):
            mk.append((n, int(f), float(np.float32(rng.uniform(-0.2, 1.2)))))
    if morph_names:
        mk.append((morph_names[0], 2 ** 24 + 3, 0.25))
        mk.append((morph_names[-1], 400, float("inf")))         # at its neighbour's exact key, the time path gives NaN
    return vmd.write_vmd(keys, mk)


def key_frames_of(v):
    """Every key frame of every bone and morph track of a parsed motion, ascending."""
    ks = {int(f) for fr, _, _, _ in mt.tracks_of(v).values() for f in fr}
    for i in range(len(v.morph_track_names)):
        ks.update(int(f) for f in v.morph_track(i)[0])
    return sorted(ks)


def random_times(seed, keys=(), n=200):
    rng = np.random.RandomState(seed)
    t = [-1.0, -0.0, 0.0, -np.inf, np.inf, 1e300, 2.0 ** 32 / 30.0, 2.0 ** 33 / 30.0, (2 ** 24 + 9) / 30.0,
         np.nextafter((2 ** 24 + 9) / 30.0, -np.inf), (2 ** 24 + 3) / 30.0, 399 / 30.0, 400 / 30.0, 1.5]
    t += list(rng.uniform(-0.5, 5.6, n))
    for k in keys:
        x = k / 30.0
        t += [x, np.nextafter(x, -np.inf), np.nextafter(x, np.inf)]
    return np.array(t, np.float64)


# ---------------------------------------------------------------------------------------- CPU ----
@needs_driver
def test_fixture_equals_a_fresh_run_of_libmmd():
    z = mt.fixture()
    poses, rates = mt.driver_expect(mt.BONE_VMD, z["bone_names"], mt.MORPH_VMD, z["morph_names"], z["times"])
    gu.assert_bits_equal(poses, z["expect_poses"], "poses")
    gu.assert_bits_equal(rates, z["expect_rates"], "rates")
    if reference_available():
        rsk = Reference.skeleton(z["rest"], z["parent"], z["level"], z["flags"])
        for i in range(0, z["times"].size, 7):
            gu.assert_bits_equal(rsk.solve(poses[i]), z["expect_palettes"][i], f"palette at t={z['times'][i]!r}")
        rsk.close()


def test_restatement_equals_the_fixture(oracle):
    z = mt.fixture()
    assert 300 < z["times"].size and os.path.getsize(mt.FIXTURE) < 420 * 1024
    gu.assert_bits_equal(mt.restate_poses(vmd.Vmd(mt.BONE_VMD), z["bone_names"], z["times"]), z["expect_poses"], "poses")
    gu.assert_bits_equal(mt.restate_rates(vmd.Vmd(mt.MORPH_VMD), z["morph_names"], z["times"]), z["expect_rates"], "rates")
    for i in range(0, z["times"].size, 5):
        pal = oracle.bone_solve(z["rest"], z["parent"], z["expect_poses"][i], z["level"], z["flags"])
        gu.assert_bits_equal(pal, z["expect_palettes"][i], f"palette at t={z['times'][i]!r}")


@needs_driver
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_restatement_equals_libmmd_on_random_motions(tmp_path, seed):
    names = ["センター", "上半身", "首", "頭", "左腕", "右腕", "BoneEN"]
    mnames = ["あ", "まばたき", "MorphEN"]
    p = tmp_path / "t.vmd"
    p.write_bytes(random_motion(seed, names, mnames))
    v = vmd.Vmd(str(p))
    keys = key_frames_of(v)
    t = random_times(seed, keys)
    assert (t * 30.0 > 2.0 ** 32).any() and max(keys) > 2 ** 24
    want_p, want_r = mt.driver_expect(str(p), names + ["無い"], str(p), mnames + ["無い"], t)
    gu.assert_bits_equal(mt.restate_poses(v, names + ["無い"], t), want_p, "poses")
    gu.assert_bits_equal(mt.restate_rates(v, mnames + ["無い"], t), want_r, "rates")
    assert np.isnan(want_r).any()                                # the infinite weight's neighbour at its exact key


def test_fixture_exercises_what_the_frame_path_does_not(oracle):
    """Point 4: at time * 30 == a key's frame the time path interpolates at bary 0 where the frame path returns the key:
    the fixture holds such (time, track) pairs whose result differs from Motion::GetBonePose(name, k).  Point 5: it holds
    times just below a key (the left key's curve at bary rounded up to 1.0f)."""
    z = mt.fixture()
    v = vmd.Vmd(mt.BONE_VMD)
    tracks = mt.tracks_of(v)
    rm = ReferenceMotion(mt.BONE_VMD) if reference_available() else None
    differs = []
    for j, n in enumerate(z["bone_names"]):
        if n not in tracks:
            continue
        fr = tracks[n][0]
        for i, t in enumerate(z["times"]):
            d = t * 30.0
            if np.isfinite(d) and d == np.floor(d) and fr[0] < d < fr[-1] and int(d) in set(fr.tolist()):
                k = int(d)
                frame_pose = oracle.bone_pose(*tracks[n], k)
                if rm is not None:
                    gu.assert_bits_equal(rm.bone_pose(n.encode("shift_jis"), k), frame_pose, "frame path")
                if not np.array_equal(gu.bits(frame_pose), gu.bits(z["expect_poses"][i, j])):
                    differs.append((float(t), n, k))
    if rm is not None:
        rm.close()
    assert len(differs) >= 1, "no exact-key time whose result differs from the frame path"
    keys = sorted({int(f) for fr, _, _, _ in tracks.values() for f in fr})
    below = [t for t in z["times"] if np.isfinite(t) and any(0 < k - t * 30.0 < 1e-9 for k in keys)]
    assert len(below) >= 10


def test_time_entry_points_are_declared_and_exported(hip_lib):
    syms = declared_symbols()
    for name in TIME_ENTRY_POINTS:
        assert name in syms and hasattr(hip_lib, name) and name in api.SIGNATURES
    hdr = open(os.path.join(os.path.dirname(mt.HERE), "include", "mmdx.h")).read()
    assert "MMDX_TIMES_ON_DEVICE = MMDX_FRAMES_ON_DEVICE" in hdr and "#define MMDX_ABI_VERSION 3u" in hdr


def test_time_entry_points_refuse_bad_arguments():
    """NULL operands, n_instances == 0, unknown flag bits and NaN host times: MMDX_ERR_INVALID_ARGUMENT before any device work."""
    lib = api.lib()
    names = ["センター", "首"]
    v = vmd.Vmd(vmd.write_vmd(synth.make_bone_keys(names, 1, keys_per=3), [("あ", 0, 0.5), ("あ", 9, 1.0)]))
    bm, mm = v.bind_bones(names), v.bind_morphs(["あ"])
    rest, parent, level, flags = synth.make_skeleton(2, 1)
    sk = vmd.Skeleton(rest, parent, level, flags)
    t = np.array([0.5, 1.0], np.float64)
    tn = np.array([0.5, np.nan], np.float64)
    out = np.zeros((2, 2, 16), np.float32)
    calls = {
        "morph": lambda tp, f, o=out.ctypes.data, n=2, h=mm.h: lib.mmdx_morph_motion_eval_time(h, None, n, tp, f, o),
        "bone": lambda tp, f, o=out.ctypes.data, n=2, h=bm.h: lib.mmdx_bone_motion_eval_time(h, None, n, tp, f, o),
        "skeleton": lambda tp, f, o=out.ctypes.data, n=2, h=bm.h: lib.mmdx_skeleton_solve_motion_time(sk.h, h, None, n, tp, f, o),
    }
    for what, call in calls.items():
        assert call(None, 0) == 1, what                                            # NULL times
        assert call(t.ctypes.data, 0, o=None) == 1, what                           # NULL output
        assert call(t.ctypes.data, 0, h=None) == 1, what                           # NULL motion
        assert call(t.ctypes.data, 0, n=0) == 1, what                              # no instances
        for bad in (1 << 1, 1 << 3, 1 << 4, 1 << 31):
            assert call(t.ctypes.data, bad) == 1 and "unknown flag" in lib.mmdx_last_error_string().decode(), (what, bad)
        assert call(tn.ctypes.data, 0) == 1 and "NaN" in lib.mmdx_last_error_string().decode(), what
        assert call(tn.ctypes.data, api.OUT_ON_DEVICE) == 1, what                 # host times with device output
    assert lib.mmdx_skeleton_solve_motion_time(None, bm.h, None, 2, t.ctypes.data, 0, out.ctypes.data) == 1
    with pytest.raises(api.MmdxError) as e:
        bm.eval_time([0.0, float("nan")])
    assert e.value.status == 1
    sk.close()


# ---------------------------------------------------------------------------------------- GPU ----
@pytest.mark.gpu
def test_gpu_golden_time_paths():
    """The fixture through all three entry points, with host and with device times."""
    z = mt.fixture()
    t = z["times"]
    n = t.size
    mm = vmd.Vmd(mt.MORPH_VMD).bind_morphs(z["morph_names"])
    bm = vmd.Vmd(mt.BONE_VMD).bind_bones(z["bone_names"])
    sk = vmd.Skeleton(z["rest"], z["parent"], z["level"], z["flags"])
    assert sk.info["solver"] == vmd.SOLVER_PARALLEL_FK
    gu.assert_bits_equal(mm.eval_time(t), z["expect_rates"], "rates (host times)")
    gu.assert_bits_equal(bm.eval_time(t), z["expect_poses"], "poses (host times)")
    gu.assert_bits_equal(sk.solve_motion_time(bm, t), z["expect_palettes"], "palettes (host times)")
    nb, nm = len(z["bone_names"]), len(z["morph_names"])
    d_t = DeviceBuffer.from_numpy(t)
    d_w, d_pose, d_pal = DeviceBuffer(n * nm * 4), DeviceBuffer(n * nb * 32), DeviceBuffer(n * nb * 64)
    for d in (d_w, d_pose, d_pal):
        d.memset(0xFF)
    mm.eval_time_device(n, d_t.ptr, d_w.ptr)
    bm.eval_time_device(n, d_t.ptr, d_pose.ptr)
    sk.solve_motion_time_device(bm, n, d_t.ptr, d_pal.ptr)
    gu.assert_bits_equal(d_w.download((n, nm), np.float32), z["expect_rates"], "rates (device times)")
    gu.assert_bits_equal(d_pose.download((n, nb, 8), np.float32), z["expect_poses"], "poses (device times)")
    gu.assert_bits_equal(d_pal.download((n, nb, 16), np.float32), z["expect_palettes"], "palettes (device times)")
    for d in (d_t, d_w, d_pose, d_pal):
        d.free()
    sk.close()


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_gpu_random_time_motions_vs_restatement(oracle, seed):
    """Random motions at random and corner times (device NaN included: the first key), through the one-launch FK path and
    through an IK / append rig (the two-launch path); palettes against the oracle solve of the restated poses."""
    nb = 40
    names = [f"bone{i}" for i in range(nb)]
    mnames = [f"m{i}" for i in range(5)]
    v = vmd.Vmd(random_motion(seed, names[:33], mnames))
    keys = key_frames_of(v)
    t = np.r_[random_times(100 + seed, keys[:60], n=150), np.nan]
    n = t.size
    poses = mt.restate_poses(v, names, t)
    rates = mt.restate_rates(v, mnames + ["none"], t)
    bm, mm = v.bind_bones(names), v.bind_morphs(mnames + ["none"])
    d_t = DeviceBuffer.from_numpy(t)
    d_pose, d_w = DeviceBuffer(n * nb * 32), DeviceBuffer(n * 6 * 4)
    bm.eval_time_device(n, d_t.ptr, d_pose.ptr)
    mm.eval_time_device(n, d_t.ptr, d_w.ptr)
    gu.assert_bits_equal(d_pose.download((n, nb, 8), np.float32), poses, "poses")
    gu.assert_bits_equal(d_w.download((n, 6), np.float32), rates, "rates")
    gu.assert_bits_equal(bm.eval_time(t[:-1]), poses[:-1], "poses (host times)")
    gu.assert_bits_equal(poses[-1], poses[3], "NaN takes the first key, as -inf")
    rest, parent, level, flags = synth.make_skeleton(nb, seed, 5, 0.25, 3)
    fk = vmd.Skeleton(rest, parent, level, flags)
    rig = synth.make_ik_rig(nb, seed, n_ik=3, n_append=4)
    ik = vmd.Skeleton(*rig)
    assert fk.info["solver"] == vmd.SOLVER_PARALLEL_FK and ik.info["solver"] == vmd.SOLVER_SERIAL
    d_pal = DeviceBuffer(n * nb * 64)
    fk.solve_motion_time_device(bm, n, d_t.ptr, d_pal.ptr)
    got_fk = d_pal.download((n, nb, 16), np.float32)
    ik.solve_motion_time_device(bm, n, d_t.ptr, d_pal.ptr)
    got_ik = d_pal.download((n, nb, 16), np.float32)
    host_ik = ik.solve_motion_time(bm, t[:-1])
    for i in range(0, n, 3):
        gu.assert_bits_equal(got_fk[i], oracle.bone_solve(rest, parent, poses[i], level, flags), f"FK palette at t={t[i]!r}")
        want = oracle.bone_solve_full(rig[0], rig[1], poses[i], rig[2], rig[3], rig[4], rig[5], rig[6])
        gu.assert_bits_equal(got_ik[i], want, f"IK palette at t={t[i]!r}")
        if i < n - 1:
            gu.assert_bits_equal(host_ik[i], want, f"IK palette (host times) at t={t[i]!r}")
    for d in (d_t, d_pose, d_w, d_pal):
        d.free()
    fk.close(); ik.close()


def _crowd_scene(seed):
    m = synth.make_model(1500, 48, 6, 200, seed=seed)
    names = [f"b{i}" for i in range(m.nb)]
    mnames = [f"m{i}" for i in range(m.nm)]
    rng = np.random.RandomState(seed)
    data = vmd.write_vmd(synth.make_bone_keys(names[:40], seed, keys_per=6, span=120),
                         [(n, int(f), float(np.float32(rng.uniform(0, 1)))) for n in mnames for f in (0, 37, 80, 119)])
    return m, names, mnames, vmd.Vmd(data)


@pytest.mark.gpu
def test_gpu_crowd_of_1024_at_device_times_end_to_end(oracle):
    """1 024 instances at sub-frame phase offsets: times -> palettes (one launch) and times -> rates, then the crowd deform,
    all in HBM; sampled instances bit for bit against the oracle deform of the restated poses and rates."""
    m, names, mnames, v = _crowd_scene(41)
    ni = 1024
    t = 0.25 + np.arange(ni) / 300.0 + (np.arange(ni) % 7) * (1.0 / 210.0)
    parent = np.asarray(m.bone_parent, np.int32)
    sk = vmd.Skeleton(m.bone_pos, parent)
    bm, mm = v.bind_bones(names), v.bind_morphs(mnames)
    with DeformModel(m) as dm:
        d_t = DeviceBuffer.from_numpy(t)
        d_pal, d_w = DeviceBuffer(ni * m.nb * 64), DeviceBuffer(ni * m.nm * 4)
        sa, sb = dm.out_sizes(api.OUT_SOA, ni)
        d_a, d_b = DeviceBuffer(sa), DeviceBuffer(sb)
        sk.solve_motion_time_device(bm, ni, d_t.ptr, d_pal.ptr, dm)
        mm.eval_time_device(ni, d_t.ptr, d_w.ptr, dm)
        dm.deform_batched_raw(ni, d_w.ptr, d_pal.ptr, d_a.ptr, d_b.ptr, api.OUT_SOA,
                              api.PALETTE_ON_DEVICE | api.WEIGHTS_ON_DEVICE | api.OUT_ON_DEVICE)
        dm.sync()
        pos = d_a.download((ni, m.nv, 3), np.float32)
        nrm = d_b.download((ni, m.nv, 3), np.float32)
        sample = [0, 1, 2, 3, 255, 511, 512, 777, 1000, 1023]
        poses = mt.restate_poses(v, names, t[sample])
        rates = mt.restate_rates(v, mnames, t[sample])
        for s, i in enumerate(sample):
            pal = oracle.bone_solve(m.bone_pos, parent.astype(np.int64), poses[s])
            want_p, want_n = oracle.deform(m, rates[s], pal)
            gu.assert_bits_equal(pos[i], want_p, f"positions of instance {i}")
            gu.assert_bits_equal(nrm[i], want_n, f"normals of instance {i}")
        for d in (d_t, d_pal, d_w, d_a, d_b):
            d.free()
    sk.close()


@pytest.mark.gpu
def test_gpu_graph_of_the_device_time_calls(oracle):
    """solve_motion_time + morph eval_time + the crowd deform recorded once; the times rewritten in place; one replay equals
    the eager calls and the restatement."""
    m, names, mnames, v = _crowd_scene(43)
    ni = 16
    parent = np.asarray(m.bone_parent, np.int32)
    sk = vmd.Skeleton(m.bone_pos, parent)
    bm, mm = v.bind_bones(names), v.bind_morphs(mnames)
    flags = api.PALETTE_ON_DEVICE | api.WEIGHTS_ON_DEVICE | api.OUT_ON_DEVICE
    with DeformModel(m) as dm:
        d_t = DeviceBuffer.from_numpy(np.arange(ni) / 60.0)
        d_pal, d_w = DeviceBuffer(ni * m.nb * 64), DeviceBuffer(ni * m.nm * 4)
        sa, sb = dm.out_sizes(api.OUT_SOA, ni)
        d_a, d_b = DeviceBuffer(sa), DeviceBuffer(sb)

        def frame():
            sk.solve_motion_time_device(bm, ni, d_t.ptr, d_pal.ptr, dm)
            mm.eval_time_device(ni, d_t.ptr, d_w.ptr, dm)
            dm.deform_batched_raw(ni, d_w.ptr, d_pal.ptr, d_a.ptr, d_b.ptr, api.OUT_SOA, flags)
        frame()
        dm.sync()
        dm.graph_begin()
        frame()
        g = dm.graph_end()
        t = 2.0 + np.arange(ni) / 144.0 + 1.0 / 7.0
        d_t.upload(t)
        frame()
        dm.sync()
        want_a, want_b = d_a.download((ni, m.nv, 3), np.float32), d_b.download((ni, m.nv, 3), np.float32)
        want_pal = d_pal.download((ni, m.nb, 16), np.float32)
        d_a.memset(0); d_b.memset(0); d_pal.memset(0)
        g.launch()
        dm.sync()
        gu.assert_bits_equal(d_a.download((ni, m.nv, 3), np.float32), want_a, "replay pos")
        gu.assert_bits_equal(d_b.download((ni, m.nv, 3), np.float32), want_b, "replay nrm")
        got_pal = d_pal.download((ni, m.nb, 16), np.float32)
        gu.assert_bits_equal(got_pal, want_pal, "replay palettes")
        poses = mt.restate_poses(v, names, t[:3])
        for i in range(3):
            gu.assert_bits_equal(got_pal[i], oracle.bone_solve(m.bone_pos, parent.astype(np.int64), poses[i]), f"palette {i}")
        g.close()
        for d in (d_t, d_pal, d_w, d_a, d_b):
            d.free()
    sk.close()


@pytest.mark.gpu
def test_cpp_motion_player_seek_time_matches_python_path(tmp_path):
    """host/motion_example.cpp with a display rate (mmdx::MotionPlayer::SeekTime at n / hz) against the same steps driven
    from Python through the *_time entry points: identical checksums."""
    from simple_mmd_renderer_amd import build, pmx
    nb = 40
    rig = synth.make_ik_rig(nb, 11, n_ik=3, n_append=4)
    m = synth.make_model(600, nb, 5, 60, seed=12)
    m.bone_pos, m.bone_parent = rig[0].copy(), rig[1].astype(m.bone_parent.dtype)
    bnames = ["骨%d" % b for b in range(nb)]
    mnames = ["表情%d" % k for k in range(m.nm)]
    (tmp_path / "m.pmx").write_bytes(pmx.write_pmx(m, pmx.PmxWriteOptions(rig=rig, bone_names=bnames, morph_names=mnames)))
    rng = np.random.RandomState(5)
    mk = [(n, int(f), float(np.float32(rng.uniform(0, 1)))) for n in mnames[:4] for f in (0, 7, 19)]
    (tmp_path / "m.vmd").write_bytes(vmd.write_vmd(synth.make_bone_keys(bnames[:30], 13, keys_per=4, span=24), mk))
    steps, hz = 50, 144.0
    exe = build.build_host_example(name="motion_example")
    r = subprocess.run([exe, str(tmp_path / "m.pmx"), str(tmp_path / "m.vmd"), str(steps), "144"], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0 and "checksum=" in r.stdout, r.stdout + r.stderr
    pm = pmx.load_pmx(str(tmp_path / "m.pmx"))
    v = vmd.Vmd(str(tmp_path / "m.vmd"))
    bm, mm, sk = v.bind_bones(pm.bone_names), v.bind_morphs(pm.morph_names), pm.skeleton()

    def fnv(a):
        h = 1469598103934665603
        for byte in np.ascontiguousarray(a).view(np.uint8).ravel().tolist():
            h = ((h ^ byte) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
        return h
    h = 0
    with DeformModel(pm.flat) as dm:
        for f in range(steps):
            t = f / hz
            rates = mm.eval_time([t], dm)[0]
            pal = sk.solve(bm.eval_time([t], dm), dm, morph_weights=rates)[0]
            _pos, nrm = dm.deform(rates, pal)
            v32 = dm.deform_vertex32(rates, pal, 0.1)
            h = (h * 31 + fnv(v32) + fnv(nrm)) & 0xFFFFFFFFFFFFFFFF
    want = "frames=%d nv=%d nb=%d mapped_bones=30 checksum=%016x" % (steps, pm.flat.nv, nb, h)
    assert r.stdout.strip() == want
    # and a sub-frame step really moves the pose where whole frames would repeat it (60 Hz shows each VMD frame twice)
    assert not np.array_equal(gu.bits(bm.eval_time([1.0 / 60.0])), gu.bits(bm.eval_time([0.0])))

"""Root motion without a GPU: mmdx_animator_root_motion and mmdx_bone_motion_in_place (include/mmdx.h).

The contract is the arithmetic the header states.  Here it is held by the golden rows of the real libmmd
(tests/golden/root_motion_expect.npz, tests/root_motion_driver.cpp) against two statements that must agree with them bit for bit:
csrc/root_math.hpp compiled for the host (tests/root_math_driver.cpp, a stand-alone program, plain and sanitized) and the numpy
restatement tests/root_motion_ref.py.  tests/test_root_motion.py runs the same rows through the gfx950 kernel.
"""
import ctypes as C
import os

import numpy as np
import pytest

from simple_mmd_renderer_amd import _capi as api
from simple_mmd_renderer_amd import vmd
from tests import golden_util as gu
from tests import motion_time_ref as mt
from tests import root_motion_ref as rm
from tests.test_capi_symbols import declared_symbols

ROOT = os.path.dirname(mt.HERE)
needs_driver = pytest.mark.skipif(not mt.driver_available(), reason="the reference's libmmd headers are not present")
ALL_AXES = api.ROOT_X | api.ROOT_Y | api.ROOT_Z


@pytest.fixture(autouse=True)
def _lib(hip_lib):
    return hip_lib


def close_all(*xs):
    for x in xs:
        for y in (x if isinstance(x, (list, tuple)) else [x]):
            y.close()


root_bank = rm.root_bank


def test_root_motion_entry_points_are_declared_exported_and_bound(hip_lib):
    syms = declared_symbols()
    for name in ("mmdx_animator_root_motion", "mmdx_bone_motion_in_place", "mmdx_bone_motion_get_keys"):
        assert name in syms and hasattr(hip_lib, name) and name in api.SIGNATURES, name
    assert C.sizeof(api.BoneMotionKeys) == 4 * 4 + 6 * 8                    # four u32, six pointers
    hdr = open(os.path.join(ROOT, "include", "mmdx.h")).read()
    for text in ("typedef struct mmdx_root_motion_args {", "enum { MMDX_ROOT_X = 1u, MMDX_ROOT_Y = 2u, MMDX_ROOT_Z = 4u };",
                 "#define MMDX_ABI_VERSION 3u", "a one-bone bank, root_bone = 0", "a select, not a multiply",
                 "only when every moved bone descends from `bone`"):
        assert text in hdr, text
    assert hip_lib.mmdx_abi_version() == 3
    assert C.sizeof(api.RootMotionArgs) == 4 * 4 + 2 * 8                    # four u32, two pointers
    assert (api.ROOT_X, api.ROOT_Y, api.ROOT_Z) == (rm.ROOT_X, rm.ROOT_Y, rm.ROOT_Z) == (1, 2, 4)
    for name in ("root_motion", "step"):
        assert callable(getattr(vmd.Animator, name)), name
    assert callable(vmd.BoneMotion.in_place)
    poser = open(os.path.join(ROOT, "simple_mmd_renderer_amd", "host", "mmdx_poser.hpp")).read()
    for call in ("mmdx_animator_root_motion(", "mmdx_bone_motion_in_place("):
        assert call in poser, call


def test_fixture_clips_and_coverage():
    """The committed clips are what the issue asks for, and the golden rows go through every case it names."""
    vs = {n: vmd.Vmd(p) for n, p in rm.VMDS.items()}
    root = {n: next((v.bone_track(i) for i, t in enumerate(v.bone_track_names) if t == rm.ROOT_NAME), None) for n, v in vs.items()}
    assert root["no_root"] is None and len(root["still"]) == 1 and vs["still"].info["max_frame"] == 0
    first, last = root["curved"][0], root["curved"][-1]
    assert first["translation"] != last["translation"]                      # it does not close: R(L) != R(0)
    assert any(k["interpolation"][:16] != root["linear"][0]["interpolation"][:16] for k in root["curved"])
    assert len(root["linear"]) == 2 and all(os.path.getsize(p) < 8192 for p in rm.VMDS.values())
    names = rm.rig_small_names()
    assert rm.ROOT_NAME not in names and all(set(v.bone_track_names) - {rm.ROOT_NAME} <= set(names) for v in vs.values())
    ms = root_bank()
    assert ms.nb == 1 and ms.n_clips == rm.N_CLIPS
    assert ms.clip_frames().tolist() == [45, 30, 0, 0, 45, 30]
    whole = [v.bind_bones(names + [rm.ROOT_NAME]) for v in (vmd.Vmd(p) for p in rm.clip_paths())]
    full = vmd.MotionSet(whole)
    assert full.clip_frames().tolist() == list(rm.CLIP_FRAMES)
    an = vmd.Animator(ms, 2, [tuple(r) for r in rm.CLIP_ROWS])
    assert [r[0] for r in an.clip_table()] == rm.table()["length"].tolist()
    close_all(an, full, whole, ms, list(vs.values()))
    z = rm.fixture()
    assert 200 <= z["dt"].size <= 600
    rm.check_coverage(z)


def _assert_rows(got, z, what):
    assert np.array_equal(got["times"].view(np.uint64), z["times"].view(np.uint64)), what + ": the instants"
    assert np.array_equal(got["folded"], z["folded"]), what + ": the fold flags"
    gu.assert_bits_equal_or_both_nan(got["expect"], z["expect"], what + ": the placements")


def test_host_build_of_the_arithmetic_and_the_restatement_equal_the_golden_rows():
    """csrc/root_math.hpp through its stand-alone driver -- built plain, and with AddressSanitizer and UBSan -- and the numpy
    restatement, each fed libmmd's R values of the fixture: instants, fold flags and placements as bit patterns."""
    z = rm.fixture()
    tab = rm.table()
    assert not np.isnan(z["expect"]).any()
    for sanitize in (False, True):
        got = rm.run_math_driver(rm.build_math_driver(sanitize), tab, z, z["r"])
        _assert_rows(got, z, "sanitized driver" if sanitize else "plain driver")
    pl = rm.plan(rm.rows_as_state(z), tab, z["dt"])
    out, _ = rm.apply(rm.rows_as_state(z), tab, z["dt"], z["r"], z["axes"], z["placements"])
    _assert_rows(dict(times=pl["times"], folded=pl["folded"], expect=out[:, :3]), z, "the restatement")
    gu.assert_bits_equal(out[:, 3:], z["placements"][:, 3:], "the restatement leaves the fourth float and the heading alone")
    # the two statements agree away from the fixture too: a seeded crowd with R made up (the arithmetic does not care where R is from)
    rng = np.random.RandomState(5)
    n = 500
    rows = {k: z[k][rng.randint(0, z["dt"].size, n)] for k, _ in rm.ROW_ARRAYS}
    rows["times_a"], rows["times_b"] = rng.uniform(-0.2, 1.7, n), rng.uniform(-0.2, 1.7, n)
    rows["dt"] = rng.choice([1 / 60, 1 / 30, -1 / 60, 0.0, 3.1], n)
    r = rng.uniform(-3, 3, (n, 2, 4, 3)).astype(np.float32)
    r[rng.rand(n) < 0.05] = np.inf                                          # infinities propagate as IEEE gives them
    got = rm.run_math_driver(rm.build_math_driver(True), tab, rows, r)
    pl = rm.plan(rm.rows_as_state(rows), tab, rows["dt"])
    out, ev = rm.apply(rm.rows_as_state(rows), tab, rows["dt"], r, rows["axes"], rows["placements"])
    assert ev["fold_forwards"].sum() > 20 and ev["fold_backwards"].sum() > 20 and np.isnan(out).any()
    _assert_rows(got, dict(times=pl["times"], folded=pl["folded"], expect=out[:, :3]), "seeded rows")


@needs_driver
def test_libmmd_driver_reproduces_the_fixture():
    z = rm.fixture()
    got = rm.run_libmmd_driver(rm.table(), z)
    _assert_rows(got, z, "libmmd")
    gu.assert_bits_equal(got["r"], z["r"], "libmmd: R")


def test_dyadic_walk_has_a_closed_form_in_the_restatement():
    """Linear keys 0 -> 16 along Z over frames 0..64, played as a loop of a stated 2.0 s, dt = 1/32: every clock is a multiple of
    1/32 and every R a multiple of 15/64, so every step displaces the root by exactly 0.234375, across the loop seams as well.
    Under a heading whose matrix is exact -- a half turn about Y -- N steps give N * 0.234375 exactly, along -Z.  R is the lerp of
    the two keys as the evaluator computes it (tests/test_root_motion.py checks the kernel against this same walk)."""
    half, _ = dyadic_walk("half")
    assert half[-1].tolist() == [0, 0, -DYADIC_STEPS * 0.234375] and DYADIC_STEPS * 0.234375 == 37.5
    assert all(p.tolist() == [0, 0, -(k + 1) * 0.234375] for k, p in enumerate(half))
    # The quarter turn the issue asks for has NO exactly representable matrix: 1 - 2*j*j = 0 needs j*j = 0.5, and no binary32 j
    # squares to it (sqrt(0.5) rounded gives 0.49999997, so M = [[6e-8, 0, -0.99999994], ..., [0.99999994, 0, 6e-8]]).  So for that
    # heading the restatement is the yardstick (the GPU test compares with it bit for bit) and the closed form holds to rounding:
    quarter, m = dyadic_walk("quarter")
    assert m[8] == np.float32(0.99999994) and m[10] == np.float32(5.9604645e-08)
    want = DYADIC_STEPS * 0.234375
    assert abs(quarter[-1][0] - want) <= want * 2.0 ** -22 and abs(quarter[-1][2]) <= want * 2.0 ** -22 and quarter[-1][1] == 0


DYADIC_LENGTH, DYADIC_DT, DYADIC_STEPS = 2.0, 1 / 32, 160


def dyadic_placement(heading):
    """'half': a half turn about Y, q = (0, 1, 0, 0), whose matrix is exactly diag(-1, 1, -1): +Z becomes -Z.
    'quarter': a quarter turn about Y, q = (0, h, 0, h) with h = float(sqrt(0.5)): +Z becomes +X up to rounding."""
    h = np.float32(np.sqrt(0.5))
    p = np.zeros((1, 8), np.float32)
    p[0, 4:] = (0, 1, 0, 0) if heading == "half" else (0, h, 0, h)
    return p


def dyadic_walk(heading):
    """DYADIC_STEPS steps of the restatement -> (the placement's translation after every step, the heading's matrix)."""
    tab = rm.ar.table_of([(DYADIC_LENGTH, rm.ar.LOOP, rm.NONE, 0.0)])
    state = {k: v for k, v in rm.ar.initial_state(1).items()}
    state["clips_a"][:] = 0
    place = dyadic_placement(heading)
    m = rm.pp.matrix_from_pose(place)[0]
    if heading == "half":
        assert m[:11].tolist() == [-1, 0, 0, 0, 0, 1, 0, 0, 0, 0, -1]
    t, folds, out = 0.0, 0, []
    for _ in range(DYADIC_STEPS):
        state["times_a"][:] = t
        pl = rm.plan(state, tab, DYADIC_DT)
        place, ev = rm.apply(state, tab, DYADIC_DT, dyadic_r(pl["times"]), rm.ROOT_Z, place)
        folds += int(ev["fold_forwards"][0])
        t = rm.ar.wrap(tab, state["clips_a"], state["times_a"] + DYADIC_DT)[0][0]
        out.append(place[0, :3].copy())
    assert folds == 2
    return out, m


def dyadic_r(times):
    """R of the dyadic walk at `times` [N, 2, 4]: z = 16 * bary, bary = float((t * 30 - 0) / 64) clamped to the keys, as the time
    clock computes it; the lerp 0 * (1 - lam) + 16 * lam in float."""
    d = np.clip(np.asarray(times, np.float64) * 30.0, 0.0, 64.0)
    lam = (d / 64.0).astype(np.float32)
    r = np.zeros(times.shape + (3,), np.float32)
    r[..., 2] = np.float32(0) * (np.float32(1) - lam) + np.float32(16) * lam
    return r


def test_root_motion_refuses_bad_arguments():
    """Everything that needs no device is decided before the first HIP call."""
    lib = api.lib()
    err = lambda: lib.mmdx_last_error_string().decode()          # noqa: E731
    ms = root_bank()
    an = vmd.Animator(ms, 4)
    dt, nan = C.c_double(1 / 60), C.c_double(float("nan"))
    size = C.sizeof(api.RootMotionArgs)

    def call(a=an.h, s=ms.h, struct_size=size, flags=0, root_bone=0, axes=ALL_AXES, dt_ptr=C.addressof(dt), placements=4096, args=True):
        x = api.RootMotionArgs(struct_size, flags, root_bone, axes, dt_ptr, placements)
        return lib.mmdx_animator_root_motion(a, s, None, C.byref(x) if args else None)
    assert call(a=None) == 1 and "NULL" in err()
    assert call(s=None) == 1 and "NULL" in err()
    assert call(args=False) == 1 and "NULL" in err()
    assert call(dt_ptr=None) == 1 and "NULL" in err()
    assert call(placements=None) == 1 and "NULL" in err()
    for bad in (0, size - 8, size + 8):
        assert call(struct_size=bad) == 1 and "struct_size" in err()
    for bad in (1, 4, 1 << 9, 1 << 11, 1 << 31):
        assert call(flags=bad) == 1 and "unknown flag" in err(), bad
    for bad in (8, 16, 0xFFFFFFF8):
        assert call(axes=bad) == 1 and "axes" in err(), bad
    assert call(root_bone=1) == 2 and "root_bone = 1" in err()                                   # BAD_INDEX: a one-bone bank
    assert call(placements=4098) == 1 and "placements" in err() and "aligned" in err()
    assert call(flags=vmd.ANIM_DT_ON_DEVICE, dt_ptr=4100) == 1 and "8-byte" in err()
    assert call(dt_ptr=C.addressof(nan)) == 1 and "dt is NaN" in err()
    # another clip count; a set without a bone side
    v = vmd.Vmd(rm.VMDS["curved"])
    bm = v.bind_bones([rm.ROOT_NAME])
    short = vmd.MotionSet([bm, bm])
    assert call(s=short.h) == 1 and "clips" in err()
    mv = vmd.Vmd(mt.MORPH_VMD)
    mms = [mv.bind_morphs(mv.morph_track_names) for _ in range(rm.N_CLIPS)]
    morphs = vmd.MotionSet(morph_motions=mms)
    assert call(s=morphs.h) == 1 and "without bone" in err()
    # the Python face raises the same statuses
    with pytest.raises(api.MmdxError) as e:
        an.root_motion(ms, 3, ALL_AXES, 4096, dt=1 / 60)
    assert e.value.status == 2
    with pytest.raises(api.MmdxError) as e:
        an.step(ms, 0, 8, 4096, dt=1 / 60)
    assert e.value.status == 1
    with pytest.raises(ValueError):
        an.root_motion(ms, 0, ALL_AXES, 4096)
    with pytest.raises(ValueError):
        an.root_motion(ms, 0, ALL_AXES, 4096, dt=0.1, dt_ptr=4096)
    close_all(morphs, mms, mv, short, bm, v, an, ms)


def oracle_rows(keys, interp_of, names, frames, times):
    """The CPU oracle path over key tables: per model bone Motion::GetBonePose at whole frames (oracle.pyoracle.Oracle.bone_pose)
    and at times in seconds (tests/motion_time_restate.c) -> f32 [len(frames) + len(times), NB, 8].  The translations and
    rotations are the tables' own; the Bezier control bytes are the file's (the tables hold presampled curves, compared as bytes)."""
    from oracle.pyoracle import Oracle
    orc, lib = Oracle(), mt.restatement()
    out = np.zeros((len(frames) + len(times), len(names), 8), np.float32)
    one = np.zeros(8, np.float32)
    for b, name in enumerate(names):
        lo, hi = int(keys["key_off"][b]), int(keys["key_off"][b + 1])
        fr = np.ascontiguousarray(keys["key_frame"][lo:hi])
        tr = np.ascontiguousarray(keys["key_tr"][lo:hi, :3])
        rot = np.ascontiguousarray(keys["key_rot"][lo:hi])
        ip = np.ascontiguousarray(interp_of[name]) if hi > lo else np.zeros((1, 64), np.int8)
        assert ip.shape[0] == max(hi - lo, 1)
        for j, f in enumerate(frames):
            out[j, b] = orc.bone_pose(fr, tr, rot, ip, f)
        if hi == lo:
            fr, tr, rot = np.zeros(1, np.uint32), np.zeros((1, 3), np.float32), np.zeros((1, 4), np.float32)
        for j, t in enumerate(times):
            lib.mt_bone_pose_time(C.c_uint32(hi - lo), mt.ptr(fr, C.c_uint32), mt.ptr(tr, C.c_float), mt.ptr(rot, C.c_float),
                                  mt.ptr(ip, C.c_int8), C.c_double(float(t)), mt.ptr(one, C.c_float))
            out[len(frames) + j, b] = one
    return out


def test_in_place_tables_byte_for_byte_and_rows_on_the_cpu_oracle_path():
    """mmdx_bone_motion_in_place on the host alone.  The key tables of the copy (mmdx_bone_motion_get_keys) equal the source's
    byte for byte, except that the translation of every key of the chosen bone holds +0 on the axes named; and the rows the CPU
    oracle computes from the copy's tables, at whole frames and at the fixture's times, equal those of the source's tables in every
    bit, except that the root's masked channels are 0."""
    names = rm.rig_small_names() + [rm.ROOT_NAME]
    root = len(names) - 1
    z = rm.fixture()
    times = np.unique(np.concatenate([z["times"].reshape(-1), [-1.0, 0.4, 1.0, 9.0]]))
    frames = [0, 5, 12, 13, 31, 44, 45, 60]
    seen_zeroed = 0
    for clip in ("curved", "linear", "still", "no_root"):
        v = vmd.Vmd(rm.VMDS[clip])
        tracks = mt.tracks_of(v)
        bm = v.bind_bones(names)
        src = bm.keys()
        assert src["key_off"].size == len(names) + 1 and src["key_off"][-1] == src["key_frame"].size == bm.n_keys
        for b, name in enumerate(names):                                     # the accessor shows what the binder made of the file
            lo, hi = int(src["key_off"][b]), int(src["key_off"][b + 1])
            fr, tr, rot, _ = tracks.get(name, (np.zeros(0, np.uint32), np.zeros((0, 3), np.float32), np.zeros((0, 4), np.float32), None))
            assert src["key_frame"][lo:hi].tolist() == fr.tolist(), (clip, name)
            gu.assert_bits_equal(src["key_tr"][lo:hi, :3], tr, f"{clip}, {name}: translations")
            gu.assert_bits_equal(src["key_rot"][lo:hi], rot, f"{clip}, {name}: rotations")
        interp_of = {n: t[3] for n, t in tracks.items()}
        src_rows = oracle_rows(src, interp_of, names, frames, times)
        lo, hi = int(src["key_off"][root]), int(src["key_off"][root + 1])
        if clip == "curved":
            assert hi - lo == 4 and (src["key_tr"][lo:hi, :3] != 0).any(0).all() and (src_rows[:, root, :3] != 0).any(0).all()
        for axes in range(8):
            ip = bm.in_place(root, axes)
            got = ip.keys()
            for k in ("key_off", "key_frame", "key_rot", "key_curve", "lut"):
                assert got[k].tobytes() == src[k].tobytes(), (clip, axes, k)
            want = src["key_tr"].copy()
            for c in range(3):
                if axes & (1 << c):
                    want[lo:hi, c] = 0.0
            assert got["key_tr"].tobytes() == want.tobytes(), (clip, axes)       # +0.0f: all bits clear
            seen_zeroed += int((got["key_tr"].view(np.uint32) != src["key_tr"].view(np.uint32)).sum())
            if axes in (ALL_AXES, api.ROOT_X | api.ROOT_Z, api.ROOT_Y):
                rows = oracle_rows(got, interp_of, names, frames, times)
                want_rows = src_rows.copy()
                for c in range(3):
                    if axes & (1 << c):
                        want_rows[:, root, c] = 0.0
                gu.assert_bits_equal(rows, want_rows, f"{clip}, axes {axes}: rows on the CPU oracle path")
            # the source is not touched, and a copy of the copy zeroes the rest
            assert bm.keys()["key_tr"].tobytes() == src["key_tr"].tobytes()
            again = ip.in_place(root, ALL_AXES)
            assert not again.keys()["key_tr"][lo:hi, :3].any()
            close_all(again, ip)
        # another bone: only its keys
        other = bm.in_place(1, ALL_AXES)
        a, b = int(src["key_off"][1]), int(src["key_off"][2])
        want = src["key_tr"].copy()
        want[a:b, :3] = 0.0
        assert other.keys()["key_tr"].tobytes() == want.tobytes(), clip
        close_all(other, bm, v)
    assert seen_zeroed >= 12 * 4                                             # curved: 4 keys x 3 channels, over the eight masks
    lib = api.lib()
    k = api.BoneMotionKeys(C.sizeof(api.BoneMotionKeys))
    assert lib.mmdx_bone_motion_get_keys(None, C.byref(k)) == 1 and lib.mmdx_bone_motion_get_keys(None, None) == 1


def test_in_place_refusals_and_shape():
    lib = api.lib()
    err = lambda: lib.mmdx_last_error_string().decode()          # noqa: E731
    names = rm.rig_small_names() + [rm.ROOT_NAME]
    v = vmd.Vmd(rm.VMDS["curved"])
    bm = v.bind_bones(names)
    h = C.c_void_p()
    root = len(names) - 1
    assert lib.mmdx_bone_motion_in_place(None, root, ALL_AXES, C.byref(h)) == 1 and "NULL" in err()
    assert lib.mmdx_bone_motion_in_place(bm.h, root, ALL_AXES, None) == 1 and "NULL" in err()
    assert lib.mmdx_bone_motion_in_place(bm.h, root, 8, C.byref(h)) == 1 and "axes" in err()
    assert lib.mmdx_bone_motion_in_place(bm.h, len(names), ALL_AXES, C.byref(h)) == 2 and "bone = %d" % len(names) in err()
    assert h.value is None
    for axes in range(8):
        ip = bm.in_place(root, axes)
        assert (ip.nb, ip.n_mapped, ip.n_keys, ip.n_curves) == (bm.nb, bm.n_mapped, bm.n_keys, bm.n_curves)
        both = vmd.MotionSet([bm, ip])
        assert both.clip_frames().tolist() == [45, 45]
        close_all(both, ip)
    with pytest.raises(api.MmdxError) as e:
        bm.in_place(len(names), ALL_AXES)
    assert e.value.status == 2
    ip = bm.in_place(root, ALL_AXES)
    bm.close()                                                   # the copy owns its tables
    assert ip.n_keys > 0
    close_all(ip, v)

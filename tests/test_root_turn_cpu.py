"""Root motion that turns, without a GPU: mmdx_animator_root_motion_turn and mmdx_bone_motion_in_place_turn (include/mmdx.h).

The contract is the arithmetic the header states.  Here it is held by the golden rows of the real libmmd
(tests/golden/root_turn_expect.npz, tests/root_turn_driver.cpp) against two statements that must agree with them bit for bit:
csrc/root_math.hpp compiled for the host (tests/root_turn_math_driver.cpp, a stand-alone program, plain and sanitized) and the numpy
restatement tests/root_turn_ref.py.  Two closure tests hold the definition itself -- the product order and the frames -- against
W_p' = W_root(t1) * W_root(t0)^-1 * W_p in float64.  tests/test_root_turn.py runs the same rows through the gfx950 kernel.
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
from tests import root_turn_ref as rt
from tests import test_root_motion_cpu as plain
from tests.test_capi_symbols import declared_symbols

F = np.float32
ROOT = os.path.dirname(mt.HERE)
needs_driver = pytest.mark.skipif(not mt.driver_available(), reason="the reference's libmmd headers are not present")
ALL_AXES = api.ROOT_X | api.ROOT_Y | api.ROOT_Z
_close = plain.close_all


@pytest.fixture(autouse=True)
def _lib(hip_lib):
    return hip_lib


def test_root_turn_entry_points_are_declared_exported_and_bound(hip_lib):
    syms = declared_symbols()
    for name in ("mmdx_animator_root_motion_turn", "mmdx_bone_motion_in_place_turn"):
        assert name in syms and hasattr(hip_lib, name) and name in api.SIGNATURES, name
    hdr = open(os.path.join(ROOT, "include", "mmdx.h")).read()
    for text in ("typedef struct mmdx_root_turn_args {", "enum { MMDX_ROOT_NORMALIZE = 1u << 14 };", "#define MMDX_ABI_VERSION 3u",
                 "mmdx_animator_root_motion_turn with mmdx_root_turn_args and MMDX_ROOT_NORMALIZE", "h' = h * dq",
                 "D = d1 + rotate(d2, M(dq1));  dq = dq1 * dq2", "the split is faithful\n * only when every moved bone descends from `bone`"):
        assert text in hdr, text
    assert "Turning is out of scope" not in hdr
    assert hip_lib.mmdx_abi_version() == 3
    assert C.sizeof(api.RootTurnArgs) == C.sizeof(api.RootMotionArgs) == 4 * 4 + 2 * 8           # four u32, two pointers
    assert api.RootTurnArgs is not api.RootMotionArgs
    # the lowest bit no other call accepts: every flag enumerator of the header below it is taken
    assert api.ROOT_NORMALIZE == rt.ROOT_NORMALIZE == 1 << 14
    taken = {int(s.split("<<")[1].split()[0].rstrip(",;")) for s in hdr.split("\n") if "= 1u <<" in s and "MMDX_CREATE" not in s
             and "MMDX_SKELETON" not in s}
    assert set(range(14)) <= taken and max(taken) == 14, sorted(taken)
    for name in ("root_turn", "step"):
        assert callable(getattr(vmd.Animator, name)), name
    assert callable(vmd.BoneMotion.in_place_turn)
    poser = open(os.path.join(ROOT, "simple_mmd_renderer_amd", "host", "mmdx_poser.hpp")).read()
    for call in ("mmdx_animator_root_motion_turn(", "mmdx_bone_motion_in_place_turn(", "void RootTurn(", "void RootTurnDeviceDt(",
                 "void StepTurn("):
        assert call in poser, call


def test_fixture_clips_and_coverage():
    """root_q8 is what the issue asks for, and the golden rows go through every case it names."""
    v = vmd.Vmd(rt.Q8_VMD)
    assert os.path.getsize(rt.Q8_VMD) < 8192
    root = next(v.bone_track(i) for i, t in enumerate(v.bone_track_names) if t == rt.ROOT_NAME)
    assert [k["frame"] for k in root] == [0, 15, 30, 45, 60]
    linear = vmd.Vmd(rm.VMDS["linear"])
    lin = next(linear.bone_track(i) for i, t in enumerate(linear.bone_track_names) if t == rt.ROOT_NAME)
    assert all(k["interpolation"][:16] == lin[0]["interpolation"][:16] for k in root)             # linear curves
    group = {tuple(s * (1.0 if k == c else 0.0) for k in range(4)) for c in range(4) for s in (1.0, -1.0)}
    rots = [tuple(abs(x) * (1 if x > 0 else -1) if x else 0.0 for x in k["rotation"]) for k in root]
    assert all(r in group for r in rots) and (0.0, 1.0, 0.0, 0.0) in rots and len(set(rots)) == 5
    for k in root:
        assert all(float(x) * 8 == int(float(x) * 8) and abs(x) <= 2 for x in k["translation"])   # small and dyadic
    assert root[0]["translation"] != root[-1]["translation"]                                       # R(L) != R(0)
    assert [(k["frame"], tuple(k["translation"]), tuple(k["rotation"])) for k in root] == [(f, t, q) for f, t, q in rt.Q8_KEYS]
    _close(linear, v)
    ms = rt.root_bank()
    assert ms.nb == 1 and ms.n_clips == rt.N_CLIPS and ms.clip_frames().tolist() == [45, 30, 0, 0, 45, 30, 60]
    an = vmd.Animator(ms, 2, [tuple(r) for r in rt.CLIP_ROWS])
    assert [r[0] for r in an.clip_table()] == rt.table()["length"].tolist()
    _close(an, ms)
    z = rt.fixture()
    assert 200 <= z["dt"].size <= 600 and os.path.getsize(rt.FIXTURE) < 10 * os.path.getsize(rm.FIXTURE)
    rt.check_coverage(z)


def _assert_rows(got, z, what):
    assert np.array_equal(got["times"].view(np.uint64), z["times"].view(np.uint64)), what + ": the instants"
    assert np.array_equal(got["folded"], z["folded"]), what + ": the fold flags"
    gu.assert_bits_equal_or_both_nan(got["expect"][:, :3], z["expect"][:, :3], what + ": the positions")
    gu.assert_bits_equal_or_both_nan(got["expect"][:, 4:], z["expect"][:, 4:], what + ": the headings")
    gu.assert_bits_equal(got["expect"][:, 3], z["expect"][:, 3], what + ": the fourth float")


def _restated(rows, tab, t, q):
    pl = rm.plan(rt.rows_as_state(rows), tab, rows["dt"])
    out, ev = rt.apply(rt.rows_as_state(rows), tab, rows["dt"], t, q, rows["axes"], (rows["flags"] & rt.ROOT_NORMALIZE) != 0,
                       rows["placements"])
    return dict(times=pl["times"], folded=pl["folded"], expect=out), ev


def test_host_build_of_the_arithmetic_and_the_restatement_equal_the_golden_rows():
    """csrc/root_math.hpp through its stand-alone driver -- built plain, and with AddressSanitizer and UBSan -- and the numpy
    restatement, each fed libmmd's (T, Q) of the fixture: instants, fold flags, positions and headings as bit patterns."""
    z = rt.fixture()
    tab = rt.table()
    assert not np.isnan(z["expect"]).any()
    gu.assert_bits_equal(z["expect"][:, 3], z["placements"][:, 3], "the fixture leaves the fourth float alone")
    nan_dt = np.isnan(z["dt"])
    gu.assert_bits_equal(z["expect"][nan_dt], z["placements"][nan_dt], "a NaN dt writes nothing")
    for sanitize in (False, True):
        got = rt.run_math_driver(rt.build_math_driver(sanitize), tab, z, z["t"], z["q"])
        _assert_rows(got, z, "sanitized driver" if sanitize else "plain driver")
    got, _ = _restated(z, tab, z["t"], z["q"])
    _assert_rows(got, z, "the restatement")
    # the two statements agree away from the fixture too: a seeded crowd with (T, Q) made up
    rng = np.random.RandomState(6)
    n = 500
    rows = {k: z[k][rng.randint(0, z["dt"].size, n)] for k, _ in rt.ROW_ARRAYS}
    rows["times_a"], rows["times_b"] = rng.uniform(-0.2, 1.7, n), rng.uniform(-0.2, 1.7, n)
    rows["dt"] = rng.choice([1 / 60, 1 / 30, -1 / 60, 0.0, 3.1], n)
    t = rng.uniform(-3, 3, (n, 2, 4, 3)).astype(F)
    q = rng.normal(size=(n, 2, 4, 4)).astype(F)                             # not normalised: the arithmetic does not care
    t[rng.rand(n) < 0.05] = np.inf                                          # infinities propagate as IEEE gives them
    q[rng.rand(n) < 0.03, :, :, 1] = np.inf
    got = rt.run_math_driver(rt.build_math_driver(True), tab, rows, t, q)
    want, ev = _restated(rows, tab, t, q)
    assert ev["fold_forwards_a"].sum() > 10 and ev["fold_backwards_b"].sum() > 5 and ev["mix"].sum() > 50
    assert np.isnan(want["expect"]).any()                                   # (an infinite T gives inf - inf)
    _assert_rows(got, want, "seeded rows")


@needs_driver
def test_libmmd_driver_reproduces_the_fixture():
    """Where libmmd's headers are present the fixture regenerates identically: the rows from the generator's recipe, every
    number from the real libmmd."""
    from tests import gen_root_turn_golden as gen
    z = rt.fixture()
    rows = gen.cases()
    for k, _ in rt.ROW_ARRAYS:
        assert np.ascontiguousarray(rows[k]).tobytes() == np.ascontiguousarray(z[k]).tobytes(), k
    got = rt.run_libmmd_driver(rt.table(), rows)
    _assert_rows(got, z, "libmmd")
    gu.assert_bits_equal(got["t"], z["t"], "libmmd: T")
    gu.assert_bits_equal(got["q"], z["q"], "libmmd: Q")


# ---------------------------------------------------------------------------------------- closure ----
Q8_PLACE = np.array([3.0, -1.5, 0.25, 0.625, 0.0, 1.0, 0.0, 0.0], F)        # a half-turn heading: an exact matrix


def q8_walk(normalize=False):
    def tq_of(times, pl):
        return rt.q8_at(times)                                               # (an instant that is not sampled is 0.0, a key)
    return rt.walk(rt.Q8, 0.0, rt.Q8_DT, rt.Q8_STEPS, Q8_PLACE, tq_of, normalize)


def test_exact_closure_on_the_quaternion_group():
    """root_q8 played from 0 with dt = 0.5: every sample lands on a key, every rotation is one of {+-1, +-i, +-j, +-k} and every
    translation dyadic, so every product is exact.  For 12 steps -- three laps: two seams inside the walk and a third that the twelfth
    step lands on -- the placement as a matrix equals
    W_root(t_k) * W_root(t_0)^-1 * W_p0 evaluated in float64, continued past each seam as the definition's fold gives it, with no
    tolerance; before the first seam that is the closed form itself."""
    for normalize in (False, True):
        out, mats, folds = q8_walk(normalize)
        assert folds == 3
        for k in range(rt.Q8_STEPS):
            assert np.array_equal(rt.world(out[k, :3], out[k, 4:]), mats[k]), (normalize, k)
            assert out[k, 3] == Q8_PLACE[3]
        w0 = rt.world(Q8_PLACE[:3], Q8_PLACE[4:])
        start = rt.world(*[a[0] for a in rt.q8_at(np.array([0.0]))])
        for k in range(3):                                                   # t = 0.5, 1.0, 1.5: no seam yet
            t, q = rt.q8_at(np.array([(k + 1) * 0.5]))
            assert np.array_equal(rt.world(out[k, :3], out[k, 4:]), rt.world(t[0], q[0]) @ np.linalg.inv(start) @ w0), k
        assert len({o.tobytes() for o in out[:, 4:]}) >= 4 and len({o.tobytes() for o in out[:, :3]}) >= 8
    # the walk does not close (R(L) != R(0)): a lap later the placement has moved on
    assert not np.array_equal(out[3, :3], Q8_PLACE[:3])


CURVED_PLACE = np.array([3.0, -2.0, 5.0, 0.5, 0.18257419, 0.36514837, 0.54772256, 0.73029674], F)     # (1, 2, 3, 4) / sqrt(30)


def curved_walk(normalize):
    """45 steps of 1/30 s along root_curved from t = 0 under a unit heading, (T, Q) from the fixture's walk rows (libmmd's)."""
    z = rt.fixture()
    rows = z["walk"]
    assert rows.size == 45
    step = iter(rows)

    def tq_of(times, pl):
        i = next(step)
        assert np.array_equal(times[0].view(np.uint64), z["times"][i].view(np.uint64)), i
        return z["t"][i:i + 1], z["q"][i:i + 1]
    out, mats, folds = rt.walk(0, 0.0, 1 / 30, 45, CURVED_PLACE, tq_of, normalize)
    return out, mats, folds, np.abs(z["t"][rows]).max()


def test_general_closure_on_the_curved_walk():
    """The placement stays within N * 64 * 2^-24 * (1 + max|T| + max|p0|) per component of the float64 chain
    W_root(t_k) * W_root(t_0)^-1 * W_p0, N the number of steps taken.  The bound is derived -- a step is tens of roundings, each at
    most 2^-24 of a value below 1 + max|T| + max|p0| -- and loose on purpose: a wrong product order or frame misses it by orders of
    magnitude.  Measured with the restatement: the worst of the 45 steps uses 0.0036 of its bound, 0.0015 with the normalisation
    (printed)."""
    for normalize in (False, True):
        out, mats, folds, t_max = curved_walk(normalize)
        assert folds <= 1 and abs(np.linalg.norm(CURVED_PLACE[4:].astype(np.float64)) - 1) < 1e-6
        scale = 1 + t_max + np.abs(CURVED_PLACE[:3]).max()
        worst = 0.0
        for k in range(45):
            err = np.abs(rt.world(out[k, :3], out[k, 4:]) - mats[k]).max()
            bound = (k + 1) * 64 * 2.0 ** -24 * scale
            worst = max(worst, err / bound)
            assert err <= bound, (normalize, k, err, bound)
        print("curved walk, normalize=%s: worst error / bound = %.4f" % (normalize, worst))
        # the closed form over the whole walk, where no seam intervened: W_root(t_k) * W_root(0)^-1 * W_p0
        z = rt.fixture()
        first, k = z["walk"][0], 43
        row = z["walk"][k]
        assert not z["folded"][z["walk"][:k + 1]].any()
        direct = rt.world(z["t"][row, 0, 1], z["q"][row, 0, 1]) @ np.linalg.inv(rt.world(z["t"][first, 0, 0], z["q"][first, 0, 0])) \
            @ rt.world(CURVED_PLACE[:3], CURVED_PLACE[4:])
        assert np.abs(rt.world(out[k, :3], out[k, 4:]) - direct).max() <= (k + 1) * 64 * 2.0 ** -24 * scale
        # what the bound is there to catch: the displacement taken in the clip's frame, not the root's, misses it by far
        wrong = CURVED_PLACE[:3].astype(np.float64) + (z["t"][row, 0, 1] - z["t"][first, 0, 0]).astype(np.float64) @ \
            rt.world((0, 0, 0), CURVED_PLACE[4:])[:3, :3]
        assert np.abs(wrong - direct[3, :3]).max() > 100 * (k + 1) * 64 * 2.0 ** -24 * scale


def test_identity_rotations_give_the_plain_call():
    """On root_linear, whose root keys all carry the identity, the turn call moves the positions as the plain call's restatement
    does (equal as values, +-0 alike) and leaves the heading unchanged as values."""
    v = vmd.Vmd(rm.VMDS["linear"])
    rng = np.random.RandomState(11)
    n = 96
    state = rm.ar.initial_state(n)
    state["clips_a"][:], state["clips_b"][:] = 1, 1
    state["times_a"][:], state["times_b"][:] = rng.uniform(0, 1, n), rng.uniform(0, 1, n)
    state["weights"][:] = rng.choice(rm.mb.WEIGHTS, n)
    state["fade_rate"][:] = rng.choice([0.0, 2.0], n)
    state["speed"][:] = rng.choice([1.0, -1.0, 0.5, 3.0], n)
    tab = rt.table()
    dt = 1 / 10
    pl = rm.plan(state, tab, dt)
    assert pl["folded"][:, 0].sum() >= 8 and pl["folded"][:, 1].sum() >= 4
    rows = mt.restate_poses(v, [rt.ROOT_NAME], pl["times"].reshape(-1))[:, 0].reshape(n, 2, 4, 8)
    t, q = rows[..., :3], rows[..., 4:]
    assert (q == rt.IDENTITY).all() and (t[..., 2] != 0).any()
    place = np.concatenate([rng.uniform(-20, 20, (n, 4)), rng.normal(size=(n, 4))], 1).astype(F)
    for axes in (ALL_AXES, api.ROOT_Z, api.ROOT_X | api.ROOT_Y):
        want, ev = rm.apply(state, tab, dt, t, axes, place)
        got, _ = rt.apply(state, tab, dt, t, q, axes, False, place)
        assert np.array_equal(got[:, :3], want[:, :3]), axes
        assert np.array_equal(got[:, 3:], place[:, 3:]), axes
        assert ev["moved"].sum() >= n // 2 or axes != ALL_AXES
    v.close()


# ---------------------------------------------------------------------------------------- in place ----
def test_in_place_turn_tables_byte_for_byte_and_rows_on_the_cpu_oracle_path():
    """mmdx_bone_motion_in_place_turn on the host alone.  The key tables of the copy equal the source's byte for byte outside the
    zeroed translation floats and the rotations of the chosen bone, which are {+0,+0,+0,1}, for every axes; the rows the CPU oracle
    computes from the copy's tables, at whole frames and at the fixture's times, are the source's except the root's masked channels
    and a root rotation of exactly {0,0,0,1}."""
    names = rm.rig_small_names() + [rt.ROOT_NAME]
    root = len(names) - 1
    z = rt.fixture()
    times = np.unique(np.concatenate([z["times"].reshape(-1), [-1.0, 0.4, 1.0, 9.0]]))[::3]
    frames = [0, 5, 12, 15, 22, 31, 44, 45, 60]
    ident = np.array([0, 0, 0, 1], F)
    turned_keys = 0
    for clip, path in (("curved", rm.VMDS["curved"]), ("q8", rt.Q8_VMD), ("still", rm.VMDS["still"]), ("no_root", rm.VMDS["no_root"])):
        v = vmd.Vmd(path)
        tracks = mt.tracks_of(v)
        bm = v.bind_bones(names)
        src = bm.keys()
        interp_of = {n: t[3] for n, t in tracks.items()}
        src_rows = plain.oracle_rows(src, interp_of, names, frames, times)
        lo, hi = int(src["key_off"][root]), int(src["key_off"][root + 1])
        if clip in ("curved", "q8"):
            assert hi - lo >= 4 and (src_rows[:, root, 4:] != ident).any(1).sum() > len(times) // 2
        for axes in range(8):
            ip = bm.in_place_turn(root, axes)
            got = ip.keys()
            for k in ("key_off", "key_frame", "key_curve", "lut"):
                assert got[k].tobytes() == src[k].tobytes(), (clip, axes, k)
            want_tr, want_rot = src["key_tr"].copy(), src["key_rot"].copy()
            for c in range(3):
                if axes & (1 << c):
                    want_tr[lo:hi, c] = 0.0
            want_rot[lo:hi] = ident
            assert got["key_tr"].tobytes() == want_tr.tobytes(), (clip, axes)
            assert got["key_rot"].tobytes() == want_rot.tobytes(), (clip, axes)   # +0.0f: all bits clear; 1.0f
            turned_keys += int((got["key_rot"].view(np.uint32) != src["key_rot"].view(np.uint32)).any(1).sum())
            if axes in (ALL_AXES, api.ROOT_X | api.ROOT_Z, 0):
                rows = plain.oracle_rows(got, interp_of, names, frames, times)
                want_rows = src_rows.copy()
                for c in range(3):
                    if axes & (1 << c):
                        want_rows[:, root, c] = 0.0
                want_rows[:, root, 4:] = ident
                gu.assert_bits_equal(rows, want_rows, f"{clip}, axes {axes}: rows on the CPU oracle path")
            assert bm.keys()["key_rot"].tobytes() == src["key_rot"].tobytes()    # the source is not touched
            # the plain copy of the same axes differs in the rotations only
            only = bm.in_place(root, axes)
            assert only.keys()["key_tr"].tobytes() == got["key_tr"].tobytes() and only.keys()["key_rot"].tobytes() == src["key_rot"].tobytes()
            _close(only, ip)
        _close(bm, v)
    assert turned_keys >= 8 * (4 + 4)
    # refusals, as mmdx_bone_motion_in_place
    lib = api.lib()
    err = lambda: lib.mmdx_last_error_string().decode()          # noqa: E731
    v = vmd.Vmd(rt.Q8_VMD)
    bm = v.bind_bones(names)
    h = C.c_void_p()
    assert lib.mmdx_bone_motion_in_place_turn(None, root, ALL_AXES, C.byref(h)) == 1 and "NULL" in err()
    assert lib.mmdx_bone_motion_in_place_turn(bm.h, root, ALL_AXES, None) == 1 and "NULL" in err()
    assert lib.mmdx_bone_motion_in_place_turn(bm.h, root, 8, C.byref(h)) == 1 and "axes" in err()
    assert lib.mmdx_bone_motion_in_place_turn(bm.h, len(names), ALL_AXES, C.byref(h)) == 2 and "bone = %d" % len(names) in err()
    assert h.value is None
    with pytest.raises(api.MmdxError) as e:
        bm.in_place_turn(len(names), ALL_AXES)
    assert e.value.status == 2
    ip = bm.in_place_turn(root, ALL_AXES)
    assert (ip.nb, ip.n_mapped, ip.n_keys, ip.n_curves) == (bm.nb, bm.n_mapped, bm.n_keys, bm.n_curves)
    bm.close()                                                   # the copy owns its tables
    assert ip.n_keys > 0
    _close(ip, v)


# ---------------------------------------------------------------------------------------- refusals ----
def test_root_turn_refuses_bad_arguments():
    """Every refusal of the plain call, decided before the first HIP call; the flags are the call's own two."""
    lib = api.lib()
    err = lambda: lib.mmdx_last_error_string().decode()          # noqa: E731
    ms = rt.root_bank()
    an = vmd.Animator(ms, 4)
    dt, nan = C.c_double(1 / 60), C.c_double(float("nan"))
    size = C.sizeof(api.RootTurnArgs)
    both = vmd.ANIM_DT_ON_DEVICE | api.ROOT_NORMALIZE

    def call(a=an.h, s=ms.h, struct_size=size, flags=0, root_bone=0, axes=ALL_AXES, dt_ptr=C.addressof(dt), placements=4096, args=True):
        x = api.RootTurnArgs(struct_size, flags, root_bone, axes, dt_ptr, placements)
        return lib.mmdx_animator_root_motion_turn(a, s, None, C.byref(x) if args else None)
    assert call(a=None) == 1 and "NULL" in err()
    assert call(s=None) == 1 and "NULL" in err()
    assert call(args=False) == 1 and "NULL" in err()
    assert call(dt_ptr=None) == 1 and "NULL" in err()
    assert call(placements=None) == 1 and "NULL" in err()
    for bad in (0, size - 8, size + 8):
        assert call(struct_size=bad) == 1 and "mmdx_root_turn_args.struct_size" in err()
    for bad in (1, 4, 1 << 9, 1 << 11, 1 << 13, 1 << 15, 1 << 31, both | 1, both | (1 << 15), both | (1 << 11)):
        assert call(flags=bad) == 1 and "unknown flag" in err(), bad
    # the two allowed bits pass the flag check: the refusal is a later one
    for good in (api.ROOT_NORMALIZE, vmd.ANIM_DT_ON_DEVICE, both):
        assert call(flags=good, root_bone=1, dt_ptr=4096) == 2 and "root_bone = 1" in err(), good
    # ... and the plain call still refuses the new bit
    x = api.RootMotionArgs(C.sizeof(api.RootMotionArgs), api.ROOT_NORMALIZE, 0, ALL_AXES, C.addressof(dt), 4096)
    assert lib.mmdx_animator_root_motion(an.h, ms.h, None, C.byref(x)) == 1 and "unknown flag" in err()
    for bad in (8, 16, 0xFFFFFFF8):
        assert call(axes=bad) == 1 and "axes" in err(), bad
    assert call(root_bone=1) == 2 and "root_bone = 1" in err()                                   # BAD_INDEX: a one-bone bank
    assert call(placements=4098) == 1 and "placements" in err() and "aligned" in err()
    assert call(flags=both, dt_ptr=4100) == 1 and "8-byte" in err()
    assert call(dt_ptr=C.addressof(nan)) == 1 and "dt is NaN" in err()
    assert call(flags=api.ROOT_NORMALIZE, dt_ptr=C.addressof(nan)) == 1 and "dt is NaN" in err()
    # another clip count; a set without a bone side
    v = vmd.Vmd(rm.VMDS["curved"])
    bm = v.bind_bones([rt.ROOT_NAME])
    short = vmd.MotionSet([bm, bm])
    assert call(s=short.h) == 1 and "clips" in err()
    mv = vmd.Vmd(mt.MORPH_VMD)
    mms = [mv.bind_morphs(mv.morph_track_names) for _ in range(rt.N_CLIPS)]
    morphs = vmd.MotionSet(morph_motions=mms)
    assert call(s=morphs.h) == 1 and "without bone" in err()
    # the Python face raises the same statuses
    with pytest.raises(api.MmdxError) as e:
        an.root_turn(ms, 3, ALL_AXES, 4096, dt=1 / 60, normalize=True)
    assert e.value.status == 2
    with pytest.raises(api.MmdxError) as e:
        an.step(ms, 0, 8, 4096, dt=1 / 60, turn=True)
    assert e.value.status == 1
    with pytest.raises(ValueError):
        an.root_turn(ms, 0, ALL_AXES, 4096)
    with pytest.raises(ValueError):
        an.root_turn(ms, 0, ALL_AXES, 4096, dt=0.1, dt_ptr=4096)
    with pytest.raises(ValueError):
        an.step(ms, 0, ALL_AXES, 4096, dt=0.1, normalize=True)              # normalize is the turn call's
    _close(morphs, mms, mv, short, bm, v, an, ms)

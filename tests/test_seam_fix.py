"""The physics seam's Fix at every pivot order and exit of its 4x4 inverse (tests/seam_cases.py: one 8-bone rig, seven override
lists, a crowd of 136 steered matrices classified by Oracle.trace_inverse).

CPU: the crowd holds every class of tests/golden/seam_fix_classes.json (24 pivot orders with finite palettes, both zero exits,
ties, zero pivots, NaN / inf / denormal / huge / mixed-scale rows); every traced input through libmmd's own Matrix4f::Inverse;
every list through libmmd's Poser; the committed libmmd palettes (tests/golden/seam_fix_expect.npz) equal a fresh run.
GPU: mmdx_skeleton_solve_pre / _post bit for bit against the oracle and the libmmd fixture -- whole crowd and cut to 1, 63, 64, 65
and 130 instances; device-resident operands (MMDX_OVERRIDES_ON_DEVICE, never run before); MMDX_SOLVE_DENSE=0/1 and
MMDX_SOLVE_SEQUENTIAL=1; the island appended to the 60-bone IK + append rig of test_physics_seam.physics_case; frames that follow
one another on one skeleton; strict == NULL and n_bones == 0."""
import ctypes as C
import os

import numpy as np
import pytest

from oracle.pyoracle import Oracle, Reference, reference_available
from simple_mmd_renderer_amd import _capi as api
from simple_mmd_renderer_amd import vmd
from simple_mmd_renderer_amd.engine import DeviceBuffer
from tests import golden_util as gu
from tests import seam_cases as sc
from tests.test_physics_seam import GOLDEN as PHYSICS_GOLDEN
from tests.test_physics_seam import physics_case, random_transforms
from tests.test_rig import random_poses

T = sc.T
NEEDS_REF = pytest.mark.skipif(not reference_available(), reason="oracle/_ref/libmmd_ref.so not built")
ENV = ("MMDX_SOLVE_DENSE", "MMDX_IK_COOP", "MMDX_SOLVE_SEQUENTIAL")


def assert_same(got, want, what):
    """Bit for bit; where `want` holds a NaN, NaN exactly there (a NaN's sign and payload differ between x86 and the GPU)."""
    if np.isnan(want).any():
        gu.assert_bits_equal_or_both_nan(got, want, what)
        assert np.array_equal(np.isnan(got), np.isnan(want)), what + ": NaN positions differ"
    else:
        gu.assert_bits_equal(got, want, what)


def assert_crowd(got, want, what, rows=None):
    kinds = sc.crowd().kinds
    for k, i in enumerate(range(got.shape[0]) if rows is None else rows):
        assert_same(got[k], want[i], f"{what}: instance {i} ({kinds[i]})")


# ---- CPU: the trace ------------------------------------------------------------------------------------------------------------------
def test_trace_records_say_what_the_inverse_did(oracle):
    """Matrices whose elimination can be followed by hand."""
    perm = np.zeros((4, 4), np.float32)
    for k, r in enumerate((2, 0, 3, 1)):                    # row r is the pivot of column k
        perm[r, k] = k + 2
    zero2 = np.arange(1, 17, dtype=np.float32).reshape(4, 4)
    zero2[2] = (0.0, -0.0, 0.0, 0.0)
    col3 = np.eye(4, dtype=np.float32)
    col3[3] = (0, 0, 1, 0)                                  # rows 2 and 3 are one row: a tie at column 2, then a zero last pivot
    tie = np.asarray([[2, 1, 0, 0], [-2, 0, 1, 0], [0, 0, 1, 1], [0, 1, 0, 3]], np.float32)    # rows 0 and 1 tie at column 0
    zp = np.asarray([[0, 1, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1], [0, 1, 1, 1]], np.float32)      # column 0 is zero: 0 / 0
    nan = np.eye(4, dtype=np.float32)
    nan[1, 2] = np.nan
    ms = [np.eye(4, dtype=np.float32), perm, zero2, col3, tie, zp, nan]
    outs = []
    rec = oracle.trace_inverse(lambda: outs.extend(oracle.matrix_inverse(m) for m in ms))
    assert rec.shape == (len(ms), len(Oracle.INVERSE_TRACE_FIELDS))
    none = Oracle.INVERSE_NONE
    for k, m in enumerate(ms):
        assert np.array_equal(rec[k, :16], gu.bits(m).reshape(16)), k
    field = lambda k, *names: tuple(int(rec[k, T[n]]) for n in names)       # noqa: E731
    full = ("pivot0", "pivot1", "pivot2", "exit", "zero_row", "ties", "zero_pivots", "nonfinite")
    assert field(0, *full) == (0, 1, 2, 0, none, 0, 0, 0)
    assert field(1, *full) == (2, 0, 3, 0, none, 0, 0, 0)
    assert field(2, *full) == (none, none, none, 1, 2, 0, 0, 0) and not outs[2].any()
    assert field(3, *full) == (0, 1, 2, 2, none, 4, 0, 0) and not outs[3].any()
    assert field(4, "pivot0", "exit", "ties") == (0, 0, 1)                  # the first of the tied rows wins
    assert field(5, "pivot0", "exit") == (0, 0) and field(5, "zero_pivots")[0] & 1 and field(5, "nonfinite") == (2,)
    assert field(6, "nonfinite")[0] & 1
    assert sc.classify(rec[1]) == {"inverted/2031"} and sc.classify(rec[2]) == {"zero_row/2", "zero_row/negative_zero"}
    assert sc.classify(rec[0]) == {"inverted/0123", "input/rigid"}
    # off again: nothing is recorded, and a full buffer counts without writing
    assert oracle.trace_inverse(lambda: None).shape[0] == 0
    with pytest.raises(ValueError, match="overflow"):
        oracle.trace_inverse(lambda: [oracle.matrix_inverse(m) for m in ms], capacity=3)


def test_traced_equals_untraced(oracle):
    """No result bit depends on the trace: random and degenerate inverses, the crowd, and the committed seam golden."""
    rng = np.random.RandomState(9)
    ms = [rng.normal(size=16).astype(np.float32) for _ in range(200)] + [m.reshape(16) for m in sc.crowd().targets]
    plain = [oracle.matrix_inverse(m) for m in ms]
    traced = []
    oracle.trace_inverse(lambda: traced.extend(oracle.matrix_inverse(m) for m in ms))
    for a, b in zip(plain, traced):
        assert a.tobytes() == b.tobytes()
    z = np.load(PHYSICS_GOLDEN, allow_pickle=False)
    rig, over, strict, _ = physics_case(int(z["nb"]), int(z["seed"]), int(z["n_ik"]), int(z["n_app"]))
    rest, parent, level, flags, ap, ar, ik = rig

    def golden():
        for i in range(z["poses"].shape[0]):
            got, _ = oracle.bone_solve_physics(rest, parent, z["poses"][i], over, strict, z["xf"][i], level, flags, ap, ar, ik)
            gu.assert_bits_equal(got, z["expect"][i], f"palette {i} with a trace active")
    assert oracle.trace_inverse(golden).shape[0] > 0
    cw = sc.crowd()
    rest, parent, level, flags, ap, ar, ik = sc.rig()
    for name in ("L2", "L5"):                               # (oracle_palettes ran under the trace)
        bones, st = sc.over(name)
        for i in range(0, sc.NI, 7):
            a, _ = oracle.bone_solve_physics(rest, parent, cw.poses[i], bones, st, cw.xf[name][i], level, flags, ap, ar, ik)
            assert a.tobytes() == sc.oracle_palettes(oracle, name)[0][i].tobytes(), (name, i)


# ---- CPU: the coverage proof ---------------------------------------------------------------------------------------------------------
def test_every_required_class_occurs(oracle):
    """Each list on its own holds every class of seam_fix_classes.json where it steers (L1, L1z, and L2 / L5 / L6 whose first
    inverse is L1's); each pivot order is held by at least two cases whose whole palette is finite and whose C row differs
    from the solve without overrides."""
    req = sc.required()
    rest, parent, level, flags, ap, ar, ik = sc.rig()
    cw = sc.crowd()
    assert len([c for c in req["required"] if c.startswith("inverted/")]) == 24
    for name, child in (("L1", sc.C), ("L1z", sc.C0)):
        pal, rec = sc.oracle_palettes(oracle, name)
        seen, finite_changed, zlp = {}, {}, set()
        for i in range(sc.NI):
            for c in sc.classify(rec[i, 0]):
                seen[c] = seen.get(c, 0) + 1
                if c.startswith("zero_last_pivot/"):
                    zlp.add(c)
                if c.startswith("inverted/") and np.isfinite(pal[i]).all():
                    plain = oracle.bone_solve_full(rest, parent, cw.poses[i], level, flags, ap, ar, ik)
                    if (gu.bits(plain[child]) != gu.bits(pal[i][child])).any():
                        finite_changed[c] = finite_changed.get(c, 0) + 1
        missing = [c for c in req["required"] if c not in seen]
        assert not missing, (name, missing)
        few = [c for c in req["required"] if c.startswith("inverted/") and finite_changed.get(c, 0) < 2]
        assert not few, (name, "pivot orders with fewer than two finite, changed cases", few)
        assert len(zlp) >= req["min_zero_last_pivot_orders"] >= 4, (name, zlp)
    # the zero exits reach the palette: C0's local matrix is zero, so its row is G * 0
    pal, rec = sc.oracle_palettes(oracle, "L1z")
    for i in range(sc.NI):
        if int(rec[i, 0, T["exit"]]) != 0:
            assert not pal[i][sc.C0][:12].any(), i


def test_zero_exit_reaches_the_post_physics_rows(oracle):
    """Under L1 a zero inverse leaves C's local (rows 0..2) zero, and D -- a post-physics child of C -- inherits it."""
    pal, rec = sc.oracle_palettes(oracle, "L1")
    hit = 0
    for i in range(sc.NI):
        if int(rec[i, 0, T["exit"]]) != 0 and np.isfinite(pal[i]).all():
            assert not pal[i][sc.D][:12].reshape(3, 4)[:, :3].any(), i
            hit += 1
    assert hit >= 8


def test_class_histogram_is_the_pinned_one(oracle):
    assert sc.histogram(oracle) == sc.required()["histogram"]


def test_neighbours_take_different_pivot_orders_and_exits(oracle):
    """Consecutive instances are lanes of one wave: under every list that steers, no two of them share (pivot order, exit, zero
    row), and each 64-lane workgroup holds at least 24 different ones."""
    for name in ("L1", "L1z", "L2", "L5", "L6"):
        rec = sc.oracle_palettes(oracle, name)[1][:, 0]
        key = [tuple(int(x) for x in r[16:21]) for r in rec]
        same = [i for i in range(sc.NI - 1) if key[i] == key[i + 1]]
        assert not same, (name, same)
        assert min(len(set(key[a:a + 64])) for a in (0, 64)) >= 24, name


def test_later_lists_reach_what_they_are_for(oracle):
    """L2: E inverts a matrix made with an inverse (all kinds of exit); L3 / L4: C inverts P's pose local, scaled by the
    non-unit quaternions; L5: the second Fix differs from the first; L6: Q inverts the identity its post-physics parent holds."""
    rec = sc.oracle_palettes(oracle, "L2")[1]
    exits = {int(r[T["exit"]]) for r in rec[:, 1]}
    assert exits == {0, 1, 2} or exits == {0, 1}, exits
    assert len({sc.pivot_order(r) for r in rec[:, 1]} - {None}) >= 12
    for name in ("L3", "L4"):
        r = sc.oracle_palettes(oracle, name)[1][:, 0]
        m = r[:, :16].copy().view(np.float32).reshape(-1, 4, 4)
        norms = np.linalg.norm(m[:, 0, :3].astype(np.float64), axis=1)
        finite = np.isfinite(norms)
        assert (np.abs(norms[finite] - 1) > 0.5).sum() >= 30, name   # 34 quaternions have length 2: no rotation matrix
        assert len({sc.pivot_order(x) for x in r} - {None}) >= 8, name
    pal5, rec5 = sc.oracle_palettes(oracle, "L5")
    pal1 = sc.oracle_palettes(oracle, "L1")[0]
    assert sum(pal5[i][sc.C].tobytes() != pal1[i][sc.C].tobytes() for i in range(sc.NI)) > sc.NI // 2
    rec6 = sc.oracle_palettes(oracle, "L6")[1][:, 1]
    assert all(np.array_equal(r[:16].copy().view(np.float32), np.eye(4, dtype=np.float32).reshape(16)) for r in rec6)


# ---- CPU: against libmmd -------------------------------------------------------------------------------------------------------------
@NEEDS_REF
def test_every_traced_input_through_libmmd_inverse(oracle):
    n = 0
    for name in sc.LISTS:
        for recs in sc.oracle_palettes(oracle, name)[1]:
            for rec in recs:
                m = rec[:16].copy().view(np.float32)
                gu.assert_bits_equal_or_both_nan(oracle.matrix_inverse(m), Reference.matrix_inverse(m), f"{name}: inverse of {m}")
                n += 1
    assert n == sc.NI * sum(len(v) for v in sc.INVERTING.values())


@NEEDS_REF
@pytest.mark.parametrize("name", list(sc.LISTS))
def test_oracle_equals_libmmd_and_the_fixture_is_a_fresh_run(oracle, name):
    want = sc.reference_palettes(name)
    assert_crowd(sc.oracle_palettes(oracle, name)[0], want, f"{name}: oracle vs libmmd")
    z = np.load(sc.EXPECT, allow_pickle=False)
    assert z[name].tobytes() == want.tobytes(), f"{name}: tests/golden/seam_fix_expect.npz is not what libmmd gives now"


def test_fixture_equals_the_oracle(oracle):
    """(Without the reference build too.)  The committed libmmd palettes against the oracle's."""
    z = np.load(sc.EXPECT, allow_pickle=False)
    assert sorted(z.files) == sorted(sc.LISTS)
    for name in sc.LISTS:
        assert z[name].shape == (sc.NI, sc.NB, 16) and z[name].dtype == np.float32
        assert_crowd(sc.oracle_palettes(oracle, name)[0], z[name], f"{name}: oracle vs the libmmd fixture")
    assert os.path.getsize(sc.EXPECT) < 512 * 1024


# ---- GPU -----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def clean_env(monkeypatch, hip_lib):
    for v in ENV:
        monkeypatch.delenv(v, raising=False)
    return monkeypatch


def seam(sk, name, ni=None, rows=None):
    """solve_pre + solve_post of list `name` over the first ni instances (or the given rows) of the crowd."""
    cw = sc.crowd()
    rows = slice(0, ni if ni is not None else sc.NI) if rows is None else rows
    bones, strict = sc.over(name)
    sk.solve_pre(cw.poses[rows])
    return sk.solve_post(bones, strict, cw.xf[name][rows])


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(sc.LISTS))
def test_gpu_every_list_equals_the_oracle_and_libmmd(clean_env, oracle, name):
    """The whole crowd (three workgroups of physics_override_kernel, the last with 8 lanes), then cut to 1, 63, 64, 65 and 130."""
    want = sc.oracle_palettes(oracle, name)[0]
    fixture = np.load(sc.EXPECT, allow_pickle=False)[name]
    sk = vmd.Skeleton(*sc.rig(), physics_seam=True)
    got = seam(sk, name)
    assert_crowd(got, want, f"{name} vs the oracle")
    assert_crowd(got, fixture, f"{name} vs libmmd")
    for ni in sc.CUTS:
        cut = seam(sk, name, ni)
        assert cut.shape[0] == ni
        assert_crowd(cut, want, f"{name}, {ni} instances vs the oracle")
        assert cut.tobytes() == got[:ni].tobytes(), f"{name}, {ni} instances: not the first rows of the whole crowd"
    sk.close()


def post_raw(sk, ni, bones, strict, skinning_ptr, flags, out_ptr, null_struct=False):
    """mmdx_skeleton_solve_post itself: strict may be None (NULL), skinning and out are addresses."""
    b = np.ascontiguousarray(bones, np.int32)
    st = np.ascontiguousarray(strict, np.uint8) if strict is not None else None
    ov = vmd.PhysicsOverrides(C.sizeof(vmd.PhysicsOverrides), b.size, b.ctypes.data if b.size else None,
                              st.ctypes.data if st is not None and st.size else None, skinning_ptr)
    api.check(api.lib().mmdx_skeleton_solve_post(sk.h, None, ni, None if null_struct else C.byref(ov), flags, out_ptr))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["L1z", "L2", "L5"])
def test_gpu_device_resident_operands_give_the_host_bytes(clean_env, oracle, name):
    """MMDX_OVERRIDES_ON_DEVICE | MMDX_OUT_ON_DEVICE: poses, skinning rows and palettes in device buffers; guard words around the
    palettes keep their pattern."""
    cw = sc.crowd()
    bones, strict = sc.over(name)
    sk = vmd.Skeleton(*sc.rig(), physics_seam=True)
    host = seam(sk, name)
    assert_crowd(host, sc.oracle_palettes(oracle, name)[0], f"{name}, host operands")
    pal_bytes, guard = sc.NI * sc.NB * 64, 256
    d_poses, d_xf, d_out = DeviceBuffer.from_numpy(cw.poses), DeviceBuffer.from_numpy(cw.xf[name]), DeviceBuffer(pal_bytes + 2 * guard)
    try:
        d_out.memset(0xA5)
        api.check(api.lib().mmdx_skeleton_solve_pre(sk.h, None, sc.NI, d_poses.ptr, None, vmd.POSES_ON_DEVICE | api.OUT_ON_DEVICE,
                                                    d_out.ptr + guard))
        post_raw(sk, sc.NI, bones, strict, d_xf.ptr, vmd.OVERRIDES_ON_DEVICE | api.OUT_ON_DEVICE, d_out.ptr + guard)
        api.check(api.lib().mmdx_device_synchronize())
        raw = d_out.download((pal_bytes + 2 * guard,), np.uint8)
        assert (raw[:guard] == 0xA5).all() and (raw[-guard:] == 0xA5).all(), "written outside the palettes"
        assert raw[guard:-guard].tobytes() == host.tobytes(), f"{name}: device-resident operands vs host operands"
        # host skinning rows into device palettes, and device skinning rows into host palettes
        api.check(api.lib().mmdx_skeleton_solve_pre(sk.h, None, sc.NI, d_poses.ptr, None, vmd.POSES_ON_DEVICE | api.OUT_ON_DEVICE,
                                                    d_out.ptr + guard))
        post_raw(sk, sc.NI, bones, strict, cw.xf[name].ctypes.data, api.OUT_ON_DEVICE, d_out.ptr + guard)
        api.check(api.lib().mmdx_device_synchronize())
        assert d_out.download((pal_bytes,), np.uint8, guard).tobytes() == host.tobytes(), f"{name}: host rows, device palettes"
        sk.solve_pre(cw.poses)
        post_raw(sk, sc.NI, bones, strict, d_xf.ptr, vmd.OVERRIDES_ON_DEVICE, sk._seam_out.ctypes.data)
        assert sk._seam_out.tobytes() == host.tobytes(), f"{name}: device rows, host palettes"
    finally:
        for b in (d_poses, d_xf, d_out):
            b.free()
        sk.close()


@pytest.mark.gpu
def test_gpu_every_solver_form_gives_the_same_bytes(clean_env, oracle):
    """MMDX_SOLVE_DENSE=1 / =0 (read per call) and a skeleton created under MMDX_SOLVE_SEQUENTIAL=1, every list."""
    sk = vmd.Skeleton(*sc.rig(), physics_seam=True)
    default = {name: seam(sk, name) for name in sc.LISTS}
    for name in sc.LISTS:
        assert_crowd(default[name], sc.oracle_palettes(oracle, name)[0], f"{name}, default")
    for dense in ("1", "0"):
        clean_env.setenv("MMDX_SOLVE_DENSE", dense)
        for name in sc.LISTS:
            got = seam(sk, name)
            assert sk.last_solve_shape()["dense"] == int(dense), (name, dense, sk.last_solve_shape())
            assert got.tobytes() == default[name].tobytes(), f"{name}: MMDX_SOLVE_DENSE={dense} vs the default"
    clean_env.delenv("MMDX_SOLVE_DENSE")
    clean_env.setenv("MMDX_SOLVE_SEQUENTIAL", "1")
    seq = vmd.Skeleton(*sc.rig(), physics_seam=True)
    assert seq.info["n_solve_rounds"] == sc.NB
    for name in sc.LISTS:
        assert seam(seq, name).tobytes() == default[name].tobytes(), f"{name}: MMDX_SOLVE_SEQUENTIAL=1 vs the default"
    seq.close()
    sk.close()


def embedded():
    """The island appended to the 60-bone IK + append rig: (rig, list, strict, first island bone, the big rig's own transforms)."""
    (rest, parent, level, flags, ap, ar, ik), big_over, big_strict, rng = physics_case(60, 2, 3, 4)
    nb = rest.shape[0]
    r, p, lv, fl = sc.rig()[:4]
    ik2 = dict(ik)
    for k, fill in (("target", -1), ("loop", 0), ("angle", 0)):
        ik2[k] = np.concatenate([ik[k], np.full(sc.NB, fill, np.asarray(ik[k]).dtype)])
    ik2["link_off"] = np.concatenate([ik["link_off"], np.full(sc.NB, np.asarray(ik["link_off"])[-1], np.asarray(ik["link_off"]).dtype)])
    rig = (np.concatenate([rest, r]), np.concatenate([parent, np.where(p < 0, -1, p + nb)]).astype(np.int64),
           np.concatenate([level, lv]), np.concatenate([flags, fl]).astype(np.uint16),
           np.concatenate([ap, np.full(sc.NB, -1, np.asarray(ap).dtype)]), np.concatenate([ar, np.zeros(sc.NB, np.float32)]), ik2)
    return rig, nb, big_over, big_strict, rng


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["L2", "L5"])
def test_gpu_island_inside_an_ik_and_append_rig(clean_env, oracle, name):
    """65 instances of the crowd as an island of physics_case(60, 2, 3, 4): the post pass has rounds and ik_coop launches around
    the override; the island's rows are the small rig's bytes, the whole palette is the oracle's."""
    rig, nb, big_over, big_strict, rng = embedded()
    ni = 65
    cw = sc.crowd()
    bones, strict = sc.over(name)
    over = np.concatenate([big_over[:3], bones + nb, big_over[3:]])
    st = np.concatenate([big_strict[:3], strict, big_strict[3:]])
    big_xf = random_transforms(rng, ni, big_over.size)
    xf = np.concatenate([big_xf[:, :3], cw.xf[name][:ni], big_xf[:, 3:]], 1)
    poses = np.concatenate([random_poses(ni, nb, 502), cw.poses[:ni]], 1)
    sk = vmd.Skeleton(*rig, physics_seam=True)
    assert sk.info["n_ik_bones"] == 3 and sk.info["n_solve_rounds"] < nb + sc.NB
    sk.solve_pre(poses)
    got = sk.solve_post(over, st, xf)
    rest, parent, level, flags, ap, ar, ik = rig
    for i in range(ni):
        want, _ = oracle.bone_solve_physics(rest, parent, poses[i], over, st, xf[i], level, flags, ap, ar, ik)
        assert_same(got[i], want, f"{name} embedded: instance {i} ({cw.kinds[i]})")
    small = sc.oracle_palettes(oracle, name)[0]
    assert_crowd(got[:, nb:], small, f"{name} embedded: the island's rows vs the small rig")
    sk.close()


@pytest.mark.gpu
def test_gpu_no_leak_between_frames(clean_env, oracle):
    """Frames that follow one another on ONE skeleton -- different lists, the crowd forwards and backwards, frames whose Fix wrote
    zero, NaN and inf local matrices -- equal the same frames on fresh skeletons and the oracle."""
    back = np.arange(sc.NI)[::-1]
    frames = [("L1", None), ("L3", back), ("L2", None), ("L1z", back), ("L4", None), ("L6", back), ("L5", None), ("L3", None)]
    assert any(not np.isfinite(sc.oracle_palettes(oracle, n)[0]).all() for n, _ in frames[:3])
    one = vmd.Skeleton(*sc.rig(), physics_seam=True)
    for k, (name, rows) in enumerate(frames):
        got = seam(one, name, rows=rows)
        fresh_sk = vmd.Skeleton(*sc.rig(), physics_seam=True)
        fresh = seam(fresh_sk, name, rows=rows)
        fresh_sk.close()
        assert got.tobytes() == fresh.tobytes(), f"frame {k} ({name}): one skeleton vs a fresh one"
        assert_crowd(got, sc.oracle_palettes(oracle, name)[0], f"frame {k} ({name})", rows=range(sc.NI) if rows is None else rows)
    # a plain one-call solve after a frame with non-finite local matrices
    rest, parent, level, flags, ap, ar, ik = sc.rig()
    seam(one, "L1")
    whole = one.solve(sc.crowd().poses)
    for i in range(0, sc.NI, 5):
        assert_same(whole[i], oracle.bone_solve_full(rest, parent, sc.crowd().poses[i], level, flags, ap, ar, ik), f"solve after L1: {i}")
    one.close()


@pytest.mark.gpu
def test_gpu_null_strict_and_empty_struct(clean_env, oracle):
    """strict == NULL is Synchronize-only for every bone; n_bones == 0 with a struct equals overrides == NULL (and the plain solve)."""
    cw = sc.crowd()
    rest, parent, level, flags, ap, ar, ik = sc.rig()
    sk = vmd.Skeleton(*sc.rig(), physics_seam=True)
    bones, _ = sc.over("L2")
    sk.solve_pre(cw.poses)
    post_raw(sk, sc.NI, bones, None, cw.xf["L2"].ctypes.data, 0, sk._seam_out.ctypes.data)
    got = sk._seam_out.copy()
    for i in range(sc.NI):
        want, _ = oracle.bone_solve_physics(rest, parent, cw.poses[i], bones, np.zeros(bones.size, np.uint8), cw.xf["L2"][i],
                                            level, flags, ap, ar, ik)
        assert_same(got[i], want, f"strict == NULL: instance {i}")
        assert got[i][sc.P].tobytes() == cw.xf["L2"][i, 0].tobytes()          # Synchronize alone: the row is the override
    sk.solve_pre(cw.poses)
    zeros = sk.solve_post(bones, np.zeros(bones.size, np.uint8), cw.xf["L2"])
    assert zeros.tobytes() == got.tobytes(), "strict == NULL vs strict all zero"
    whole = sk.solve(cw.poses)
    sk.solve_pre(cw.poses)
    post_raw(sk, sc.NI, np.zeros(0, np.int32), None, None, 0, sk._seam_out.ctypes.data)
    empty = sk._seam_out.copy()
    sk.solve_pre(cw.poses)
    post_raw(sk, sc.NI, np.zeros(0, np.int32), None, None, 0, sk._seam_out.ctypes.data, null_struct=True)
    assert empty.tobytes() == sk._seam_out.tobytes() == whole.tobytes(), "n_bones == 0 vs overrides == NULL vs the one-call solve"
    sk.close()

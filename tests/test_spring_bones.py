"""Spring bones: mmdx_spring_set_* and mmdx_spring_step (include/mmdx.h).

There is no libmmd counterpart (the reference moves such bones with Bullet): as for the animator, the contract is the arithmetic the
header states, held by three statements that must agree bit for bit, with no tolerance anywhere (a NaN only has to be a NaN) --
  * csrc/spring_math.hpp and csrc/spring_table.hpp compiled for the host (tests/spring_math_driver.cpp, a stand-alone program, plain
    and sanitized),
  * the numpy restatement tests/spring_ref.py, written from the header's text,
  * the gfx950 kernel (the same header compiled for the device),
and the physical properties are asserted on the restatement, on the CPU.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from simple_mmd_renderer_amd import _capi as api
from simple_mmd_renderer_amd import vmd
from simple_mmd_renderer_amd.engine import DeviceBuffer, SpringSet, chains_below, device_count
from tests import host_program as hp
from tests import palette_place_ref as pp
from tests import spring_ref as sr
from tests.test_capi_symbols import declared_symbols
from tests.test_palette_sockets import crowd_placements, rig_model, rig_small

ENTRY_POINTS = ("mmdx_spring_set_create", "mmdx_spring_set_destroy", "mmdx_spring_set_get_info", "mmdx_spring_step",
                "mmdx_spring_get_state", "mmdx_spring_set_state")
ROOT = os.path.dirname(sr.HERE)
INVALID, BAD_INDEX = 1, 2
F, U = np.float32, np.uint32
ULP = 2.0 ** -23
GUARD = 256                                          # sentinel bytes in front of and behind the palettes
SENT = 0xEE
DEV = api.PALETTE_ON_DEVICE | api.OUT_ON_DEVICE
PLACE_DEV = DEV | api.PLACE_ON_DEVICE


@pytest.fixture(autouse=True)
def _lib(hip_lib):
    return hip_lib


def _close(*things):
    for t in things:
        for x in (t if isinstance(t, (list, tuple)) else [t]):
            (x.free if hasattr(x, "free") else x.close)()


# ---------------------------------------------------------------------------------------- CPU ----
def test_spring_entry_points_are_declared_exported_and_bound(hip_lib):
    syms = declared_symbols()
    for name in ENTRY_POINTS:
        assert name in syms and hasattr(hip_lib, name) and name in api.SIGNATURES, name
    hdr = open(os.path.join(ROOT, "include", "mmdx.h")).read()
    for text in ("typedef struct mmdx_spring_set_desc {", "typedef struct mmdx_spring_set_info {", "typedef struct mmdx_spring_args {",
                 "#define MMDX_ABI_VERSION 3u", "MMDX_SPRING_RESET = (1u << 16)", "MMDX_SPRING_DT_ON_DEVICE = (1u << 17)",
                 "#define MMDX_SPRING_MAX_JOINTS 32", "#define MMDX_SPRING_MAX_COLLIDERS 16", "float(sqrt(double(",
                 "solve -> place -> springs -> palette bounds -> cull"):
        assert text in hdr, text
    assert hip_lib.mmdx_abi_version() == 3
    desc, info, args, reset, dt_dev, pal_dev, mj, mc = hp.c_values(
        ["sizeof(mmdx_spring_set_desc)", "sizeof(mmdx_spring_set_info)", "sizeof(mmdx_spring_args)", "MMDX_SPRING_RESET",
         "MMDX_SPRING_DT_ON_DEVICE", "MMDX_PALETTE_ON_DEVICE", "MMDX_SPRING_MAX_JOINTS", "MMDX_SPRING_MAX_COLLIDERS"])
    assert C.sizeof(api.SpringSetDesc) == desc == 4 * 4 + 6 * 8 + 3 * 4 + 4
    assert C.sizeof(api.SpringSetInfo) == info == 8 * 4
    assert C.sizeof(api.SpringArgs) == args == 4 * 4 + 3 * 8
    assert (api.SPRING_RESET, api.SPRING_DT_ON_DEVICE, api.PALETTE_ON_DEVICE) == (reset, dt_dev, pal_dev) == (1 << 16, 1 << 17, 1)
    assert (api.SPRING_MAX_JOINTS, api.SPRING_MAX_COLLIDERS, sr.MAX_JOINTS, sr.MAX_COLLIDERS) == (mj, mc, mj, mc) == (32, 16, 32, 16)
    for m in ("from_skeleton", "step", "reset", "state", "set_state", "close"):
        assert callable(getattr(SpringSet, m)), m
    poser = open(os.path.join(ROOT, "simple_mmd_renderer_amd", "host", "mmdx_poser.hpp")).read()
    for text in ("class SpringSet", "mmdx_spring_set_create(", "mmdx_spring_set_destroy(", "mmdx_spring_step("):
        assert text in poser, text
    bench = open(os.path.join(ROOT, "include", "mmdx_bench.h")).read()
    assert "mmdx_spring" not in bench


def _driver_segments(case, want):
    steps = [(dt, r, case["pals"][s]) for s, (dt, r) in enumerate(zip(case["dts"], case["resets"]))]
    planted = sr.plant(case, want[sr.PLANT_AT - 1][1], case["pals"][sr.PLANT_AT])
    return [(None, steps[:sr.PLANT_AT]), (planted, steps[sr.PLANT_AT:])]


def test_case_table_contains_every_branch_the_header_names():
    """From the numpy side alone: what the driver and the kernel are about to be compared on."""
    case = sr.case_table()
    _, count = sr.run_case(case)
    missing = [k for k in sr.CASES if count.get(k, 0) < 1]
    assert not missing, (missing, count)
    assert [n for _, n, _ in case["table"]["chains"]] == [2, 1, 32, 1]
    assert sorted(set(sr.CASE_DTS[k] > 0 for k in range(len(sr.CASE_DTS)))) == [False, True]


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_host_build_of_the_arithmetic_equals_the_numpy_restatement(sanitize):
    case = sr.case_table()
    want, _ = sr.run_case(case)
    tb, got = sr.run_driver(sr.build_driver(sanitize), case["parent"], case["rest"], case["chains"], case["params"], case["colliders"],
                            case["gravity"], case["tails"], _driver_segments(case, want))
    t = case["table"]
    assert tb["bone"].tolist() == t["bone"].tolist() and tb["chains"] == t["chains"]
    sr.assert_same(tb["h"], t["h"], "rest positions")
    sr.assert_same(tb["t"], t["t"], "tails")
    for s, ((gp, gs), (wp, ws)) in enumerate(zip(got, want)):
        sr.assert_same(gp, wp, f"palettes after step {s}")
        sr.assert_same(gs, ws, f"state after step {s}")
    assert np.isnan(want[5][0]).any() and np.isfinite(want[7][1][:, :35]).all()      # the NaN frame, and everybody healed after it
    # the default tails, through the driver: the next joint's rest position, the last joint's h + (h - h of its parent)
    parent, rest, chains = sr.chain_rig((3, 1))
    pal = sr.sway_palettes(2, len(parent), 1)[0]
    tb, got = sr.run_driver(sr.build_driver(sanitize), parent, rest, chains, np.array([1.0, 0.1, 1.0, 0.0], F).repeat(2).reshape(4, 2).T,
                            None, (0.0, -9.8, 0.0), None, [(None, [(1 / 60, False, pal)])])
    t = sr.build_table(parent, rest, chains, [1.0, 0.1, 1.0, 0.0])
    sr.assert_same(tb["t"], t["t"], "default tails")
    assert (tb["t"][0] == rest[chains[0][1]]).all() and (tb["t"][2] == rest[chains[0][2]] + (rest[chains[0][2]] - rest[chains[0][1]])).all()
    wp, ws = sr.step(t, pal, sr.nan_state(2, 4), 1 / 60)
    sr.assert_same(got[0][0], wp, "default tails: palettes")
    sr.assert_same(got[0][1], ws, "default tails: state")


def _geometry(table, pal):
    """Per joint of every instance, from the palettes a step left: (H, la, T of the joint's own new row) in float64 from the
    restatement's binary32 values -- P is the parent's NEW row."""
    out = []
    with np.errstate(all="ignore"):
        for first, n, anchor in table["chains"]:
            for j in range(first, first + n):
                parent_row = pal[:, anchor] if j == first else pal[:, table["bone"][j - 1]]
                hh, t0 = sr.pt(table["h"][j], parent_row), sr.pt(table["t"][j], parent_row)
                out.append((hh.astype(np.float64), sr.length(t0 - hh).astype(np.float64), sr.pt(table["t"][j], pal[:, table["bone"][j]]).astype(np.float64)))
    return out


def test_length_is_kept_and_the_row_carries_the_tail_over_300_steps():
    """A swaying anchor, 8 instances, chains of 8, 2 and 1 joints, a collider in the way of the long one.  Every step, every joint:
    | |c - H| - la | <= 8 * 2^-23 * (la + max|H|)  (four roundings go into the normalise-scale-add, relative to the larger of segment
    and coordinate), and pt(t, new row) is within 4 * 2^-23 * max|c| of c."""
    parent, rest, chains = sr.chain_rig((8, 2, 1))
    ni, n_steps = 8, 300
    t0 = sr.build_table(parent, rest, chains, np.zeros(4, F))
    colliders = (np.array([0], U), np.array([[*t0["h"][4], 0.5]], F))
    table = sr.build_table(parent, rest, chains, [[12.0, 0.3, 1.0, 0.05], [0.0, 0.1, 1.0, 0.0], [40.0, 0.6, 0.3, 0.0]], (0.0, -9.8, 0.0), colliders)
    pals = sr.sway_palettes(ni, len(parent), n_steps)
    state, count = sr.nan_state(ni, 11), {}
    worst_len = worst_tail = 0.0
    for s in range(n_steps):
        pal, state = sr.step(table, pals[s], state, 1 / 60, count=count)
        for j, (hh, la, carried) in enumerate(_geometry(table, pal)):
            c = state[:, j, :3].astype(np.float64)
            err = np.abs(np.linalg.norm(c - hh, axis=1) - la)
            bound = 8 * ULP * (la + np.abs(hh).max(axis=1))
            assert (err <= bound).all(), (s, j, err.max(), bound.min())
            worst_len = max(worst_len, float((err / bound).max()))
            terr = np.abs(carried - c).max(axis=1)
            tb = 4 * ULP * np.abs(c).max(axis=1)
            assert (terr <= tb).all(), (s, j, terr.max(), tb.min())
            worst_tail = max(worst_tail, float((terr / tb).max()))
    print("worst length error / bound %.3f, worst tail error / bound %.3f" % (worst_len, worst_tail))
    assert count["collider_hit"] > 0 and count["rotated"] > 300 * 8 * 10 and np.isfinite(state).all()


def test_reset_and_rest_are_rigid_every_bit():
    """Zero gravity: a reset step returns the anchor's row for every joint, every bit, and the steps after it (dt > 0, the anchor
    standing still) keep doing so; on the identity palette every joint row is the identity."""
    parent, rest, chains = sr.chain_rig((32, 2, 1))
    nb, ni = len(parent), 6
    table = sr.build_table(parent, rest, chains, [[12.0, 0.3, 1.0, 0.05], [0.0, 0.1, 1.0, 0.0], [40.0, 0.6, 0.3, 0.0]], (0.0, 0.0, 0.0))
    pal_in = sr.sway_palettes(ni, nb, 3)[2]
    pal_in[1] = sr.rigid_rows(np.random.RandomState(1), nb, scale=np.full(nb, 1.7))          # unrelated, scaled rows
    ident = np.tile(np.eye(4, dtype=F).reshape(16), (ni, nb, 1))
    for what, src in (("swaying", pal_in), ("identity", ident)):
        state = np.random.RandomState(2).normal(size=(ni, 35, 6)).astype(F)
        for s in range(4):
            count = {}
            pal, state = sr.step(table, src, state, 1 / 60, reset=(s == 0), count=count)
            assert count["rigid"] == ni * 35 and count.get("rotated", 0) == 0, (what, s, count)
            for first, n, anchor in table["chains"]:
                for j in range(first, first + n):
                    assert pal[:, table["bone"][j]].tobytes() == src[:, anchor].tobytes(), (what, s, j)
        if what == "identity":
            assert pal.tobytes() == ident.tobytes()


def _hanging(start, n_steps):
    """One joint of length 1 below a fixed head at the origin (identity palette), stiffness 0, drag 0.1, gravity (0, -9.8, 0), dt 1/60;
    the tail's rest direction is `start`.  -> the angle to gravity in degrees after every step, and the tail positions."""
    parent, rest = np.array([-1, 0], np.int32), np.array([[0, 0, 0], [0, 0, 0]], F)
    table = sr.build_table(parent, rest, [[1]], [0.0, 0.1, 1.0, 0.0], (0.0, -9.8, 0.0), tails=np.array([start], F))
    pal = np.tile(np.eye(4, dtype=F).reshape(16), (1, 2, 1))
    state, angles, tails = sr.nan_state(1, 1), [], []
    for _ in range(n_steps):
        _, state = sr.step(table, pal, state, 1 / 60)
        c = state[0, 0, :3].astype(np.float64)
        angles.append(np.degrees(np.arccos(np.clip(-c[1] / np.linalg.norm(c), -1, 1))))
        tails.append(c)
    return np.array(angles), np.array(tails)


def test_a_hanging_tail_stays_and_a_horizontal_one_falls():
    """stiffness 0, drag 0.1.  A tail that starts at H + la * g^ stays within the length bound of it for 300 steps.  From a
    horizontal start (90 degrees) the angle to gravity after N = 100 steps is below the start angle and below 1.8e-3 degrees: a CPU
    run of the restatement gave 80.72 degrees after 1 step, 1.78e-4 after 100 and 0.0 (exactly along gravity) after 200 and 300; the
    bound is the value seen at N with a 10x margin.  The GPU needs no tolerance of its own: it is held to the restatement bitwise."""
    angles, tails = _hanging((0.0, -1.0, 0.0), 300)
    assert (np.abs(tails - np.array([0.0, -1.0, 0.0])).max(axis=1) <= 8 * ULP * (1.0 + 0.0)).all(), np.abs(tails - [0, -1, 0]).max()
    angles, _ = _hanging((1.0, 0.0, 0.0), 300)
    print("angle to gravity after 1, 100, 200, 300 steps:", angles[0], angles[99], angles[199], angles[299])
    assert angles[0] < 90.0 and angles[99] < angles[0] and angles[99] < 1.8e-3 and angles[99:].max() < 1.8e-3


def test_spring_set_create_refuses_what_the_header_lists_without_a_device(hip_lib):
    parent, rest, chains = sr.chain_rig((3, 2, 1))          # bones: 0 root, 1-2 its children, 3-5, 6-7, 8 the chains
    sk = vmd.Skeleton(rest, parent)
    err = lambda: (hip_lib.mmdx_last_error_string() or b"").decode()          # noqa: E731
    out = C.c_void_p()
    keep = []

    def create(chains=chains, params=None, colliders=None, gravity=(0, -9.8, 0), tails=None, max_instances=4, struct_size=None, reserved0=0,
               skeleton=sk.h, n_colliders=None, null=()):
        off = np.zeros(len(chains) + 1, U)
        off[1:] = np.cumsum([len(c) for c in chains])
        bones = np.array([b for c in chains for b in c], U)
        prm = np.array(params if params is not None else [[1.0, 0.1, 1.0, 0.0]] * len(chains), F)
        d = api.SpringSetDesc(C.sizeof(api.SpringSetDesc) if struct_size is None else struct_size, len(chains), 0, max_instances)
        d.chain_offset, d.joint_bone, d.chain_params = off.ctypes.data, bones.ctypes.data if bones.size else None, prm.ctypes.data
        keep.extend([off, bones, prm])
        if tails is not None:
            t = np.array(tails, F)
            d.joint_tail = t.ctypes.data
            keep.append(t)
        if colliders is not None:
            cb, cs = np.array(colliders[0], U), np.array(colliders[1], F)
            d.n_colliders, d.collider_bone, d.collider_sphere = cb.size, cb.ctypes.data, cs.ctypes.data
            keep.extend([cb, cs])
        if n_colliders is not None:
            d.n_colliders = n_colliders
        d.gravity[:] = gravity
        d.reserved0 = reserved0
        for name in null:
            setattr(d, name, None)
        return hip_lib.mmdx_spring_set_create(skeleton, C.byref(d), C.byref(out))
    sphere = [0.0, 0.0, 0.0, 0.5]
    assert create(skeleton=None) == INVALID and "NULL" in err()
    assert hip_lib.mmdx_spring_set_create(sk.h, None, C.byref(out)) == INVALID and "NULL" in err()
    assert create(struct_size=C.sizeof(api.SpringSetDesc) - 4) == INVALID and "struct_size" in err()
    assert create(reserved0=1) == INVALID and "reserved0" in err()
    assert create(chains=[[3, 4, 40]]) == BAD_INDEX and "joint_bone[2] = 40" in err()
    assert create(colliders=([9], [sphere])) == BAD_INDEX and "collider_bone[0] = 9" in err()
    assert create(chains=[[3, 5]]) == INVALID and "is not the joint before it" in err()            # 5's parent is 4
    assert create(chains=[[4, 3]]) == INVALID and "anchor of chain 0, bone 3, is a joint" in err()      # upside down
    assert create(chains=[[0]]) == INVALID and "has no parent" in err()
    assert create(chains=[[3], [4, 5]]) == INVALID and "anchor of chain 1, bone 3, is a joint" in err()
    assert create(colliders=([0, 4], [sphere, sphere])) == INVALID and "collider_bone[1] = 4 is a joint" in err()
    assert create(chains=[[3, 4], [6], [6, 7]]) == INVALID and "listed twice" in err()
    assert create(chains=[[3], []]) == INVALID and "chain 1 has 0 joints" in err()
    assert create(chains=[]) == INVALID and "n_chains == 0" in err()
    long_parent, long_rest, long_chains = sr.chain_rig((33,))
    long_sk = vmd.Skeleton(long_rest, long_parent)
    assert create(chains=long_chains, skeleton=long_sk.h) == INVALID and "chain 0 has 33 joints" in err()
    assert create(chains=[long_chains[0][:32]], skeleton=long_sk.h) == api.OK
    hip_lib.mmdx_spring_set_destroy(out)
    assert create(colliders=([0] * 17, [sphere] * 17)) == INVALID and "n_colliders = 17" in err()
    assert create(colliders=([0] * 16, [sphere] * 16)) == api.OK
    hip_lib.mmdx_spring_set_destroy(out)
    nan = float("nan")
    for k in range(4):
        prm = [[1.0, 0.1, 1.0, 0.0] for _ in chains]
        prm[1][k] = nan
        assert create(params=prm) == INVALID and "chain_params[1]" in err(), k
    assert create(gravity=(0, nan, 0)) == INVALID and "gravity" in err()
    assert create(colliders=([0], [[0.0, nan, 0.0, 1.0]])) == INVALID and "collider_sphere[0]" in err()
    bad_tails = np.zeros((6, 3), F)
    bad_tails[4, 1] = nan
    assert create(tails=bad_tails) == INVALID and "joint_tail[4]" in err()
    for drag in (-0.001, 1.001, float("inf")):
        assert create(params=[[1.0, drag, 1.0, 0.0]] * 3) == INVALID and "drag is outside [0, 1]" in err(), drag
    assert create(max_instances=0) == INVALID and "max_instances" in err()
    assert create(null=("chain_params",)) == INVALID and "NULL" in err()
    assert create(colliders=([0], [sphere]), null=("collider_sphere",)) == INVALID and "NULL" in err()
    assert out.value is None                                               # a refusal hands out nothing
    # what is allowed: drag 0 and 1, an infinite stiffness, a negative radius, no colliders; and the set reports itself
    for drag in (0.0, 1.0):
        s = SpringSet(sk, chains, [float("inf"), drag, -1.0, -0.5], 7, colliders=([0, 1], [sphere, sphere]))
        assert s.info() == dict(n_chains=3, n_joints=6, n_colliders=2, max_instances=7, n_bones=9, device_ordinal=-1)
        s.close()
    s = SpringSet.from_skeleton(sk, [3, 6, 8], [1.0, 0.1, 1.0, 0.0], 2)
    assert s.info()["n_joints"] == 6 and chains_below(sk, [3, 6, 8]) == chains and chains_below(sk, [0]) == [[0]]
    info = api.SpringSetInfo(8)
    assert hip_lib.mmdx_spring_set_get_info(s.h, C.byref(info)) == INVALID and "struct_size" in err()
    hip_lib.mmdx_spring_set_destroy(None)                                  # like free(NULL)
    sk.close()                                                             # the set copied what it needs
    assert s.info()["n_bones"] == 9
    _close(s, long_sk)


def test_spring_step_refuses_bad_arguments_before_any_device_call(hip_lib):
    """Every call here carries its defect AND n_instances above the set's max_instances or another host-side refusal behind it, so
    none of them can reach a device."""
    parent, rest, chains = sr.chain_rig((3, 2, 1))
    sk = vmd.Skeleton(rest, parent)
    s = SpringSet(sk, chains, [1.0, 0.1, 1.0, 0.0], 4)
    err = lambda: (hip_lib.mmdx_last_error_string() or b"").decode()          # noqa: E731
    dt = C.c_float(1 / 60)
    P = 0x10000                                                            # stands for a device address; never dereferenced
    ids = np.array([0, 9], U)

    def call(set_h=s.h, struct_size=None, flags=api.PALETTE_ON_DEVICE, ni=4, reserved0=0, palettes=P, dt_ptr=C.addressof(dt), select=None,
             null_args=False):
        a = api.SpringArgs(C.sizeof(api.SpringArgs) if struct_size is None else struct_size, flags, ni, reserved0, palettes, dt_ptr)
        if select is not None:
            a.select = C.pointer(select)
        return hip_lib.mmdx_spring_step(set_h, None, None if null_args else C.byref(a))
    host_bad = vmd.instance_select(ids.ctypes.data, 2, None, on_device=False)          # id 9 >= 4: the refusal behind the others
    assert call(select=host_bad) == INVALID and "ids[1] = 9 is not below n_instances" in err()          # the guard itself
    assert call(set_h=None) == INVALID and "NULL" in err()
    assert call(null_args=True) == INVALID and "NULL" in err()
    assert call(struct_size=C.sizeof(api.SpringArgs) - 8, select=host_bad) == INVALID and "struct_size" in err()
    for bad in (2, 4, 1 << 10, 1 << 15, 1 << 18, 1 << 31):
        assert call(flags=api.PALETTE_ON_DEVICE | bad, select=host_bad) == INVALID and "unknown flag bits" in err(), bad
    assert call(flags=api.SPRING_RESET, select=host_bad) == INVALID and "MMDX_PALETTE_ON_DEVICE" in err()
    assert call(flags=api.PALETTE_ON_DEVICE | api.SPRING_RESET | api.SPRING_DT_ON_DEVICE, dt_ptr=P, select=host_bad) == INVALID and "ids[1]" in err()
    assert call(reserved0=1, select=host_bad) == INVALID and "reserved0" in err()
    assert call(ni=5) == INVALID and "n_instances = 5 is above the set's max_instances = 4" in err()
    assert call(palettes=None, select=host_bad) == INVALID and "palettes / dt is NULL" in err()
    assert call(dt_ptr=None, select=host_bad) == INVALID and "palettes / dt is NULL" in err()
    assert call(palettes=P + 4, select=host_bad) == INVALID and "16-byte" in err()
    assert call(flags=api.PALETTE_ON_DEVICE | api.SPRING_DT_ON_DEVICE, dt_ptr=P + 2, select=host_bad) == INVALID and "4-byte" in err()
    sel = vmd.instance_select(P + 2, 2)
    assert call(select=sel) == INVALID and "4-byte aligned" in err()
    sel = vmd.instance_select(ids.ctypes.data, 2, None, on_device=False)
    sel.reserved0 = 1
    assert call(select=sel) == INVALID and "reserved0" in err()
    assert call(ni=0, palettes=None, dt_ptr=None) == api.OK                # nothing to do, nothing looked at
    state = np.zeros((5, 6, 6), F)
    assert hip_lib.mmdx_spring_get_state(s.h, None, 5, state.ctypes.data) == INVALID and "max_instances" in err()
    assert hip_lib.mmdx_spring_set_state(s.h, None, 5, state.ctypes.data) == INVALID and "max_instances" in err()
    assert hip_lib.mmdx_spring_get_state(s.h, None, 2, None) == INVALID and "NULL" in err()
    with pytest.raises(ValueError):
        s.step(P)
    with pytest.raises(ValueError):
        s.step(P, dt=0.1, dt_ptr=P)
    _close(s, sk)


def test_kernel_resources_no_spills_no_scratch_no_lds():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), api.LIB_PATH, "spring"],
                         capture_output=True, text=True, check=True).stdout.splitlines()
    names = {l.split(" vgpr ")[0].strip() for l in out}
    assert names == {"spring_step_kernel<true>", "spring_step_kernel<false>"}
    for l in out:
        f = l.split(" vgpr ")[1].split()
        res = dict(zip(["vgpr"] + f[1::2], (int(v) for v in f[0::2])))
        assert res["spill"] == 0 and res["scratch"] == 0 and res["lds"] == 0 and res["vgpr"] <= 128, l


# ---------------------------------------------------------------------------------------- GPU ----
@pytest.fixture
def gpu(hip_lib):
    assert device_count() >= 1, "no HIP device visible: the GPU tests must run on the MI355X box"
    return hip_lib


class Guarded:
    """Device palettes [ni][nb][16] with GUARD sentinel bytes on both sides.  The copies are synchronous copies of the null stream,
    which a model's own stream does not wait for and is not waited for by: upload and read synchronise the model's stream first, so
    no copy overtakes a step that is still running."""

    def __init__(self, ni, nb, dm):
        self.shape = (ni, nb, 16)
        self.nbytes = ni * nb * 64
        self.dm = dm
        self.buf = DeviceBuffer(self.nbytes + 2 * GUARD)
        self.ptr = self.buf.ptr + GUARD
        self.buf.memset(SENT)

    def upload(self, pal):
        self.dm.sync()
        self.buf.upload(np.ascontiguousarray(pal, F), GUARD)

    def read(self, what):
        self.dm.sync()
        raw = self.buf.download((self.nbytes + 2 * GUARD,), np.uint8)
        assert (raw[:GUARD] == SENT).all() and (raw[GUARD + self.nbytes:] == SENT).all(), what + ": a guard byte changed"
        return raw[GUARD:GUARD + self.nbytes].view(F).reshape(self.shape)

    def free(self):
        self.buf.free()


N_STEPS, CHECK_AT, NI_MAX = 25, (1, 2, 25), 257
_rigs = {}


def _long_rig_poses(ni, nb, step):
    """Local poses of the 40-bone rig for one step of a moving clip: every bone turns a little, the root and the anchors a lot."""
    rng = np.random.RandomState(900 + step)
    poses = np.zeros((ni, nb, 8), F)
    ang = 0.5 * np.sin(0.3 * step + np.arange(ni)[:, None] * 0.37 + np.arange(nb)[None, :] * 0.11)
    axis = rng.normal(size=(nb, 3))
    axis /= np.linalg.norm(axis, axis=1, keepdims=True)
    poses[:, :, 4:7] = np.sin(ang / 2)[:, :, None] * axis[None]
    poses[:, :, 7] = np.cos(ang / 2)
    poses[:, 0, 0:3] = 0.3 * np.sin(0.2 * step + np.arange(ni)[:, None] + np.arange(3)[None, :])
    return poses


def rig(name):
    """(skeleton arrays, chains, params, colliders, model-space palettes [N_STEPS, 257, NB, 16], placed palettes, restatement results
    per space: {step: (pal, state)}), computed once per rig and shared, never modified.  The palettes come from mmdx_skeleton_solve of
    a moving clip (rig_small's own frames, a lap later for every 75 instances; synthetic poses for the 40-bone rig)."""
    if name in _rigs:
        return _rigs[name]
    if name == "long":                                                       # 40 bones: chains of 32, 2 and 1 joints, 16 colliders
        parent, rest, chains = sr.chain_rig((32, 2, 1), extra=4)
        sk = vmd.Skeleton(rest, parent)
        params = [[12.0, 0.3, 1.0, 0.05], [0.0, 0.1, 1.0, 0.0], [40.0, 0.6, 0.3, 0.02]]
        rng = np.random.RandomState(16)
        colliders = (np.arange(16) % 5, np.concatenate([rest[5:37:2] + rng.uniform(-0.3, 0.3, (16, 3)), rng.uniform(0.1, 0.5, (16, 1))], axis=1))
        colliders[1][0] = [*rest[6], 0.3]                                        # on the long chain's anchor, centred on its first rest tail
        poses = lambda s: _long_rig_poses(NI_MAX, len(parent), s)          # noqa: E731
    else:
        z = rig_small()
        parent, rest = z["parent"], z["rest"].astype(F)
        sk = vmd.Skeleton(rest, parent, z["level"], z["flags"])
        lap = (np.arange(NI_MAX) // 75 * 0.125).astype(F)[:, None]

        def poses(s):
            p = z["expect_poses"][(np.arange(NI_MAX) + 3 * s) % 75].copy()
            p[:, :, 0] += lap
            return p
        if name == "small1":                                                 # one chain of one joint, no collider
            chains, params, colliders = [[20]], [[20.0, 0.2, 1.0, 0.0]], None
        else:                                                                # "small3": chains of 2, 1 and 1 joints, one collider
            chains, params = [[18, 10], [13], [19]], [[20.0, 0.2, 1.0, 0.1], [0.0, 0.1, 1.0, 0.0], [60.0, 0.5, 0.2, 0.0]]
            colliders = ([16], [[*rest[10], 0.3]])      # on the first chain's anchor, centred on its first joint's rest tail: the tail
            #                                             starts AT the centre and is pushed out as soon as it moves
    with rig_model() as dm:
        model_space = np.stack([sk.solve(poses(s), dm) for s in range(N_STEPS)])
    sk.close()
    assert np.isfinite(model_space).all() and model_space[0].tobytes() != model_space[1].tobytes()
    placed = np.stack([pp.place_crowd(model_space[s], crowd_placements(NI_MAX), False) for s in range(N_STEPS)])
    table = sr.build_table(parent, rest, chains, params, (0.0, -9.8, 0.0), colliders)
    nj = len(table["bone"])
    want = {}
    for space, pals in (("model space", model_space), ("placed", placed)):
        state, count, res = sr.nan_state(NI_MAX, nj), {}, {}
        for s in range(N_STEPS):
            pal, state = sr.step(table, pals[s], state, 1 / 60, count=count)
            if s + 1 in CHECK_AT:
                res[s + 1] = (pal, state)
        assert count["rotated"] > 0 and (colliders is None or count["collider_hit"] > 0), (name, space, count)
        want[space] = res
    _rigs[name] = dict(parent=parent, rest=rest, chains=chains, params=params, colliders=colliders, table=table, nb=len(parent), nj=nj,
                       pals={"model space": model_space, "placed": placed}, want=want)
    return _rigs[name]


def _skeleton_and_set(r, max_instances):
    if r["nb"] == 24:
        z = rig_small()
        sk = vmd.Skeleton(r["rest"], r["parent"], z["level"], z["flags"])
    else:
        sk = vmd.Skeleton(r["rest"], r["parent"])
    return sk, SpringSet(sk, r["chains"], r["params"], max_instances, colliders=r["colliders"])


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["small1", "small3", "long"])
@pytest.mark.parametrize("ni", [1, 63, 64, 65, 257])
def test_gpu_rows_and_state_equal_the_restatement(gpu, ni, name):
    """25 steps from solved palettes of a moving clip, model space and placed; after 1, 2 and 25 steps the whole palette array (joint
    rows rewritten, every other row and the guard bytes untouched) and the state equal the restatement's, byte for byte.  A partial
    wave, a whole one, one lane more, five workgroups per chain; host dt on even steps, device dt on odd ones."""
    r = rig(name)
    nb, nj = r["nb"], r["nj"]
    joint = np.zeros(nb, bool)
    joint[r["table"]["bone"]] = True
    with rig_model() as dm:
        sk, sset = _skeleton_and_set(r, ni + 3)
        d_pal, d_dt = Guarded(ni, nb, dm), DeviceBuffer.from_numpy(np.array([1 / 60], F))
        for space in ("model space", "placed"):
            sset.reset(0x10000, n_instances=0)                                # nothing to do
            if space == "placed":
                sset.set_state(sr.nan_state(ni + 3, nj), dm)                  # a fresh start: NaN state is a reset
            for s in range(N_STEPS):
                src = r["pals"][space][s][:ni]
                d_pal.upload(src)
                if s % 2:
                    sset.step(d_pal, dt_ptr=d_dt.ptr, n_instances=ni, model=dm)
                else:
                    sset.step(d_pal, dt=1 / 60, n_instances=ni, model=dm)
                if s + 1 in CHECK_AT:
                    what = f"{name}, NI {ni}, {space}, after {s + 1} steps"
                    dm.sync()
                    got = d_pal.read(what)
                    wp, ws = r["want"][space][s + 1]
                    sr.assert_same(got, wp[:ni], what + ": palettes")
                    assert got[:, ~joint].tobytes() == src[:, ~joint].tobytes(), what + ": a row that is no joint changed"
                    state = sset.state(ni + 3, dm)
                    sr.assert_same(state[:ni], ws[:ni], what + ": state")
                    assert np.isnan(state[ni:]).all(), what + ": the state of an instance beyond n_instances was written"
        assert sset.info()["device_ordinal"] >= 0
        _close(d_pal, d_dt, sset, sk)


SEL_IDS = np.array([3, 64, 0, 7, 33, 1, 12, 40], U)
SEL_IDS_DEV = np.array([3, 64, 0, 70, 7, 0xFFFFFFFF, 12, 40], U)              # 70 and 2^32-1 are no instances of 65


@pytest.mark.gpu
@pytest.mark.parametrize("where", ["host list", "device list"])
def test_gpu_select_steps_the_listed_instances_only(gpu, where):
    """65 instances of the 3-chain set on placed palettes.  Everybody is stepped twice; then lists with count NULL, 0, 5 and 100:
    listed instances get the restatement's rows and state, unlisted palette rows and state keep every byte; then a reset through a
    list, and a step of the rest."""
    ni = 65
    r = rig("small3")
    nb, nj, table = r["nb"], r["nj"], r["table"]
    pals = r["pals"]["placed"][:, :ni]
    with rig_model() as dm:
        sk, sset = _skeleton_and_set(r, ni)
        d_pal = Guarded(ni, nb, dm)
        state = sr.nan_state(ni, nj)
        for s in range(2):
            d_pal.upload(pals[s])
            sset.step(d_pal, dt=1 / 60, n_instances=ni, model=dm)
            _, state = sr.step(table, pals[s], state, 1 / 60)
        ids = SEL_IDS if where == "host list" else SEL_IDS_DEV
        d_ids, d_cnt = DeviceBuffer.from_numpy(ids), DeviceBuffer(4)
        plans = [(c, False) for c in (None, 0, 5, 100)] + [(None, True)]
        for k, (count, reset) in enumerate(plans):
            what = f"{where}, count {count}, reset {reset}"
            if where == "host list":
                cnt = C.c_uint32(count or 0)
                sel = vmd.instance_select(ids.ctypes.data, ids.size, C.addressof(cnt) if count is not None else None, on_device=False)
            else:
                d_cnt.upload(np.array([count or 0], U))
                sel = vmd.instance_select(d_ids.ptr, ids.size, d_cnt.ptr if count is not None else None)
            src = pals[2 + k]
            d_pal.upload(src)
            sset.step(d_pal, dt=1 / 60, n_instances=ni, select=sel, model=dm, reset=reset)
            dm.sync()
            used = [int(i) for i in (ids if count is None else ids[:min(count, ids.size)]) if i < ni]
            wp, state_new = sr.step(table, src, state, 1 / 60, reset, ids=used)
            unlisted = np.ones(ni, bool)
            unlisted[used] = False
            assert wp[unlisted].tobytes() == src[unlisted].tobytes() and state_new[unlisted].tobytes() == state[unlisted].tobytes()
            sr.assert_same(d_pal.read(what), wp, what + ": palettes")
            sr.assert_same(sset.state(ni, dm), state_new, what + ": state")
            state = state_new
        # the listed instances were reset; now the rest of the crowd steps
        rest_ids = np.array([i for i in range(ni) if i not in used], U)
        d_rest = DeviceBuffer.from_numpy(rest_ids)
        src = pals[8]
        d_pal.upload(src)
        sset.step(d_pal, dt=1 / 60, n_instances=ni, select=vmd.instance_select(d_rest.ptr, rest_ids.size), model=dm)
        wp, state_new = sr.step(table, src, state, 1 / 60, ids=rest_ids)
        sr.assert_same(d_pal.read("the rest"), wp, "the rest: palettes")
        sr.assert_same(sset.state(ni, dm), state_new, "the rest: state")
        # a list of capacity 0, and a host id that is no instance
        d_pal.upload(src)
        sset.step(d_pal, dt=1 / 60, n_instances=ni, select=vmd.instance_select(d_ids.ptr, 0), model=dm)
        assert d_pal.read("n_ids 0").tobytes() == src.tobytes()
        bad = np.array([1, 65], U)
        with pytest.raises(api.MmdxError, match="is not below n_instances"):
            sset.step(d_pal, dt=1 / 60, n_instances=ni, select=vmd.instance_select(bad.ctypes.data, 2, None, on_device=False), model=dm)
        sr.assert_same(sset.state(ni, dm), state_new, "after the refusals: state")
        _close(d_pal, d_ids, d_cnt, d_rest, sset, sk)


@pytest.mark.gpu
def test_gpu_recorded_frame_replayed_40_times_on_a_borrowed_stream(gpu):
    """[mmdx_skeleton_solve_motion_set_blend_time, mmdx_palette_place, mmdx_spring_step, mmdx_palette_bounds] recorded once on a
    stream of the test's that the model borrows, replayed 40 times with the clip times and dt rewritten in device memory: after every
    replay the palettes equal the restatement's step on the palettes solve and place give for those times, the state equals 40
    restatement steps, and the boxes are finite.  A host dt and a host list are refused while recording."""
    from tests import hip_stream_util as hs
    from tests import motion_blend_ref as mb
    from tests import palette_bounds_ref as pb
    hs.hip()
    ni, n_replays = 65, 40
    r = rig("small3")
    nb, nj, table = r["nb"], r["nj"], r["table"]
    z = rig_small()
    names = [str(n) for n in mb.fixture()["bone_names"]]
    vs = [vmd.Vmd(p) for p in mb.BONE_VMDS]
    bms = [v.bind_bones(names) for v in vs]
    ms = vmd.MotionSet(bms)
    rng = np.random.RandomState(40)
    ca, cb = (np.arange(ni) % 2).astype(U), ((np.arange(ni) + 1) % 2).astype(U)
    w = rng.uniform(0, 1, ni).astype(F)
    t0 = rng.uniform(0, 1.5, ni)
    dts = rng.uniform(1 / 144, 1 / 30, n_replays).astype(F)
    dts[11] = 0.0
    with rig_model() as dm, hs.Stream() as S:
        sk, sset = _skeleton_and_set(r, ni)
        d_ca, d_cb, d_w = DeviceBuffer.from_numpy(ca), DeviceBuffer.from_numpy(cb), DeviceBuffer.from_numpy(w)
        d_ta, d_tb, d_dt = DeviceBuffer(ni * 8), DeviceBuffer(ni * 8), DeviceBuffer(4)
        d_place, d_pal, d_bnd = DeviceBuffer.from_numpy(crowd_placements(ni)), Guarded(ni, nb, dm), DeviceBuffer(ni * 24)
        d_ids = DeviceBuffer.from_numpy(np.arange(ni, dtype=U))

        def solve_place():
            sk.solve_motion_set_blend_time_device(ms, ni, d_ca.ptr, d_ta.ptr, d_cb.ptr, d_tb.ptr, d_w.ptr, d_pal.ptr, dm)
            dm.place_palettes(ni, d_pal.ptr, d_place.ptr, d_pal.ptr, PLACE_DEV)

        def frame():
            solve_place()
            sset.step(d_pal, dt_ptr=d_dt.ptr, n_instances=ni, select=vmd.instance_select(d_ids.ptr, ni), model=dm)
            dm.palette_bounds_raw(ni, d_pal.ptr, d_bnd.ptr, DEV, 1.0, 1.0)
        try:
            dm.set_stream(S.ptr)
            times = [(t0 + 0.04 * k, t0 * 0.5 + 0.03 * k) for k in range(n_replays)]
            solved = []
            for ta, tb in times:                                              # what solve and place give, un-recorded
                d_ta.upload(np.ascontiguousarray(ta, np.float64))
                d_tb.upload(np.ascontiguousarray(tb, np.float64))
                solve_place()
                S.synchronize()
                solved.append(d_pal.read("solve and place"))
            assert solved[0].tobytes() != solved[1].tobytes() and np.isfinite(solved).all()
            d_dt.upload(np.array([0.0], F))
            frame()                                                           # the run before recording: the set goes to the device
            S.synchronize()
            sset.set_state(sr.nan_state(ni, nj), dm)
            d_pal.buf.memset(SENT)
            dm.graph_begin()
            try:
                assert S.capture_status() == hs.CAPTURE_ACTIVE
                frame()
                with pytest.raises(api.MmdxError, match="dt must be in device memory"):
                    sset.step(d_pal, dt=1 / 60, n_instances=ni, model=dm)
                host_ids = np.arange(3, dtype=U)
                with pytest.raises(api.MmdxError, match="instance list must be in device memory"):
                    sset.step(d_pal, dt_ptr=d_dt.ptr, n_instances=ni, model=dm,
                              select=vmd.instance_select(host_ids.ctypes.data, 3, None, on_device=False))
                with pytest.raises(api.MmdxError, match="while a graph is being recorded"):
                    sset.state(ni, dm)
                assert S.capture_status() == hs.CAPTURE_ACTIVE
            finally:
                graph = dm.graph_end()
            try:
                S.synchronize()
                assert (d_pal.buf.download((d_pal.nbytes + 2 * GUARD,), np.uint8) == SENT).all(), "recording ran something"
                assert np.isnan(sset.state(ni, dm)).all()
                state = sr.nan_state(ni, nj)
                for k, (ta, tb) in enumerate(times):
                    d_ta.upload(np.ascontiguousarray(ta, np.float64))
                    d_tb.upload(np.ascontiguousarray(tb, np.float64))
                    d_dt.upload(dts[k:k + 1])
                    graph.launch()
                    S.synchronize()
                    wp, state = sr.step(table, solved[k], state, dts[k])
                    sr.assert_same(d_pal.read(f"replay {k}"), wp, f"replay {k}: palettes")
                    if k in (0, 11, 39):
                        sr.assert_same(sset.state(ni, dm), state, f"replay {k}: state")
                        boxes = d_bnd.download((ni, 6), F)
                        sr.assert_same(boxes, pb.palette_bounds(dm.bone_boxes(), wp, 1.0, 1.0), f"replay {k}: boxes of the rewritten rows")
                sset.close()                                                  # took part in the recording
                with pytest.raises(api.MmdxError, match="destroyed"):
                    graph.launch()
            finally:
                graph.close()
        finally:
            dm.set_stream(None)
        _close(d_ca, d_cb, d_w, d_ta, d_tb, d_dt, d_place, d_pal, d_bnd, d_ids, sk, ms, bms, vs)


@pytest.mark.gpu
def test_gpu_state_round_trip_and_a_step_from_a_set_state(gpu):
    ni = 65
    r = rig("long")
    nb, nj, table = r["nb"], r["nj"], r["table"]
    with rig_model() as dm:
        sk, sset = _skeleton_and_set(r, ni + 2)
        assert np.isnan(sset.state(model=dm)).all() and sset.state(model=dm).shape == (ni + 2, nj, 6)
        rng = np.random.RandomState(8)
        given = (r["pals"]["placed"][3][:ni, table["bone"], 12:15][:, :, None, :] + rng.normal(0, 0.05, (ni, nj, 2, 3))).reshape(ni, nj, 6).astype(F)
        given[5, 3, 2], given[6, 0, :] = np.inf, np.nan
        sset.set_state(given, dm)
        back = sset.state(ni + 2, dm)
        sr.assert_same(back[:ni], given, "round trip")
        assert np.isnan(back[ni:]).all()
        sset.set_state(given[:7] * 2, dm)                                     # a prefix
        given[:7] *= 2
        sr.assert_same(sset.state(ni, dm), given, "a prefix set")
        d_pal = Guarded(ni, nb, dm)
        src = r["pals"]["placed"][4][:ni]
        d_pal.upload(src)
        sset.step(d_pal, dt=1 / 60, n_instances=ni, model=dm)
        count = {}
        wp, ws = sr.step(table, src, given, 1 / 60, count=count)
        assert count["heal"] >= 2 and count["rotated"] > ni * 20
        sr.assert_same(d_pal.read("a step from a set state"), wp, "a step from a set state: palettes")
        sr.assert_same(sset.state(ni, dm), ws, "a step from a set state: state")
        _close(d_pal, sset, sk)

"""Reach: mmdx_reach_set_* and mmdx_palette_reach (include/mmdx.h).

There is no libmmd counterpart (the reference has no two-bone IK on finished palettes): as for the springs and the aim, the contract is
the arithmetic the header states, held by three statements that must agree bit for bit, with no tolerance anywhere (a NaN only has to
be a NaN) --
  * csrc/reach_math.hpp and csrc/reach_table.hpp compiled for the host (tests/reach_math_driver.cpp, a stand-alone program, plain and
    sanitized),
  * the numpy restatement tests/reach_ref.py, written from the header's text,
  * the gfx950 kernel (the same header compiled for the device),
and the geometric properties are asserted on the restatement, on the CPU, within tolerances measured against a binary64 evaluation of
the same formulas.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from simple_mmd_renderer_amd import _capi as api
from simple_mmd_renderer_amd import synth, vmd
from simple_mmd_renderer_amd.engine import AimSet, DeformModel, DeviceBuffer, ReachSet, SocketSet, SpringSet, device_count
from tests import host_program as hp
from tests import palette_place_ref as pp
from tests import palette_sockets_ref as ps
from tests import reach_ref as rr
from tests.test_capi_symbols import declared_symbols
from tests.test_palette_sockets import crowd_placements, rig_model, rig_small
from tests.test_spring_bones import GUARD, SENT, Guarded

ENTRY_POINTS = ("mmdx_reach_set_create", "mmdx_reach_set_destroy", "mmdx_reach_set_get_info", "mmdx_palette_reach")
ROOT = os.path.dirname(rr.HERE)
INVALID, BAD_INDEX, UNSUPPORTED = 1, 2, 6
F, U = np.float32, np.uint32
DEV = api.PALETTE_ON_DEVICE | api.OUT_ON_DEVICE
PLACE_DEV = DEV | api.PLACE_ON_DEVICE
LDS = 16 * (3 * 12 + 1) * 4
# The worst case of the binary32 restatement, evaluated in binary64, over the case table and 3 000 steps of a target circling the
# swaying 41-bone rig, every set of the rig (test_tolerances_... prints the figures): the tip against Gc relative to max(1, |Gc|),
# the two bone lengths relative to l1 and l2, the new elbow's distance from the plane of dh and the bend direction relative to l1 --
# these three as they are, whatever m: by m they show no 1 / m growth (the worst tip, 4.5e-5, is at m = 1.1e-3; below m = 1e-4 it
# is 1.1e-6) -- and |C C^T - I| TIMES m for C_0 (m = 1 + cs of M_a) and C_1 (the smaller m of M_a and M_b): u and v of a rot are unit
# vectors to a rounding error, which the formula divides by m, as the aim's does, and the sweep shows it (unscaled 3.4e-2 at
# m < 1e-4, 1.2e-6 at m > 0.5).  The assertions take 4 x these figures, for inputs not seen.
WORST = dict(tip=4.6e-5, length=4.6e-5, rigid0=1.2e-6, rigid1=1.2e-6, plane=4.4e-6)
TOL = {k: 4 * v for k, v in WORST.items()}


@pytest.fixture(autouse=True)
def _lib(hip_lib):
    return hip_lib


def _close(*things):
    for t in things:
        for x in (t if isinstance(t, (list, tuple)) else [t]):
            (x.free if hasattr(x, "free") else x.close)()


# ---------------------------------------------------------------------------------------- CPU ----
def test_reach_entry_points_are_declared_exported_and_bound(hip_lib):
    syms = declared_symbols()
    for name in ENTRY_POINTS:
        assert name in syms and hasattr(hip_lib, name) and name in api.SIGNATURES, name
    hdr = open(os.path.join(ROOT, "include", "mmdx.h")).read()
    for text in ("typedef struct mmdx_reach_set_desc {", "typedef struct mmdx_reach_set_info {", "typedef struct mmdx_reach_args {",
                 "#define MMDX_ABI_VERSION 3u", "MMDX_REACH_TARGETS_ON_DEVICE = (1u << 19)", "#define MMDX_REACH_MAX_REACHES 16",
                 "MMDX_REACH_KEEP_END_ROTATION = 1u"):
        assert text in hdr, text
    assert hip_lib.mmdx_abi_version() == 3
    desc, info, args, tgt_dev, pal_dev, mr, keep = hp.c_values(
        ["sizeof(mmdx_reach_set_desc)", "sizeof(mmdx_reach_set_info)", "sizeof(mmdx_reach_args)", "MMDX_REACH_TARGETS_ON_DEVICE",
         "MMDX_PALETTE_ON_DEVICE", "MMDX_REACH_MAX_REACHES", "MMDX_REACH_KEEP_END_ROTATION"])
    assert C.sizeof(api.ReachSetDesc) == desc == 2 * 4 + 5 * 8 + 4 + 4
    assert C.sizeof(api.ReachSetInfo) == info == 6 * 4
    assert C.sizeof(api.ReachArgs) == args == 4 * 4 + 3 * 8
    assert (api.REACH_TARGETS_ON_DEVICE, api.PALETTE_ON_DEVICE) == (tgt_dev, pal_dev) == (1 << 19, 1)
    assert (api.REACH_MAX_REACHES, rr.MAX_REACHES) == (mr, mr) == (16, 16)
    assert api.REACH_KEEP_END_ROTATION == rr.KEEP_END_ROTATION == keep == 1
    others = hp.c_values(["MMDX_ANIM_DT_ON_DEVICE | MMDX_ROOT_NORMALIZE | MMDX_EVENTS_DOMINANT_SIDE | MMDX_BLEND_A_ON_DEVICE | "
                          "MMDX_BLEND_B_ON_DEVICE | MMDX_BLEND_PARAMS_ON_DEVICE | MMDX_PLACE_ON_DEVICE | MMDX_PLACE_MATRIX | "
                          "MMDX_SPRING_RESET | MMDX_SPRING_DT_ON_DEVICE | MMDX_AIM_TARGETS_ON_DEVICE | 0xFF"])[0]
    assert tgt_dev & others == 0                                           # a bit no other call accepts
    kernel_reach, = hp.c_values(["MMDX_DEBUG_KERNEL_REACH"], headers=("mmdx.h", "mmdx_bench.h"))
    assert kernel_reach == 6 and api.DEBUG_KERNELS[kernel_reach] == "reach"
    for m in ("reach", "reach_raw", "info", "close", "__enter__", "__exit__"):
        assert callable(getattr(ReachSet, m)), m
    for m in ("aim", "aim_raw", "info", "close", "__enter__", "__exit__"):          # (the neighbour class keeps what it had)
        assert callable(getattr(AimSet, m)) and m in vars(AimSet), m
    poser = open(os.path.join(ROOT, "simple_mmd_renderer_amd", "host", "mmdx_poser.hpp")).read()
    for text in ("class ReachSet", "mmdx_reach_set_create(", "mmdx_reach_set_destroy(", "mmdx_palette_reach("):
        assert text in poser, text


def test_case_table_contains_every_branch_the_header_names():
    """From the numpy side alone: what the driver and the kernel are about to be compared on."""
    case = rr.case_table()
    count = {}
    out = rr.reach(case["table"], case["pal"], case["targets"], count=count)
    missing = [k for k in rr.CASES if count.get(k, 0) < 1]
    assert not missing, (missing, count)
    assert [len(k["rows"]) for k in case["table"]] == [8, 3, 4, 3]
    assert sorted({d for k in case["table"] for _, d in k["rows"]}) == [0, 1, 2]
    nan_in, nan_out = np.isnan(case["pal"]).any(axis=(1, 2)), np.isnan(out).any(axis=(1, 2))
    assert np.nonzero(nan_in)[0].tolist() == np.nonzero(nan_out)[0].tolist() == [18, 19, 20, 21]      # a NaN row stays with its instance
    dead = [3, 4, 5, 6, 7]                                                 # weight 0, negative, NaN; a target that is not finite
    assert out[dead].tobytes() == case["pal"][dead].tobytes()
    rows = lambda k: [b for b, _ in case["table"][k]["rows"]]              # noqa: E731
    same = lambda i, k: out[i][rows(k)].tobytes() == case["pal"][i][rows(k)].tobytes()      # noqa: E731
    assert all(same(i, 3) for i in range(32))                             # lmin > lmax: never written
    assert same(8, 0) and same(11, 0) and same(12, 2) and same(13, 2)      # on A; the pole along dh; antiparallel in step 3, in step 4
    assert same(9, 0) and not same(10, 0)                                  # u1 == v1 and u2 == v2: the identity; the pole bends the elbow
    assert same(18, 0) and same(19, 0) and same(20, 0) and not same(18, 1) and not same(19, 2)      # all or nothing, per reach
    assert np.isnan(out[21, 10]).any() and np.isfinite(out[21, 12]).all() and out[21, 12].tobytes() != case["pal"][21, 12].tobytes()


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_host_build_of_the_arithmetic_equals_the_numpy_restatement(sanitize):
    case = rr.case_table()
    want = rr.reach(case["table"], case["pal"], case["targets"])
    shared = case["targets"][1]                                            # one target for everyone (weight 0.5)
    want_shared = rr.reach(case["table"], case["pal"], shared)
    exe = rr.build_driver(sanitize)
    tb, got = rr.run_driver(exe, case["parent"], case["rest"], case["reaches"], [(case["pal"], case["targets"]), (case["pal"], shared)])
    for a, b in zip(tb, case["table"]):
        assert a["rows"] == b["rows"]
        rr.assert_same(a["h"], np.stack([b["ha"], b["hb"], b["hc"]]), "rest positions")
    rr.assert_same(got[0], want, "palettes")
    rr.assert_same(got[1], want_shared, "palettes, one target for everyone")
    assert want.tobytes() != case["pal"].tobytes() and want_shared.tobytes() != case["pal"].tobytes()
    for name, reaches in rr.rig_sets().items():                            # the sets the GPU tests use, through the same two
        table = rr.build_table(case["parent"], case["rest"], reaches)
        pal = rr.fk_palettes(case["parent"], case["rest"], 9, step=2)
        tgt = rr.near_targets(table[0], pal, 4)
        _, got = rr.run_driver(exe, case["parent"], case["rest"], reaches, [(pal, tgt)])
        rr.assert_same(got[0], rr.reach(table, pal, tgt), name)


def _sweep():
    """The 3 000-step sweep as 3 000 instances of one call: the swaying 41-bone rig (the targets circle per reach)."""
    parent, rest = rr.reach_rig()
    return parent, rest, rr.fk_palettes(parent, rest, 3000, step=1, amplitude=0.5)


def _errors(table, pal, targets):
    """The worst figures of WORST over every applied (instance, reach) of the binary32 restatement, evaluated in binary64, and how
    many were applied.  With MMDX_REACH_KEEP_END_ROTATION the 3x3 of the end bone's row is asserted to be value for value what it was."""
    f8 = np.float64
    trace = []
    got = rr.reach(table, pal, targets, trace=trace)
    live = rr.live_rows(pal, targets)
    worst, n = dict.fromkeys(WORST, 0.0), 0
    norm = lambda v: np.sqrt((v * v).sum(axis=1))                          # noqa: E731
    up = lambda key, v: worst.__setitem__(key, max(worst[key], float(np.max(v))))      # noqa: E731
    for k, t in zip(table, trace):
        new, old = got[live].astype(f8), pal[live].astype(f8)
        ok = t["ok"] & np.isfinite(new[:, [k["a"], k["b"], k["c"]]]).all(axis=(1, 2)) & np.isfinite(t["c1"]).all(axis=1)
        if not ok.any():
            continue
        n += int(ok.sum())
        new, old = new[ok], old[ok]
        A, Gc, l1, l2, dh, bend = (t[x][ok].astype(f8) for x in ("A", "Gc", "l1", "l2", "dh", "bend"))
        tip, b1 = rr.tip_now(k, new), rr.pt(k["hb"].astype(f8), new[:, k["b"]])
        m_a, m_b = t["m_a"][ok].astype(f8), t["m_b"][ok].astype(f8)
        up("tip", np.abs(tip - Gc).max(axis=1) / np.maximum(1.0, np.abs(Gc).max(axis=1)))
        up("length", np.abs(norm(b1 - rr.pt(k["ha"].astype(f8), new[:, k["a"]])) - l1) / l1)
        up("length", np.abs(norm(tip - b1) - l2) / l2)
        for key, c, m in (("rigid0", t["c0"], m_a), ("rigid1", t["c1"], np.minimum(m_a, m_b))):      # (rot divides a rounding error by m)
            r = c[ok][:, [0, 1, 2, 4, 5, 6, 8, 9, 10]].reshape(-1, 3, 3).astype(f8)
            up(key, np.abs(r @ r.transpose(0, 2, 1) - np.eye(3)).max(axis=(1, 2)) * m)
        normal = np.cross(dh, bend)
        flat = norm(normal) > 0.5                                          # (dh and the bend direction are perpendicular unit vectors)
        up("plane", (np.abs(((b1 - A) * normal).sum(axis=1)) / l1)[flat])
        if k["flags"] & rr.KEEP_END_ROTATION:
            three = [0, 1, 2, 4, 5, 6, 8, 9, 10]
            assert (new[:, k["c"]][:, three] == old[:, k["c"]][:, three]).all(), "the end bone's rotation changed"
            assert (new[:, k["c"], 12:15] != old[:, k["c"], 12:15]).any()
    return worst, n


def test_tolerances_the_tip_ends_on_the_clamped_target_and_the_limb_stays_rigid():
    """The tip (with the flag: the end bone's pivot) ends on Gc; |B' - A| and |T' - B'| keep l1 and l2; C_0 and C_1 are rigid; the new
    elbow lies in the plane of dh and the bend direction (or the pole); with the flag the 3x3 of row'(c) is that of row(c) -- over the
    case table and the sweep, every set of the rig."""
    parent, rest, pal = _sweep()
    case = rr.case_table()
    figures = [_errors(case["table"], case["pal"], case["targets"])]
    for name, reaches in rr.rig_sets().items():
        table = rr.build_table(parent, rest, reaches)
        figures.append(_errors(table, pal, rr.circling_targets(table[0], pal.shape[0])))
        assert figures[-1][1] > 2000, (name, figures[-1][1])                # (the sweep is not a sweep of refusals)
    worst = {k: max(f[0][k] for f in figures) for k in WORST}
    print("worst of %d applied reaches: %s" % (sum(f[1] for f in figures), ", ".join("%s %.3g" % kv for kv in worst.items())))
    for k in WORST:
        assert worst[k] <= TOL[k], (k, worst[k], TOL[k])


def test_weight_fades_extension_clamps_and_the_pole_picks_the_side():
    """Weight w: the tip moves the share w of the way (to the tolerance of the tip).  max_extension 0.9: a far target leaves the tip at
    0.9 of the limb's length from A.  A straight limb bends towards its pole, and towards the other side with the pole negated."""
    parent, rest, pal = _sweep()
    pal = pal[:400]
    table = rr.build_table(parent, rest, [rr.make_reach(18, 19, 20)])
    k = table[0]
    tgt = rr.near_targets(k, pal, 12, spread=0.6)
    t0 = rr.tip_now(k, pal)
    for w in (0.25, 0.5, 1.0):
        t = tgt.copy()
        t[:, 3] = w
        trace = []
        moved = rr.tip_now(k, rr.reach(table, pal, t, trace=trace))
        want = t0 + (tgt[:, :3].astype(np.float64) - t0) * w
        inside = trace[0]["ok"] & (np.abs(trace[0]["Gc"].astype(np.float64) - want).max(axis=1) < 1e-5)
        assert inside.sum() > 100                                           # (targets the clamp left alone)
        assert (np.abs(moved - want).max(axis=1) / np.maximum(1.0, np.abs(want).max(axis=1)))[inside].max() <= TOL["tip"]
    far = tgt.copy()
    far[:, :3] += 50.0
    trace = []
    out = rr.reach(rr.build_table(parent, rest, [rr.make_reach(18, 19, 20, max_extension=0.9)]), pal, far, trace=trace)
    a = rr.pt(k["ha"].astype(np.float64), pal[:, k["a"]].astype(np.float64))
    full = (trace[0]["l1"] + trace[0]["l2"]).astype(np.float64)
    dist = np.linalg.norm(rr.tip_now(k, out) - a, axis=1)
    assert trace[0]["ok"].all() and (np.abs(dist / full - 0.9) <= TOL["length"] + TOL["tip"]).all()
    ident = np.tile(np.eye(4, dtype=F).reshape(16), (1, len(parent), 1))
    elbows = []
    for pole in ((0, 0, -1), (0, 0, 1)):
        arm = rr.build_table(parent, rest, [rr.make_reach(10, 12, 13, pole=pole)])
        out = rr.reach(arm, ident, np.array([4, 5, 0, 1], F))
        elbows.append(rr.pt(arm[0]["hb"].astype(np.float64), out[:, 12].astype(np.float64))[0])
        assert np.abs(rr.tip_now(arm[0], out)[0] - [4, 5, 0]).max() <= TOL["tip"] * 5      # (relative to max(1, |Gc|) = 5)
    assert elbows[0][2] < -1.0 and elbows[1][2] > 1.0 and abs(elbows[0][1] - 5) < 1e-6      # l1 = l2 = 2, d = 3: the elbow 1.32 off the axis


def _skeleton(parent, rest):
    return vmd.Skeleton(rest, parent)


def _reach_set(sk, reaches):
    """engine.ReachSet from reaches as rr.make_reach makes them (a tip point of None: the end bone's rest position)."""
    return ReachSet(sk, [{k: v for k, v in r.items() if v is not None} for r in reaches])


def test_reach_set_create_refuses_what_the_header_lists_without_a_device(hip_lib):
    parent, rest = rr.reach_rig()
    sk = _skeleton(parent, rest)
    err = lambda: (hip_lib.mmdx_last_error_string() or b"").decode()          # noqa: E731
    out = C.c_void_p()
    keep = []

    def create(reaches=None, struct_size=None, reserved0=0, skeleton=sk.h, null=(), n_reaches=None):
        reaches = [rr.make_reach(10, 12, 13)] if reaches is None else reaches
        arrays = rr.desc_arrays(reaches, rest)
        keep.extend(arrays)
        d = api.ReachSetDesc(C.sizeof(api.ReachSetDesc) if struct_size is None else struct_size, len(reaches) if n_reaches is None else n_reaches)
        d.bones, d.tip_point, d.pole, d.max_extension, d.flags = (a.ctypes.data for a in arrays)
        d.reserved0 = reserved0
        for name in null:
            setattr(d, name, None)
        return hip_lib.mmdx_reach_set_create(skeleton, C.byref(d), C.byref(out))
    nan, inf = float("nan"), float("inf")
    assert create(skeleton=None) == INVALID and "NULL" in err()
    assert hip_lib.mmdx_reach_set_create(sk.h, None, C.byref(out)) == INVALID and "NULL" in err()
    assert hip_lib.mmdx_reach_set_create(sk.h, None, None) == INVALID and "out_set" in err()
    assert create(struct_size=C.sizeof(api.ReachSetDesc) - 8) == INVALID and "struct_size" in err()
    assert create(reserved0=1) == INVALID and "reserved0" in err()
    assert create(reaches=[rr.make_reach(41, 12, 13, tip_point=(0, 0, 0))]) == BAD_INDEX and "bones[0][0] = 41" in err()
    assert create(reaches=[rr.make_reach(10, 12, 13), rr.make_reach(14, 99, 17, tip_point=(0, 0, 0))]) == BAD_INDEX and "bones[1][1] = 99" in err()
    assert create(reaches=[rr.make_reach(10, 12, 41, tip_point=(0, 0, 0))]) == BAD_INDEX and "bones[0][2] = 41" in err()
    assert create(reaches=[rr.make_reach(12, 10, 13)]) == INVALID and "b = 10 of reach 0 is not a strict descendant of a = 12" in err()      # upside down
    assert create(reaches=[rr.make_reach(10, 10, 13)]) == INVALID and "b = 10 of reach 0 is not a strict descendant" in err()
    assert create(reaches=[rr.make_reach(10, 14, 15)]) == INVALID and "b = 14 of reach 0 is not a strict descendant" in err()                  # a sibling branch
    assert create(reaches=[rr.make_reach(10, 12, 12)]) == INVALID and "c = 12 of reach 0 is not a strict descendant of b = 12" in err()
    assert create(reaches=[rr.make_reach(10, 12, 11)]) == INVALID and "c = 11 of reach 0 is not a strict descendant" in err()
    assert create(reaches=[rr.make_reach(10, 12, 15)]) == INVALID and "c = 15 of reach 0 is not a strict descendant" in err()
    for ext in (0.0, -0.5, 1.001, inf):
        assert create(reaches=[rr.make_reach(10, 12, 13, max_extension=ext)]) == INVALID and "max_extension of reach 0 is outside (0, 1]" in err(), ext
    assert create(reaches=[rr.make_reach(10, 12, 13, max_extension=nan)]) == INVALID and "NaN" in err()
    assert create(reaches=[rr.make_reach(10, 12, 13, tip_point=(0, nan, 0))]) == INVALID and "NaN" in err()
    assert create(reaches=[rr.make_reach(10, 12, 13, pole=(0, 0, nan))]) == INVALID and "NaN" in err()
    assert create(reaches=[rr.make_reach(10, 12, 13, pole=(0, 0, 0))]) == INVALID and "pole of reach 0 is zero or not finite" in err()
    assert create(reaches=[rr.make_reach(10, 12, 13, pole=(0, inf, 0))]) == INVALID and "zero or not finite" in err()
    assert create(n_reaches=0) == INVALID and "n_reaches = 0" in err()
    limbs = 17                                                             # 17 three-bone limbs on a root: 17 disjoint subtrees
    flat_parent = np.array([-1] + [p for r in range(limbs) for p in (0, 1 + 3 * r, 2 + 3 * r)], np.int32)
    flat = _skeleton(flat_parent, np.zeros((1 + 3 * limbs, 3), F))
    many = [rr.make_reach(1 + 3 * r, 2 + 3 * r, 3 + 3 * r, tip_point=(0, 0, 0)) for r in range(limbs)]
    assert create(reaches=many, skeleton=flat.h) == INVALID and "n_reaches = 17" in err()
    assert create(reaches=many[:16], skeleton=flat.h) == api.OK
    hip_lib.mmdx_reach_set_destroy(out)
    flat.close()
    huge_parent = np.zeros((1 << 20) + 1, np.int32)                        # 2^20 + 1 bones: a root, one limb, leaves
    huge_parent[[0, 2, 3]] = -1, 1, 2
    huge = _skeleton(huge_parent, np.zeros((huge_parent.size, 3), F))
    assert create(reaches=[rr.make_reach(1, 2, 3, tip_point=(0, 0, 0))], skeleton=huge.h) == UNSUPPORTED and "more than 2^20 bones" in err()
    huge.close()
    for flags in (2, 3, 1 << 31):
        assert create(reaches=[rr.make_reach(10, 12, 13, flags=flags)]) == INVALID and "unknown flag bits in flags of reach 0" in err(), flags
    assert create(reaches=[rr.make_reach(4, 5, 10), rr.make_reach(10, 12, 13)]) == INVALID \
        and "the subtrees of reach 0 and reach 1 intersect at bone 10" in err()
    assert create(reaches=[rr.make_reach(12, 13, 32), rr.make_reach(10, 11, 12)]) == INVALID and "intersect at bone 12" in err()
    assert create(reaches=[rr.make_reach(18, 19, 20), rr.make_reach(18, 19, 20)]) == INVALID and "intersect" in err()
    for name in ("bones", "tip_point", "pole", "max_extension", "flags"):
        assert create(null=(name,)) == INVALID and "NULL" in err(), name
    assert out.value is None                                               # a refusal hands out nothing
    # what is allowed: extension 1 and a tiny one, a tip point anywhere, both flag values; and the set reports itself
    s = ReachSet(sk, [dict(bones=(10, 12, 13), max_extension=1.0, tip_point=(1e6, 0, 0)), dict(bones=(14, 15, 17), max_extension=1e-3, pole=(0, 5, 0)),
                      dict(bones=(18, 19, 20), keep_end_rotation=True), dict(bones=(36, 37, 38), flags=1)])
    assert s.info() == dict(n_reaches=4, n_subtree_rows=8 + 4 + 3 + 3, n_bones=41, device_ordinal=-1)
    info = api.ReachSetInfo(8)
    assert hip_lib.mmdx_reach_set_get_info(s.h, C.byref(info)) == INVALID and "struct_size" in err()
    with ReachSet(sk, [dict(bones=(18, 19, 20))]) as r, AimSet(sk, [dict(links=[7])]) as a:      # both are context managers
        assert r.info()["n_reaches"] == 1 and a.info()["n_aims"] == 1
    assert r.h is None and a.h is None
    hip_lib.mmdx_reach_set_destroy(None)                                   # like free(NULL)
    sk.close()                                                             # the set copied what it needs
    assert s.info()["n_bones"] == 41
    s.close()


def test_palette_reach_refuses_bad_arguments_before_any_device_call(hip_lib):
    """Every call here carries its defect AND a host list with an id that is no instance behind it (or is refused ahead of any
    pointer being looked at), so none of them can reach a device."""
    parent, rest = rr.reach_rig()
    sk = _skeleton(parent, rest)
    s = ReachSet(sk, [dict(bones=(10, 12, 13))])
    err = lambda: (hip_lib.mmdx_last_error_string() or b"").decode()          # noqa: E731
    tgt = np.zeros((4, 4), F)
    P = 0x10000                                                            # stands for a device address; never dereferenced
    ids = np.array([0, 9], U)
    ON = api.PALETTE_ON_DEVICE | api.REACH_TARGETS_ON_DEVICE

    def call(set_h=s.h, struct_size=None, flags=api.PALETTE_ON_DEVICE, ni=4, stride=4, palettes=P, targets=tgt.ctypes.data, select=None,
             null_args=False):
        a = api.ReachArgs(C.sizeof(api.ReachArgs) if struct_size is None else struct_size, flags, ni, stride, palettes, targets)
        if select is not None:
            a.select = C.pointer(select)
        return hip_lib.mmdx_palette_reach(set_h, None, None if null_args else C.byref(a))
    host_bad = vmd.instance_select(ids.ctypes.data, 2, None, on_device=False)          # id 9 >= 4: the refusal behind the others
    assert call(select=host_bad) == INVALID and "ids[1] = 9 is not below n_instances" in err()          # the guard itself
    assert call(flags=ON, targets=P, select=host_bad) == INVALID and "ids[1]" in err()
    assert call(set_h=None) == INVALID and "NULL" in err()
    assert call(null_args=True) == INVALID and "NULL" in err()
    assert call(struct_size=C.sizeof(api.ReachArgs) - 8, select=host_bad) == INVALID and "struct_size" in err()
    for bad in (2, 4, 1 << 8, 1 << 10, 1 << 16, 1 << 17, 1 << 18, 1 << 20, 1 << 31):
        assert call(flags=api.PALETTE_ON_DEVICE | bad, select=host_bad) == INVALID and "unknown flag bits" in err(), bad
    assert call(flags=api.REACH_TARGETS_ON_DEVICE, select=host_bad) == INVALID and "MMDX_PALETTE_ON_DEVICE" in err()
    for stride in (1, 2, 3, 5, 6, 18):
        assert call(stride=stride, select=host_bad) == INVALID and "target_stride = %d" % stride in err()
    assert call(palettes=None, select=host_bad) == INVALID and "palettes / targets is NULL" in err()
    assert call(targets=None, select=host_bad) == INVALID and "palettes / targets is NULL" in err()
    assert call(palettes=P + 4, select=host_bad) == INVALID and "palettes must be 16-byte aligned" in err()
    assert call(flags=ON, targets=P + 8, select=host_bad) == INVALID and "device targets must be 16-byte aligned" in err()
    assert call(ni=(1 << 23) + 1, select=host_bad) == UNSUPPORTED and "2^23" in err()
    big = vmd.instance_select(P, (1 << 23) + 1)
    assert call(select=big) == UNSUPPORTED and "2^23" in err()
    sel = vmd.instance_select(P + 2, 2)
    assert call(select=sel) == INVALID and "4-byte aligned" in err()
    sel = vmd.instance_select(ids.ctypes.data, 2, None, on_device=False)
    sel.reserved0 = 1
    assert call(select=sel) == INVALID and "reserved0" in err()
    assert call(ni=0, palettes=None, targets=None) == api.OK               # nothing to do, nothing looked at
    assert call(ni=0, palettes=None, targets=None, stride=0) == api.OK
    _close(s, sk)


def test_planner_swept_on_the_cpu():
    """plan_reach_launch through the sanitized driver: 16 instances to a workgroup of 256 lanes at every crowd size; the workgroups
    cover the cells exactly once; LDS is 16 * (3 * 12 + 1) words."""
    cells = [1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 257, 1000, 4095, 4096, 4097, 16384, 100000, (1 << 23) - 1, 1 << 23]
    got = rr.plan(cells, rr.build_driver(True))
    assert len(got) == len(cells)
    for c, (block, threads, nblocks, lds) in zip(cells, got):
        assert (block, threads, lds) == (16, 256, LDS) and LDS == 2368, (c, block, threads, lds)
        assert (nblocks - 1) * block < c <= nblocks * block


def test_kernel_resources_no_spills_no_scratch():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), api.LIB_PATH, "reach_kernel"],
                         capture_output=True, text=True, check=True).stdout.splitlines()
    names = {l.split(" vgpr ")[0].strip() for l in out}
    assert names == {"reach_kernel<true>", "reach_kernel<false>"}
    for l in out:
        f = l.split(" vgpr ")[1].split()
        res = dict(zip(["vgpr"] + f[1::2], (int(v) for v in f[0::2])))
        assert res["spill"] == 0 and res["scratch"] == 0 and res["vgpr"] <= 128, l


# ---------------------------------------------------------------------------------------- GPU ----
@pytest.fixture
def gpu(hip_lib):
    assert device_count() >= 1, "no HIP device visible: the GPU tests must run on the MI355X box"
    return hip_lib


NI_MAX = 257
_rig = {}


def rig():
    """The 41-bone rig, computed once and shared, never modified: palettes of 257 instances in model space and placed, the palettes
    of a second model ("the props": the same rig at another step, for a sockets slab), and per reach set of rr.rig_sets() its table
    and, per space, its targets: near the first reach's tip, every fifth at weight 0.4, some at weight 0."""
    if not _rig:
        parent, rest = rr.reach_rig()
        place = crowd_placements(NI_MAX)
        pals = {"model space": rr.fk_palettes(parent, rest, NI_MAX, step=5)}
        pals["placed"] = pp.place_crowd(pals["model space"], place, False)
        props = pp.place_crowd(rr.fk_palettes(parent, rest, NI_MAX, step=9, amplitude=0.7), place, False)
        sets = rr.rig_sets()
        tables = {k: rr.build_table(parent, rest, v) for k, v in sets.items()}
        targets = {}
        for n, (name, table) in enumerate(tables.items()):
            for space, pal in pals.items():
                t = rr.near_targets(table[0], pal, 20 + n)
                t[:, 3] = np.where(np.arange(NI_MAX) % 5 == 4, 0.4, 1.0)
                t[3::37, 3] = 0.0                                          # some instances do not reach
                targets[name, space] = t
        _rig.update(parent=parent, rest=rest, nb=len(parent), sets=sets, tables=tables, pals=pals, props=props, targets=targets)
    return _rig


def big_model():
    """A model with the rig's 41 bones (the calls take a stream and, for the sockets, a bone count from it)."""
    return DeformModel(synth.make_model(64, 41, 0, 0, seed=31))


def _shape(dm):
    s = dm.last_launch_shape()
    return s["kernel"], s["threads"], s["group"], s["ngroups"], s["lds"], s["select"]


@pytest.mark.gpu
@pytest.mark.parametrize("ni", [1, 15, 16, 17, 33, 257])
def test_gpu_rows_equal_the_restatement(gpu, ni):
    """Every set of the rig (1 and 4 reaches; subtrees of 3, 4, 8 with non-contiguous indices, 11, 26 and 37 rows, so that phase B's
    item count is no multiple of 256; twist bones between a and b and between b and c; both flag values), model space and placed,
    targets every 4 floats, one target for everyone, host targets and a real sockets slab of a second model at stride 16: the whole
    palette array between its sentinels equals the restatement's, byte for byte, and the debug record proves the launch shape."""
    r = rig()
    nb = r["nb"]
    with big_model() as dm:
        sk = _skeleton(r["parent"], r["rest"])
        d_pal = Guarded(ni, nb, dm)
        sockets = SocketSet.from_skeleton(dm, sk, [0, 13, 20])
        d_props, d_slab = DeviceBuffer.from_numpy(r["props"][:ni]), DeviceBuffer(3 * ni * 64)
        sockets.sockets(d_props, d_slab, n_instances=ni)
        dm.sync()
        slab = d_slab.download((3, ni, 16), F)[1]                           # where each instance's prop hand is
        assert (slab[:, 15] == 1.0).all()
        for name, reaches in r["sets"].items():
            rset = _reach_set(sk, reaches)
            table = r["tables"][name]
            assert rset.info()["n_subtree_rows"] == sum(len(k["rows"]) for k in table) and rset.info()["n_reaches"] == len(table)
            for space in ("model space", "placed"):
                src, tgt = r["pals"][space][:ni], r["targets"][name, space][:ni]
                d_tgt = DeviceBuffer.from_numpy(tgt)
                plans = [("stride 4", d_tgt.ptr, 4, tgt), ("one target", d_tgt.ptr + 16 * (ni // 2), 0, tgt[ni // 2]),
                         ("host targets", tgt, None, tgt)]
                if space == "placed":
                    plans.append(("sockets slab", d_slab.ptr + ni * 64 + 48, 16, slab[:, 12:16]))
                for what, ptr, stride, want_tgt in plans:
                    what = f"{name}, NI {ni}, {space}, {what}"
                    d_pal.upload(src)
                    if stride is None:
                        rset.reach(dm, d_pal, ptr, n_instances=ni)
                    else:
                        rset.reach(dm, d_pal, ptr, stride=stride, n_instances=ni)
                    assert _shape(dm) == ("reach", 256, 16, (ni + 15) // 16, LDS, 0), what
                    want = rr.reach(table, src, want_tgt)
                    got = d_pal.read(what)
                    rr.assert_same(got, want, what)
                    outside = np.ones(nb, bool)
                    outside[[b for k in table for b, _ in k["rows"]]] = False
                    assert got[:, outside].tobytes() == src[:, outside].tobytes(), what + ": a row outside the subtrees changed"
                    assert want.tobytes() != src.tobytes(), what
                d_tgt.free()
            assert rset.info()["device_ordinal"] >= 0
            rset.close()
        _close(d_pal, d_props, d_slab, sockets, sk)


@pytest.mark.gpu
def test_gpu_a_nan_row_stays_with_its_instance(gpu):
    """65 instances, the 4-reach set, placed.  A NaN in the row of b of instance 20 and an infinite target of instance 21: their
    neighbours, in the same workgroup, stay exact, instance 21 keeps every byte, instance 20 every byte of that reach."""
    r = rig()
    ni, nb, table = 65, r["nb"], r["tables"]["limbs"]
    src, tgt = r["pals"]["placed"][:ni].copy(), r["targets"]["limbs", "placed"][:ni].copy()
    src[20, 12, 6] = np.nan
    tgt[21, 1] = np.inf
    with big_model() as dm:
        sk = _skeleton(r["parent"], r["rest"])
        rset = _reach_set(sk, r["sets"]["limbs"])
        d_pal, d_tgt = Guarded(ni, nb, dm), DeviceBuffer.from_numpy(tgt)
        d_pal.upload(src)
        rset.reach(dm, d_pal, d_tgt, n_instances=ni)
        assert _shape(dm) == ("reach", 256, 16, 5, LDS, 0)
        got, want = d_pal.read("a NaN row"), rr.reach(table, src, tgt)
        rr.assert_same(got, want, "a NaN row")
        arm = [b for b, _ in table[0]["rows"]]
        assert got[20][arm].tobytes() == src[20][arm].tobytes() and got[20].tobytes() != src[20].tobytes()
        assert np.isfinite(np.delete(got, 20, axis=0)).all() and got[21].tobytes() == src[21].tobytes()
        assert got[19].tobytes() != src[19].tobytes() and got[22].tobytes() != src[22].tobytes()
        _close(d_pal, d_tgt, rset, sk)


@pytest.mark.gpu
def test_gpu_case_table_through_the_kernel(gpu):
    """The 32 instances of the case table -- every branch of steps 0-6 --, tiled over 81 instances with a shift, so that every case
    sits on several lanes of six workgroups per reach: the kernel's rows equal the restatement's."""
    case = rr.case_table()
    ni = 81
    pick = (np.arange(ni) * 5 + 3) % 32                                     # (5 and 32 are coprime: every case, at changing lanes)
    pal, targets = case["pal"][pick], case["targets"][pick]
    assert set(pick.tolist()) == set(range(32))
    nb = pal.shape[1]
    with big_model() as dm:
        sk = _skeleton(case["parent"], case["rest"])
        rset = _reach_set(sk, case["reaches"])
        d_pal, d_tgt = Guarded(ni, nb, dm), DeviceBuffer.from_numpy(targets)
        d_pal.upload(pal)
        rset.reach(dm, d_pal, d_tgt, n_instances=ni)
        assert _shape(dm) == ("reach", 256, 16, 6, LDS, 0)
        rr.assert_same(d_pal.read("the case table"), rr.reach(case["table"], pal, targets), "the case table")
        _close(d_pal, d_tgt, rset, sk)


SEL_IDS = np.array([3, 64, 0, 7, 33, 1, 12, 40, 16, 17, 63, 21, 22, 23, 24, 25, 26, 27], U)
SEL_IDS_DEV = np.array([3, 64, 0, 70, 7, 0xFFFFFFFF, 12, 40, 16, 17, 63, 21, 22, 23, 24, 25, 26, 27], U)     # 70 and 2^32-1: no instances of 65


@pytest.mark.gpu
@pytest.mark.parametrize("where", ["host list", "device list"])
def test_gpu_select_reaches_the_listed_instances_only(gpu, where):
    """65 instances, the 4-reach set, placed palettes, 18 list positions (two workgroups of 16).  Lists with count NULL, 0, 5, 17 and
    100 (above n_ids): listed instances get the restatement's rows -- by their own target, not the list position's --, unlisted ones
    keep every byte; device ids that are no instance are skipped; a duplicate-free shuffle of all 65; a list of capacity 0; a host id
    that is no instance."""
    ni = 65
    r = rig()
    nb, table = r["nb"], r["tables"]["limbs"]
    src, tgt = r["pals"]["placed"][:ni], r["targets"]["limbs", "placed"][:ni]
    with big_model() as dm:
        sk = _skeleton(r["parent"], r["rest"])
        rset = _reach_set(sk, r["sets"]["limbs"])
        d_pal, d_tgt = Guarded(ni, nb, dm), DeviceBuffer.from_numpy(tgt)
        ids = SEL_IDS if where == "host list" else SEL_IDS_DEV
        shuffled = np.random.RandomState(5).permutation(ni).astype(U)
        d_cnt = DeviceBuffer(4)
        for ids, counts in ((ids, (None, 0, 5, 17, 100)), (shuffled, (None, 40))):
            d_ids = DeviceBuffer.from_numpy(ids)
            for count in counts:
                what = f"{where}, {ids.size} ids, count {count}"
                if where == "host list":
                    cnt = C.c_uint32(count or 0)
                    sel = vmd.instance_select(ids.ctypes.data, ids.size, C.addressof(cnt) if count is not None else None, on_device=False)
                else:
                    d_cnt.upload(np.array([count or 0], U))
                    sel = vmd.instance_select(d_ids.ptr, ids.size, d_cnt.ptr if count is not None else None)
                d_pal.upload(src)
                rset.reach(dm, d_pal, d_tgt, select=sel, n_instances=ni)
                used = [int(i) for i in (ids if count is None else ids[:min(count, ids.size)]) if i < ni]
                want = rr.reach(table, src, tgt, ids=used)
                unlisted = np.ones(ni, bool)
                unlisted[used] = False
                assert want[unlisted].tobytes() == src[unlisted].tobytes() and (not used or want.tobytes() != src.tobytes())
                rr.assert_same(d_pal.read(what), want, what)
                if used:
                    cells = ids.size if where == "device list" else len(used)
                    assert _shape(dm) == ("reach", 256, 16, (cells + 15) // 16, LDS, 1), what
            dm.sync()
            d_ids.free()
        d_ids = DeviceBuffer.from_numpy(SEL_IDS)
        d_pal.upload(src)
        rset.reach(dm, d_pal, d_tgt, select=vmd.instance_select(d_ids.ptr, 0), n_instances=ni)
        assert d_pal.read("n_ids 0").tobytes() == src.tobytes()
        bad = np.array([1, 65], U)
        with pytest.raises(api.MmdxError, match="is not below n_instances"):
            rset.reach(dm, d_pal, d_tgt, select=vmd.instance_select(bad.ctypes.data, 2, None, on_device=False), n_instances=ni)
        assert d_pal.read("after the refusal").tobytes() == src.tobytes()
        _close(d_pal, d_tgt, d_ids, d_cnt, rset, sk)


@pytest.mark.gpu
def test_gpu_recorded_frame_replayed_40_times_on_a_borrowed_stream(gpu, monkeypatch):
    """[blend solve, place, sockets of a second model, aim, reach, spring step, palette bounds] recorded once on a stream of the test's
    that both models borrow, replayed 40 times with the clip times, the hero's palettes and dt rewritten in device memory: after every
    replay the palettes equal the restatements' aim, reach and spring step on the palettes solve and place give for those times, with
    the targets the sockets call wrote.  The aim's subtree holds the reach's, the reach's holds a spring chain and its anchor: reach
    reads what aim wrote, the springs read what reach wrote.  Host targets, a host list and a fresh set are refused while recording."""
    from tests import aim_ref as ar
    from tests import hip_stream_util as hs
    from tests import motion_blend_ref as mb
    from tests import palette_bounds_ref as pb
    from tests import spring_ref as sr
    monkeypatch.delenv("MMDX_AIM_BLOCK", raising=False)
    hs.hip()
    ni, n_replays = 65, 40
    z = rig_small()
    parent, rest = z["parent"], z["rest"].astype(F)
    nb = len(parent)
    aims = [ar.make_aim([3, 7], eye_bone=16, shares=[0.5, 1.0], cos_limits=[0.7, 0.2], forward=(0.0, 0.3, -1.0))]
    atable = ar.build_table(parent, rest, aims)
    reaches = [rr.make_reach(7, 16, 18, max_extension=0.97, pole=(0.0, 1.0, 0.0))]
    rtable = rr.build_table(parent, rest, reaches)
    assert sorted(b for b, _ in atable[0]["rows"]) == [3, 7, 9, 10, 13, 16, 17, 18]
    assert rtable[0]["rows"] == [(7, 0), (10, 2), (16, 1), (17, 0), (18, 2)]
    chains, params = [[18, 10], [13]], [[20.0, 0.2, 1.0, 0.1], [0.0, 0.1, 1.0, 0.0]]
    stable = sr.build_table(parent, rest, chains, params, (0.0, -9.8, 0.0), None)
    names = [str(n) for n in mb.fixture()["bone_names"]]
    vs = [vmd.Vmd(p) for p in mb.BONE_VMDS]
    bms = [v.bind_bones(names) for v in vs]
    ms = vmd.MotionSet(bms)
    rng = np.random.RandomState(41)
    ca, cb = (np.arange(ni) % 2).astype(U), ((np.arange(ni) + 1) % 2).astype(U)
    w = rng.uniform(0, 1, ni).astype(F)
    t0 = rng.uniform(0, 1.5, ni)
    dts = rng.uniform(1 / 144, 1 / 30, n_replays).astype(F)
    hero_parent, hero_rest = ar.aim_rig()
    hero_place = np.roll(crowd_placements(ni), 1, axis=0)                   # everybody looks at and reaches for a neighbour
    hero_pals = [pp.place_crowd(ar.fk_palettes(hero_parent, hero_rest, ni, step=11 * k), hero_place, False) for k in range(3)]
    with rig_model() as dm, big_model() as hero, hs.Stream() as S:
        sk = vmd.Skeleton(rest, parent, z["level"], z["flags"])
        hero_sk = _skeleton(hero_parent, hero_rest)
        aset = AimSet(sk, [dict(links=[3, 7], eye_bone=16, shares=[0.5, 1.0], cos_limits=[0.7, 0.2], forward=(0.0, 0.3, -1.0))])
        rset = _reach_set(sk, reaches)
        sset = SpringSet(sk, chains, params, ni)
        sockets = SocketSet.from_skeleton(hero, hero_sk, [7, 13])              # the hero's head, for the aim, and hand, for the reach
        d_ca, d_cb, d_w = DeviceBuffer.from_numpy(ca), DeviceBuffer.from_numpy(cb), DeviceBuffer.from_numpy(w)
        d_ta, d_tb, d_dt = DeviceBuffer(ni * 8), DeviceBuffer(ni * 8), DeviceBuffer(4)
        d_place, d_pal, d_bnd = DeviceBuffer.from_numpy(crowd_placements(ni)), Guarded(ni, nb, dm), DeviceBuffer(ni * 24)
        d_hero, d_slab = DeviceBuffer(ni * 41 * 64), DeviceBuffer(2 * ni * 64)
        d_ids = DeviceBuffer.from_numpy(np.arange(ni, dtype=U))
        hand = d_slab.ptr + ni * 64 + 48

        def solve_place():
            sk.solve_motion_set_blend_time_device(ms, ni, d_ca.ptr, d_ta.ptr, d_cb.ptr, d_tb.ptr, d_w.ptr, d_pal.ptr, dm)
            dm.place_palettes(ni, d_pal.ptr, d_place.ptr, d_pal.ptr, PLACE_DEV)

        def frame():
            solve_place()
            sockets.sockets(d_hero, d_slab, n_instances=ni)
            aset.aim(dm, d_pal, d_slab.ptr + 48, stride=16, n_instances=ni)
            rset.reach(dm, d_pal, hand, stride=16, select=vmd.instance_select(d_ids.ptr, ni), n_instances=ni)
            sset.step(d_pal, dt_ptr=d_dt.ptr, n_instances=ni, model=dm)
            dm.palette_bounds_raw(ni, d_pal.ptr, d_bnd.ptr, DEV, 1.0, 1.0)
        try:
            dm.set_stream(S.ptr)
            hero.set_stream(S.ptr)
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
            d_hero.upload(hero_pals[0])
            fresh = ReachSet(sk, [dict(bones=(3, 9, 13))])                    # never ran on the device
            frame()                                                           # the run before recording: the sets go to the device
            S.synchronize()
            sset.set_state(sr.nan_state(ni, 3), dm)
            d_pal.buf.memset(SENT)
            dm.graph_begin()
            try:
                assert S.capture_status() == hs.CAPTURE_ACTIVE
                frame()
                with pytest.raises(api.MmdxError, match="targets must be in device memory"):
                    rset.reach(dm, d_pal, np.zeros((ni, 4), F), n_instances=ni)
                host_ids = np.arange(3, dtype=U)
                with pytest.raises(api.MmdxError, match="instance list must be in device memory"):
                    rset.reach(dm, d_pal, hand, stride=16, n_instances=ni,
                               select=vmd.instance_select(host_ids.ctypes.data, 3, None, on_device=False))
                with pytest.raises(api.MmdxError, match="must have run on this device before"):
                    fresh.reach(dm, d_pal, hand, stride=16, n_instances=ni)
                assert S.capture_status() == hs.CAPTURE_ACTIVE
            finally:
                graph = dm.graph_end()
            try:
                S.synchronize()
                assert (d_pal.buf.download((d_pal.nbytes + 2 * GUARD,), np.uint8) == SENT).all(), "recording ran something"
                state = sr.nan_state(ni, 3)
                for k, (ta, tb) in enumerate(times):
                    d_ta.upload(np.ascontiguousarray(ta, np.float64))
                    d_tb.upload(np.ascontiguousarray(tb, np.float64))
                    d_dt.upload(dts[k:k + 1])
                    d_hero.upload(hero_pals[k % 3])
                    graph.launch()
                    S.synchronize()
                    slab = d_slab.download((2, ni, 16), F)
                    rr.assert_same(slab, ps.sockets(hero_pals[k % 3], [7, 13], hero_rest[[7, 13]]), f"replay {k}: the heroes' heads and hands")
                    aimed = ar.aim(atable, solved[k], slab[0][:, 12:16])
                    reached = rr.reach(rtable, aimed, slab[1][:, 12:16])
                    assert aimed.tobytes() != solved[k].tobytes() and reached.tobytes() != aimed.tobytes()
                    wp, state = sr.step(stable, reached, state, dts[k])
                    rr.assert_same(d_pal.read(f"replay {k}"), wp, f"replay {k}: palettes")
                    if k in (0, 11, 39):
                        boxes = d_bnd.download((ni, 6), F)
                        rr.assert_same(boxes, pb.palette_bounds(dm.bone_boxes(), wp, 1.0, 1.0), f"replay {k}: boxes of the rewritten rows")
                rset.close()                                                 # took part in the recording
                with pytest.raises(api.MmdxError, match="destroyed"):
                    graph.launch()
            finally:
                graph.close()
        finally:
            dm.set_stream(None)
            hero.set_stream(None)
        _close(d_ca, d_cb, d_w, d_ta, d_tb, d_dt, d_place, d_pal, d_bnd, d_hero, d_slab, d_ids, fresh, aset, sset, sockets, sk, hero_sk, ms, bms,
               vs)

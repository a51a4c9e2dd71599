"""Look-at: mmdx_aim_set_* and mmdx_palette_aim (include/mmdx.h).

There is no libmmd counterpart (the reference has no look-at): as for the springs, the contract is the arithmetic the header states,
held by three statements that must agree bit for bit, with no tolerance anywhere (a NaN only has to be a NaN) --
  * csrc/aim_math.hpp and csrc/aim_table.hpp compiled for the host (tests/aim_math_driver.cpp, a stand-alone program, plain and
    sanitized),
  * the numpy restatement tests/aim_ref.py, written from the header's text,
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
from simple_mmd_renderer_amd.engine import AimSet, DeformModel, DeviceBuffer, SocketSet, SpringSet, device_count
from tests import aim_ref as ar
from tests import host_program as hp
from tests import palette_place_ref as pp
from tests import palette_sockets_ref as ps
from tests.test_capi_symbols import declared_symbols
from tests.test_palette_sockets import crowd_placements, rig_model, rig_small
from tests.test_spring_bones import GUARD, SENT, Guarded

ENTRY_POINTS = ("mmdx_aim_set_create", "mmdx_aim_set_destroy", "mmdx_aim_set_get_info", "mmdx_palette_aim")
ROOT = os.path.dirname(ar.HERE)
INVALID, BAD_INDEX, UNSUPPORTED = 1, 2, 6
F, U = np.float32, np.uint32
DEV = api.PALETTE_ON_DEVICE | api.OUT_ON_DEVICE
PLACE_DEV = DEV | api.PLACE_ON_DEVICE
# The worst case of the binary32 restatement, evaluated in binary64, over the case table and 3 000 steps of a target circling the
# swaying 41-bone rig, every set of the rig (test_tolerances_... prints the figures): the forward direction of a one-link aim against
# v 4.4e-7 per component, |R R^T - I| * m 3.7e-6 (m = 1 + cs of the link), the pivot 4.2e-7 relative to max(1, |H|).  The
# assertions take 4 x that, for inputs not seen.
TOL_DIR, TOL_ORTHO, TOL_PIVOT = 4 * 4.4e-7, 4 * 3.7e-6, 4 * 4.2e-7


@pytest.fixture(autouse=True)
def _lib(hip_lib):
    return hip_lib


def _close(*things):
    for t in things:
        for x in (t if isinstance(t, (list, tuple)) else [t]):
            (x.free if hasattr(x, "free") else x.close)()


# ---------------------------------------------------------------------------------------- CPU ----
def test_aim_entry_points_are_declared_exported_and_bound(hip_lib):
    syms = declared_symbols()
    for name in ENTRY_POINTS:
        assert name in syms and hasattr(hip_lib, name) and name in api.SIGNATURES, name
    hdr = open(os.path.join(ROOT, "include", "mmdx.h")).read()
    for text in ("typedef struct mmdx_aim_set_desc {", "typedef struct mmdx_aim_set_info {", "typedef struct mmdx_aim_args {",
                 "#define MMDX_ABI_VERSION 3u", "MMDX_AIM_TARGETS_ON_DEVICE = (1u << 18)", "#define MMDX_AIM_MAX_AIMS 16",
                 "#define MMDX_AIM_MAX_LINKS 4", "solve -> place -> aim -> springs -> palette", "Append and IK relations are not followed",
                 "The ids of one call must be distinct", "Sign and payload of a NaN are not part of the contract"):
        assert text in hdr, text
    assert hip_lib.mmdx_abi_version() == 3
    desc, info, args, tgt_dev, pal_dev, ma, ml = hp.c_values(
        ["sizeof(mmdx_aim_set_desc)", "sizeof(mmdx_aim_set_info)", "sizeof(mmdx_aim_args)", "MMDX_AIM_TARGETS_ON_DEVICE",
         "MMDX_PALETTE_ON_DEVICE", "MMDX_AIM_MAX_AIMS", "MMDX_AIM_MAX_LINKS"])
    assert C.sizeof(api.AimSetDesc) == desc == 2 * 4 + 6 * 8 + 4 + 4
    assert C.sizeof(api.AimSetInfo) == info == 6 * 4
    assert C.sizeof(api.AimArgs) == args == 4 * 4 + 3 * 8
    assert (api.AIM_TARGETS_ON_DEVICE, api.PALETTE_ON_DEVICE) == (tgt_dev, pal_dev) == (1 << 18, 1)
    assert (api.AIM_MAX_AIMS, api.AIM_MAX_LINKS, ar.MAX_AIMS, ar.MAX_LINKS) == (ma, ml, ma, ml) == (16, 4, 16, 4)
    others = hp.c_values(["MMDX_ANIM_DT_ON_DEVICE | MMDX_ROOT_NORMALIZE | MMDX_EVENTS_DOMINANT_SIDE | MMDX_BLEND_A_ON_DEVICE | "
                          "MMDX_BLEND_B_ON_DEVICE | MMDX_BLEND_PARAMS_ON_DEVICE | MMDX_PLACE_ON_DEVICE | MMDX_PLACE_MATRIX | "
                          "MMDX_SPRING_RESET | MMDX_SPRING_DT_ON_DEVICE | 0xFF"])[0]
    assert tgt_dev & others == 0                                           # a bit no other call accepts
    kernel_aim, = hp.c_values(["MMDX_DEBUG_KERNEL_AIM"], headers=("mmdx.h", "mmdx_bench.h"))
    assert api.DEBUG_KERNELS[kernel_aim] == "aim"
    for m in ("aim", "aim_raw", "info", "close"):
        assert callable(getattr(AimSet, m)), m
    poser = open(os.path.join(ROOT, "simple_mmd_renderer_amd", "host", "mmdx_poser.hpp")).read()
    for text in ("class AimSet", "mmdx_aim_set_create(", "mmdx_aim_set_destroy(", "mmdx_palette_aim("):
        assert text in poser, text


def test_case_table_contains_every_branch_the_header_names():
    """From the numpy side alone: what the driver and the kernel are about to be compared on."""
    case = ar.case_table()
    count = {}
    out = ar.aim(case["table"], case["pal"], case["targets"], count=count)
    missing = [k for k in ar.CASES if count.get(k, 0) < 1]
    assert not missing, (missing, count)
    assert [len(a["bone"]) for a in case["table"]] == [4, 2, 1, 1]
    assert np.isnan(out).any() and np.isfinite(out[:28]).all()             # the NaN link row of instance 28, and only there
    dead = [3, 4, 5, 6, 7]                                                 # weight 0, negative, NaN; a target that is not finite
    assert out[dead].tobytes() == case["pal"][dead].tobytes()


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_host_build_of_the_arithmetic_equals_the_numpy_restatement(sanitize):
    case = ar.case_table()
    want = ar.aim(case["table"], case["pal"], case["targets"])
    shared = case["targets"][1]                                            # one target for everyone (weight 0.5)
    want_shared = ar.aim(case["table"], case["pal"], shared)
    tb, got = ar.run_driver(ar.build_driver(sanitize), case["parent"], case["rest"], case["aims"],
                            [(case["pal"], case["targets"]), (case["pal"], shared)])
    for a, b in zip(tb, case["table"]):
        assert a["bone"].tolist() == b["bone"].tolist() and a["rows"] == b["rows"]
        ar.assert_same(a["h"], b["h"], "rest positions")
        ar.assert_same(a["sin_limit"], b["sin_limit"], "sin_limit")
    assert [len(a["rows"]) for a in tb] == [26, 3, 1, 2]
    ar.assert_same(got[0], want, "palettes")
    ar.assert_same(got[1], want_shared, "palettes, one target for everyone")
    for name, aims in ar.rig_sets().items():                               # the sets the GPU tests use, through the same two
        pal, tgt = ar.fk_palettes(case["parent"], case["rest"], 9, step=2), ar.circling_targets(9, 4)
        _, got = ar.run_driver(ar.build_driver(sanitize), case["parent"], case["rest"], aims, [(pal, tgt)])
        ar.assert_same(got[0], ar.aim(ar.build_table(case["parent"], case["rest"], aims), pal, tgt), name)


def _sweep():
    """The 3 000-step sweep as 3 000 instances of one call: a target circling the swaying 41-bone rig."""
    parent, rest = ar.aim_rig()
    n = 3000
    return parent, rest, ar.fk_palettes(parent, rest, n, step=1, amplitude=0.5), ar.circling_targets(n, 0)


def _errors(table, pal, targets):
    """(|R R^T - I| * m with m = 1 + cs of the link, pivot error relative to max(1, |H|)): the worst over every applied link of the
    binary32 restatement, evaluated in binary64.  (u and v2 are unit vectors to a rounding error d, and the formula turns that into
    4 d / m of non-orthogonality: the bound on R goes with 1 / m, as it does for the springs' step 7.)"""
    trace = []
    got = ar.aim(table, pal, targets, trace=trace)
    ortho = pivot = 0.0
    tgt = np.broadcast_to(np.asarray(targets, F).reshape(-1, 4), (pal.shape[0], 4))
    with np.errstate(all="ignore"):
        live = np.nonzero((tgt[:, 3] > 0) & ar.finite(tgt).all(axis=1))[0]
    it = iter(trace)
    for a in table:
        for l in range(len(a["bone"])):
            t = next(it)
            ok = t["applied"] & np.isfinite(t["r"]).all(axis=(1, 2)) & np.isfinite(t["hh"]).all(axis=1)
            if not ok.any():
                continue
            r = t["r"][ok].astype(np.float64)
            ortho = max(ortho, float((np.abs(r @ r.transpose(0, 2, 1) - np.eye(3)).max(axis=(1, 2)) * t["m"][ok]).max()))
            hh = t["hh"][ok].astype(np.float64)
            moved = ar.pt(a["h"][l].astype(np.float64), got[live][ok][:, a["bone"][l]].astype(np.float64))
            good = np.isfinite(moved).all(axis=1)
            pivot = max(pivot, float((np.abs(moved - hh).max(axis=1) / np.maximum(1.0, np.abs(hh).max(axis=1)))[good].max()))
    return ortho, pivot


def test_tolerances_a_single_link_points_at_the_target_and_rotations_are_rigid():
    """L = 1, share 1, no limit, the eye on the pivot: the new forward direction is v.  Every applied R is orthonormal to TOL_ORTHO / m
    and every link's pivot stays where it was -- over the case table and the sweep, every set of the rig."""
    parent, rest, pal, targets = _sweep()
    one = ar.build_table(parent, rest, [ar.make_aim([7], eye_point=rest[7], forward=(0.2, -0.1, -1.0))])
    out = ar.aim(one, pal, targets)
    v = ar.to_target(one[0], pal, targets)
    err_dir = float(np.abs(ar.forward_now(one[0], out) - v).max())
    assert np.abs(ar.forward_now(one[0], pal) - v).max() > 0.5             # (it was not there before)
    case = ar.case_table()
    figures = [_errors(case["table"], case["pal"], case["targets"])]
    for aims in ar.rig_sets().values():
        figures.append(_errors(ar.build_table(parent, rest, aims), pal, targets))
    ortho, pivot = (max(f[k] for f in figures) for k in range(2))
    print("direction %.3g, |R R^T - I| * m %.3g, pivot %.3g" % (err_dir, ortho, pivot))
    assert err_dir <= TOL_DIR and ortho <= TOL_ORTHO and pivot <= TOL_PIVOT, (err_dir, ortho, pivot)


def test_two_links_leave_a_smaller_angle_than_they_found():
    """Neck (share 0.5) and head (share 1), the eye in front of the head, no limits: the angle between the forward direction and the
    direction to the target is strictly smaller afterwards, for every step of the sweep; with the eye off the pivot it is not zero."""
    parent, rest, pal, targets = _sweep()
    table = ar.build_table(parent, rest, [ar.make_aim([6, 7], eye_bone=8, shares=[0.5, 1.0])])
    out = ar.aim(table, pal, targets)
    angle = lambda p: np.degrees(np.arccos(np.clip((ar.forward_now(table[0], p) * ar.to_target(table[0], p, targets)).sum(axis=1), -1, 1)))  # noqa: E731
    before, after = angle(pal), angle(out)
    print("angle before %.2f .. %.2f, after %.3g .. %.3g degrees" % (before.min(), before.max(), after.min(), after.max()))
    assert (after < before).all() and before.min() > 1.0 and after.max() < 0.5 * before.max()


def test_weight_fades_and_limit_caps_the_turn():
    """Weight w with share 1: the turn grows with w.  A limit of cos 0.9 on a single link: the forward direction ends within the
    limit of where it was (to TOL_DIR), and exactly on it where the target is further away."""
    parent, rest, pal, targets = _sweep()
    pal, targets = pal[:400], targets[:400]
    aim = ar.make_aim([7], eye_point=rest[7])
    table = ar.build_table(parent, rest, [aim])
    f0 = ar.forward_now(table[0], pal)
    turned = []
    for w in (0.25, 0.5, 1.0):
        t = targets.copy()
        t[:, 3] = w
        turned.append((f0 * ar.forward_now(table[0], ar.aim(table, pal, t))).sum(axis=1))
    assert (turned[0] > turned[1]).all() and (turned[1] > turned[2]).all()
    limited = ar.build_table(parent, rest, [ar.make_aim([7], eye_point=rest[7], cos_limits=[0.9])])
    cs = (f0 * ar.forward_now(limited[0], ar.aim(limited, pal, targets))).sum(axis=1)
    far = turned[2] < 0.9 - 1e-3
    assert far.sum() > 100 and np.abs(cs[far] - 0.9).max() <= TOL_DIR and (cs >= 0.9 - TOL_DIR).all()


def _skeleton(parent, rest):
    return vmd.Skeleton(rest, parent)


def _aim_set(sk, aims):
    """engine.AimSet from aims as ar.make_aim makes them (an eye point of None: the eye bone's rest position)."""
    return AimSet(sk, [{k: v for k, v in a.items() if v is not None} for a in aims])


def test_aim_set_create_refuses_what_the_header_lists_without_a_device(hip_lib):
    parent, rest = ar.aim_rig()
    sk = _skeleton(parent, rest)
    err = lambda: (hip_lib.mmdx_last_error_string() or b"").decode()          # noqa: E731
    out = C.c_void_p()
    keep = []

    def create(aims=None, struct_size=None, reserved0=0, skeleton=sk.h, null=(), n_aims=None, offsets=None):
        aims = [ar.make_aim([7])] if aims is None else aims
        arrays = ar.desc_arrays(aims, rest)
        if offsets is not None:
            arrays = (np.array(offsets, U),) + arrays[1:]
        keep.extend(arrays)
        d = api.AimSetDesc(C.sizeof(api.AimSetDesc) if struct_size is None else struct_size, len(aims) if n_aims is None else n_aims)
        d.link_offset, d.link_bone, d.link_params, d.eye_bone, d.eye_point, d.forward = (a.ctypes.data for a in arrays)
        d.reserved0 = reserved0
        for name in null:
            setattr(d, name, None)
        return hip_lib.mmdx_aim_set_create(skeleton, C.byref(d), C.byref(out))
    nan = float("nan")
    assert create(skeleton=None) == INVALID and "NULL" in err()
    assert hip_lib.mmdx_aim_set_create(sk.h, None, C.byref(out)) == INVALID and "NULL" in err()
    assert hip_lib.mmdx_aim_set_create(sk.h, None, None) == INVALID and "out_set" in err()
    assert create(struct_size=C.sizeof(api.AimSetDesc) - 8) == INVALID and "struct_size" in err()
    assert create(reserved0=1) == INVALID and "reserved0" in err()
    assert create(aims=[ar.make_aim([7, 41], eye_bone=7)]) == BAD_INDEX and "link_bone[1] = 41" in err()
    assert create(aims=[ar.make_aim([7], eye_bone=41, eye_point=(0, 0, 0))]) == BAD_INDEX and "eye_bone[0] = 41" in err()
    assert create(aims=[ar.make_aim([7, 5])]) == INVALID and "link_bone[1] = 5 is not a strict descendant" in err()      # upside down
    assert create(aims=[ar.make_aim([7, 7])]) == INVALID and "not a strict descendant" in err()
    assert create(aims=[ar.make_aim([10, 7])]) == INVALID and "not a strict descendant" in err()                         # a sibling branch
    assert create(aims=[ar.make_aim([5, 7], eye_bone=6)]) == INVALID and "eye_bone[0] = 6 is outside the subtree" in err()
    assert create(aims=[ar.make_aim([7], eye_bone=10)]) == INVALID and "outside the subtree" in err()
    assert create(n_aims=0) == INVALID and "n_aims = 0" in err()
    flat = _skeleton(np.array([-1] + [0] * 17, np.int32), np.zeros((18, 3), F))          # 17 leaves: 17 disjoint subtrees
    many = [ar.make_aim([b], eye_point=(0, 0, 0)) for b in range(1, 18)]
    assert create(aims=many, skeleton=flat.h) == INVALID and "n_aims = 17" in err()
    assert create(aims=many[:16], skeleton=flat.h) == api.OK
    hip_lib.mmdx_aim_set_destroy(out)
    flat.close()
    assert create(offsets=[0, 0]) == INVALID and "aim 0 has 0 links" in err()
    assert create(offsets=[1, 2]) == INVALID and "link_offset[0]" in err()
    assert create(aims=[ar.make_aim([3, 18, 19, 20]), ar.make_aim([24, 25, 26, 27, 28])]) == INVALID and "aim 1 has 5 links" in err()
    assert create(aims=[ar.make_aim([4, 5, 6, 7]), ar.make_aim([3, 18, 19, 20])]) == api.OK
    hip_lib.mmdx_aim_set_destroy(out)
    for share in (-0.001, 1.001, float("inf")):
        assert create(aims=[ar.make_aim([7], shares=[share])]) == INVALID and "share is outside [0, 1]" in err(), share
    for cl in (-1.001, 1.001, float("-inf")):
        assert create(aims=[ar.make_aim([7], cos_limits=[cl])]) == INVALID and "cos_limit is outside [-1, 1]" in err(), cl
    assert create(aims=[ar.make_aim([6, 7], shares=[0.5, nan])]) == INVALID and "link_params[1] holds a NaN" in err()
    assert create(aims=[ar.make_aim([6, 7], cos_limits=[nan, 0.5])]) == INVALID and "link_params[0] holds a NaN" in err()
    assert create(aims=[ar.make_aim([7], eye_point=(0, nan, 0))]) == INVALID and "NaN" in err()
    assert create(aims=[ar.make_aim([7], forward=(0, 0, nan))]) == INVALID and "NaN" in err()
    assert create(aims=[ar.make_aim([7], forward=(0, 0, 0))]) == INVALID and "forward of aim 0 is zero or not finite" in err()
    assert create(aims=[ar.make_aim([7], forward=(0, float("inf"), 0))]) == INVALID and "zero or not finite" in err()
    assert create(aims=[ar.make_aim([5]), ar.make_aim([7])]) == INVALID and "the subtrees of aim 0 and aim 1 intersect at bone 7" in err()
    assert create(aims=[ar.make_aim([8]), ar.make_aim([7])]) == INVALID and "intersect at bone 8" in err()
    assert create(aims=[ar.make_aim([8]), ar.make_aim([8])]) == INVALID and "intersect" in err()
    for name in ("link_offset", "link_bone", "link_params", "eye_bone", "eye_point", "forward"):
        assert create(null=(name,)) == INVALID and "NULL" in err(), name
    assert out.value is None                                               # a refusal hands out nothing
    # what is allowed: share 0 and 1, limits -1 and 1, an eye point anywhere; and the set reports itself
    s = AimSet(sk, [dict(links=[4, 5, 6, 7], eye_bone=8, shares=[0.0, 1.0, 0.5, 1.0], cos_limits=[-1.0, 1.0, 0.0, 0.5], eye_point=(1e6, 0, 0)),
                    dict(links=[2], eye_bone=39), dict(links=[40], forward=(0, 2, 0))])
    assert s.info() == dict(n_aims=3, n_links=6, n_subtree_rows=26 + 2 + 1, n_bones=41, device_ordinal=-1)
    info = api.AimSetInfo(8)
    assert hip_lib.mmdx_aim_set_get_info(s.h, C.byref(info)) == INVALID and "struct_size" in err()
    hip_lib.mmdx_aim_set_destroy(None)                                     # like free(NULL)
    sk.close()                                                             # the set copied what it needs
    assert s.info()["n_bones"] == 41
    s.close()


def test_palette_aim_refuses_bad_arguments_before_any_device_call(hip_lib):
    """Every call here carries its defect AND a host list with an id that is no instance behind it (or is refused ahead of any
    pointer being looked at), so none of them can reach a device."""
    parent, rest = ar.aim_rig()
    sk = _skeleton(parent, rest)
    s = AimSet(sk, [dict(links=[6, 7])])
    err = lambda: (hip_lib.mmdx_last_error_string() or b"").decode()          # noqa: E731
    tgt = np.zeros((4, 4), F)
    P = 0x10000                                                            # stands for a device address; never dereferenced
    ids = np.array([0, 9], U)
    ON = api.PALETTE_ON_DEVICE | api.AIM_TARGETS_ON_DEVICE

    def call(set_h=s.h, struct_size=None, flags=api.PALETTE_ON_DEVICE, ni=4, stride=4, palettes=P, targets=tgt.ctypes.data, select=None,
             null_args=False):
        a = api.AimArgs(C.sizeof(api.AimArgs) if struct_size is None else struct_size, flags, ni, stride, palettes, targets)
        if select is not None:
            a.select = C.pointer(select)
        return hip_lib.mmdx_palette_aim(set_h, None, None if null_args else C.byref(a))
    host_bad = vmd.instance_select(ids.ctypes.data, 2, None, on_device=False)          # id 9 >= 4: the refusal behind the others
    assert call(select=host_bad) == INVALID and "ids[1] = 9 is not below n_instances" in err()          # the guard itself
    assert call(flags=ON, targets=P, select=host_bad) == INVALID and "ids[1]" in err()
    assert call(set_h=None) == INVALID and "NULL" in err()
    assert call(null_args=True) == INVALID and "NULL" in err()
    assert call(struct_size=C.sizeof(api.AimArgs) - 8, select=host_bad) == INVALID and "struct_size" in err()
    for bad in (2, 4, 1 << 8, 1 << 10, 1 << 16, 1 << 17, 1 << 19, 1 << 31):
        assert call(flags=api.PALETTE_ON_DEVICE | bad, select=host_bad) == INVALID and "unknown flag bits" in err(), bad
    assert call(flags=api.AIM_TARGETS_ON_DEVICE, select=host_bad) == INVALID and "MMDX_PALETTE_ON_DEVICE" in err()
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
    """plan_aim_launch through the sanitized driver: 16 instances to a workgroup at every crowd size (the A/B found none at which 64
    is faster), MMDX_AIM_BLOCK = 64 forces 64 and any other value changes nothing; the workgroups cover the cells exactly once; LDS
    is block * (12 * L + 1) words, at most 12.25 KB."""
    cells = [1, 15, 16, 17, 63, 64, 65, 257, 1000, 4095, 4096, 4097, 16384, 100000, 1 << 23]
    rows = [(c, l, e) for c in cells for l in (1, 2, 3, 4) for e in (0, 16, 64, 32, -1, 128, 1)]
    got = ar.plan(*zip(*rows), ar.build_driver(True))
    assert len(got) == len(rows)
    for (c, l, e), (block, threads, nblocks, lds) in zip(rows, got):
        assert block == (64 if e == 64 else 16) and threads == 256, (c, l, e, block)
        assert (nblocks - 1) * block < c <= nblocks * block
        assert lds == block * (12 * l + 1) * 4 <= 12544


def test_kernel_resources_no_spills_no_scratch():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), api.LIB_PATH, "aim_kernel"],
                         capture_output=True, text=True, check=True).stdout.splitlines()
    names = {l.split(" vgpr ")[0].strip() for l in out}
    assert names == {"aim_kernel<true>", "aim_kernel<false>"}
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
    """The 41-bone rig, computed once and shared, never modified: palettes of 257 instances in model space and placed, targets for
    either, and per aim set of ar.rig_sets() its table."""
    if not _rig:
        parent, rest = ar.aim_rig()
        model_space = ar.fk_palettes(parent, rest, NI_MAX, step=5)
        place = crowd_placements(NI_MAX)
        placed = pp.place_crowd(model_space, place, False)
        local = ar.circling_targets(NI_MAX, 9)
        local[:, 3] = np.where(np.arange(NI_MAX) % 5 == 4, 0.4, 1.0)
        local[3::37, 3] = 0.0                                              # some instances do not look
        world = local.copy()
        world[:, 0] += place[:, 0]
        world[:, 2] += place[:, 2]
        _rig.update(parent=parent, rest=rest, nb=len(parent), sets=ar.rig_sets(),
                    tables={k: ar.build_table(parent, rest, v) for k, v in ar.rig_sets().items()},
                    pals={"model space": model_space, "placed": placed}, targets={"model space": local, "placed": world})
    return _rig


def big_model():
    """A model with the rig's 41 bones (the calls take a stream and, for the sockets, a bone count from it)."""
    return DeformModel(synth.make_model(64, 41, 0, 0, seed=31))


def _shape(dm):
    s = dm.last_launch_shape()
    return s["kernel"], s["threads"], s["group"], s["ngroups"], s["lds"], s["select"]


@pytest.mark.gpu
@pytest.mark.parametrize("block", [16, 64])
@pytest.mark.parametrize("ni", [1, 15, 16, 17, 63, 64, 65, 257])
def test_gpu_rows_equal_the_restatement(gpu, monkeypatch, ni, block):
    """Every set of the rig (1, 2 and 4 links; 1 and 3 aims; subtrees of 1, 2, 3, 11, 25, 26 and 37 rows, so that phase B's item count is no
    multiple of 256), model space and placed, targets every 4 floats, one target for everyone and a real sockets slab at stride 16:
    the whole palette array between its sentinels equals the restatement's, byte for byte, and the debug record proves the block."""
    r = rig()
    nb = r["nb"]
    monkeypatch.setenv("MMDX_AIM_BLOCK", str(block))
    with big_model() as dm:
        sk = _skeleton(r["parent"], r["rest"])
        d_pal = Guarded(ni, nb, dm)
        sockets = SocketSet.from_skeleton(dm, sk, [0, 7, 40])
        d_hero, d_slab = DeviceBuffer.from_numpy(np.roll(r["pals"]["placed"][:ni], 1, axis=0)), DeviceBuffer(3 * ni * 64)
        sockets.sockets(d_hero, d_slab, n_instances=ni)
        dm.sync()
        slab = d_slab.download((3, ni, 16), F)[1]                           # where each instance's neighbour's head is
        assert (slab[:, 15] == 1.0).all()
        for name, aims in r["sets"].items():
            aset = _aim_set(sk, aims)
            table = r["tables"][name]
            assert aset.info()["n_subtree_rows"] == sum(len(a["rows"]) for a in table)
            max_links = max(len(a["bone"]) for a in table)
            for space in ("model space", "placed"):
                src, tgt = r["pals"][space][:ni], r["targets"][space][:ni]
                d_tgt = DeviceBuffer.from_numpy(tgt)
                plans = [("stride 4", d_tgt.ptr, 4, tgt), ("one target", d_tgt.ptr + 16 * (ni // 2), 0, tgt[ni // 2]),
                         ("host targets", tgt, None, tgt)]
                if space == "placed":
                    plans.append(("sockets slab", d_slab.ptr + ni * 64 + 48, 16, slab[:, 12:16]))
                for what, ptr, stride, want_tgt in plans:
                    what = f"{name}, NI {ni}, block {block}, {space}, {what}"
                    d_pal.upload(src)
                    if stride is None:
                        aset.aim(dm, d_pal, ptr, n_instances=ni)
                    else:
                        aset.aim(dm, d_pal, ptr, stride=stride, n_instances=ni)
                    assert _shape(dm) == ("aim", 256, block, (ni + block - 1) // block, block * (12 * max_links + 1) * 4, 0), what
                    want = ar.aim(table, src, want_tgt)
                    got = d_pal.read(what)
                    ar.assert_same(got, want, what)
                    outside = np.ones(nb, bool)
                    outside[[b for a in table for b, _ in a["rows"]]] = False
                    assert got[:, outside].tobytes() == src[:, outside].tobytes(), what + ": a row outside the subtrees changed"
                    assert ni == 1 or want.tobytes() != src.tobytes()      # (alone, an instance is its own neighbour: the target is on its eye)
                d_tgt.free()
            assert aset.info()["device_ordinal"] >= 0
            aset.close()
        _close(d_pal, d_hero, d_slab, sockets, sk)
    monkeypatch.delenv("MMDX_AIM_BLOCK")


@pytest.mark.gpu
def test_gpu_default_block_is_16_and_a_nan_row_stays_with_its_instance(gpu, monkeypatch):
    """Without MMDX_AIM_BLOCK 65 instances take 16 to a workgroup.  A NaN in a link row of instance 20 and an infinite target of
    instance 21: their neighbours, in the same workgroup, stay exact, instance 21 keeps every byte."""
    monkeypatch.delenv("MMDX_AIM_BLOCK", raising=False)
    r = rig()
    ni, nb, table = 65, r["nb"], r["tables"]["mixed"]
    src, tgt = r["pals"]["placed"][:ni].copy(), r["targets"]["placed"][:ni].copy()
    src[20, 5, 6] = np.nan
    tgt[21, 1] = np.inf
    with big_model() as dm:
        sk = _skeleton(r["parent"], r["rest"])
        aset = _aim_set(sk, r["sets"]["mixed"])
        d_pal, d_tgt = Guarded(ni, nb, dm), DeviceBuffer.from_numpy(tgt)
        d_pal.upload(src)
        aset.aim(dm, d_pal, d_tgt, n_instances=ni)
        assert _shape(dm) == ("aim", 256, 16, 5, 16 * 49 * 4, 0)
        got, want = d_pal.read("a NaN row"), ar.aim(table, src, tgt)
        ar.assert_same(got, want, "a NaN row")
        assert np.isnan(got[20]).any() and np.isfinite(np.delete(got, 20, axis=0)).all()
        assert got[21].tobytes() == src[21].tobytes()
        _close(d_pal, d_tgt, aset, sk)


@pytest.mark.gpu
@pytest.mark.parametrize("block", [16, 64])
def test_gpu_case_table_through_the_kernel(gpu, monkeypatch, block):
    """The 32 instances of the case table -- every branch of steps 0-2, two workgroups per aim at 16 -- equal the restatement."""
    monkeypatch.setenv("MMDX_AIM_BLOCK", str(block))
    case = ar.case_table()
    ni, nb = case["pal"].shape[:2]
    with big_model() as dm:
        sk = _skeleton(case["parent"], case["rest"])
        aset = _aim_set(sk, case["aims"])
        d_pal, d_tgt = Guarded(ni, nb, dm), DeviceBuffer.from_numpy(case["targets"])
        d_pal.upload(case["pal"])
        aset.aim(dm, d_pal, d_tgt, n_instances=ni)
        ar.assert_same(d_pal.read("the case table"), ar.aim(case["table"], case["pal"], case["targets"]), "the case table")
        _close(d_pal, d_tgt, aset, sk)


SEL_IDS = np.array([3, 64, 0, 7, 33, 1, 12, 40, 16, 17, 63, 21, 22, 23, 24, 25, 26, 27], U)
SEL_IDS_DEV = np.array([3, 64, 0, 70, 7, 0xFFFFFFFF, 12, 40, 16, 17, 63, 21, 22, 23, 24, 25, 26, 27], U)     # 70 and 2^32-1: no instances of 65


@pytest.mark.gpu
@pytest.mark.parametrize("where", ["host list", "device list"])
def test_gpu_select_aims_the_listed_instances_only(gpu, monkeypatch, where):
    """65 instances, the 3-aim set, placed palettes, 18 list positions (two workgroups of 16).  Lists with count NULL, 0, 5, 17 and
    100: listed instances get the restatement's rows -- by their own target, not the list position's --, unlisted ones keep every
    byte; a list of capacity 0; a host id that is no instance."""
    monkeypatch.setenv("MMDX_AIM_BLOCK", "16")
    ni = 65
    r = rig()
    nb, table = r["nb"], r["tables"]["mixed"]
    src, tgt = r["pals"]["placed"][:ni], r["targets"]["placed"][:ni]
    with big_model() as dm:
        sk = _skeleton(r["parent"], r["rest"])
        aset = _aim_set(sk, r["sets"]["mixed"])
        d_pal, d_tgt = Guarded(ni, nb, dm), DeviceBuffer.from_numpy(tgt)
        ids = SEL_IDS if where == "host list" else SEL_IDS_DEV
        d_ids, d_cnt = DeviceBuffer.from_numpy(ids), DeviceBuffer(4)
        for count in (None, 0, 5, 17, 100):
            what = f"{where}, count {count}"
            if where == "host list":
                cnt = C.c_uint32(count or 0)
                sel = vmd.instance_select(ids.ctypes.data, ids.size, C.addressof(cnt) if count is not None else None, on_device=False)
            else:
                d_cnt.upload(np.array([count or 0], U))
                sel = vmd.instance_select(d_ids.ptr, ids.size, d_cnt.ptr if count is not None else None)
            d_pal.upload(src)
            aset.aim(dm, d_pal, d_tgt, select=sel, n_instances=ni)
            used = [int(i) for i in (ids if count is None else ids[:min(count, ids.size)]) if i < ni]
            want = ar.aim(table, src, tgt, ids=used)
            unlisted = np.ones(ni, bool)
            unlisted[used] = False
            assert want[unlisted].tobytes() == src[unlisted].tobytes() and (not used or want.tobytes() != src.tobytes())
            ar.assert_same(d_pal.read(what), want, what)
            if used:
                cells = ids.size if where == "device list" else len(used)
                assert _shape(dm) == ("aim", 256, 16, (cells + 15) // 16, 16 * 49 * 4, 1), what
        d_pal.upload(src)
        aset.aim(dm, d_pal, d_tgt, select=vmd.instance_select(d_ids.ptr, 0), n_instances=ni)
        assert d_pal.read("n_ids 0").tobytes() == src.tobytes()
        bad = np.array([1, 65], U)
        with pytest.raises(api.MmdxError, match="is not below n_instances"):
            aset.aim(dm, d_pal, d_tgt, select=vmd.instance_select(bad.ctypes.data, 2, None, on_device=False), n_instances=ni)
        assert d_pal.read("after the refusal").tobytes() == src.tobytes()
        _close(d_pal, d_tgt, d_ids, d_cnt, aset, sk)


@pytest.mark.gpu
def test_gpu_recorded_frame_replayed_40_times_on_a_borrowed_stream(gpu, monkeypatch):
    """[blend solve, place, sockets of a second model, aim, spring step, palette bounds] recorded once on a stream of the test's that
    both models borrow, replayed 40 times with the clip times, the hero's palettes and dt rewritten in device memory: after every
    replay the palettes equal the restatements' aim and spring step on the palettes solve and place give for those times, with the
    targets the sockets call wrote.  The aim's subtree holds the spring chains and their anchor: the springs read what aim wrote.
    Host targets, a host list and a fresh set are refused while recording."""
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
    table = ar.build_table(parent, rest, aims)
    assert sorted(b for b, _ in table[0]["rows"]) == [3, 7, 9, 10, 13, 16, 17, 18]
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
    hero_place = np.roll(crowd_placements(ni), 3, axis=0)                   # everybody watches somebody else's head
    hero_pals = [pp.place_crowd(ar.fk_palettes(hero_parent, hero_rest, ni, step=11 * k), hero_place, False) for k in range(3)]
    with rig_model() as dm, big_model() as hero, hs.Stream() as S:
        sk = vmd.Skeleton(rest, parent, z["level"], z["flags"])
        hero_sk = _skeleton(hero_parent, hero_rest)
        aset = AimSet(sk, [dict(links=[3, 7], eye_bone=16, shares=[0.5, 1.0], cos_limits=[0.7, 0.2], forward=(0.0, 0.3, -1.0))])
        sset = SpringSet(sk, chains, params, ni)
        sockets = SocketSet.from_skeleton(hero, hero_sk, [7])
        d_ca, d_cb, d_w = DeviceBuffer.from_numpy(ca), DeviceBuffer.from_numpy(cb), DeviceBuffer.from_numpy(w)
        d_ta, d_tb, d_dt = DeviceBuffer(ni * 8), DeviceBuffer(ni * 8), DeviceBuffer(4)
        d_place, d_pal, d_bnd = DeviceBuffer.from_numpy(crowd_placements(ni)), Guarded(ni, nb, dm), DeviceBuffer(ni * 24)
        d_hero, d_slab = DeviceBuffer(ni * 41 * 64), DeviceBuffer(ni * 64)
        d_ids = DeviceBuffer.from_numpy(np.arange(ni, dtype=U))

        def solve_place():
            sk.solve_motion_set_blend_time_device(ms, ni, d_ca.ptr, d_ta.ptr, d_cb.ptr, d_tb.ptr, d_w.ptr, d_pal.ptr, dm)
            dm.place_palettes(ni, d_pal.ptr, d_place.ptr, d_pal.ptr, PLACE_DEV)

        def frame():
            solve_place()
            sockets.sockets(d_hero, d_slab, n_instances=ni)
            aset.aim(dm, d_pal, d_slab.ptr + 48, stride=16, select=vmd.instance_select(d_ids.ptr, ni), n_instances=ni)
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
            fresh = AimSet(sk, [dict(links=[7])])                             # never ran on the device
            frame()                                                           # the run before recording: the sets go to the device
            S.synchronize()
            sset.set_state(sr.nan_state(ni, 3), dm)
            d_pal.buf.memset(SENT)
            dm.graph_begin()
            try:
                assert S.capture_status() == hs.CAPTURE_ACTIVE
                frame()
                with pytest.raises(api.MmdxError, match="targets must be in device memory"):
                    aset.aim(dm, d_pal, np.zeros((ni, 4), F), n_instances=ni)
                host_ids = np.arange(3, dtype=U)
                with pytest.raises(api.MmdxError, match="instance list must be in device memory"):
                    aset.aim(dm, d_pal, d_slab.ptr + 48, stride=16, n_instances=ni,
                             select=vmd.instance_select(host_ids.ctypes.data, 3, None, on_device=False))
                with pytest.raises(api.MmdxError, match="must have run on this device before"):
                    fresh.aim(dm, d_pal, d_slab.ptr + 48, stride=16, n_instances=ni)
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
                    heads = d_slab.download((ni, 16), F)
                    ar.assert_same(heads, ps.sockets(hero_pals[k % 3], [7], hero_rest[[7]])[0], f"replay {k}: the heroes' heads")
                    aimed = ar.aim(table, solved[k], heads[:, 12:16])
                    assert aimed.tobytes() != solved[k].tobytes()
                    wp, state = sr.step(stable, aimed, state, dts[k])
                    ar.assert_same(d_pal.read(f"replay {k}"), wp, f"replay {k}: palettes")
                    if k in (0, 11, 39):
                        boxes = d_bnd.download((ni, 6), F)
                        ar.assert_same(boxes, pb.palette_bounds(dm.bone_boxes(), wp, 1.0, 1.0), f"replay {k}: boxes of the rewritten rows")
                aset.close()                                                 # took part in the recording
                with pytest.raises(api.MmdxError, match="destroyed"):
                    graph.launch()
            finally:
                graph.close()
        finally:
            dm.set_stream(None)
            hero.set_stream(None)
        _close(d_ca, d_cb, d_w, d_ta, d_tb, d_dt, d_place, d_pal, d_bnd, d_hero, d_slab, d_ids, fresh, sset, sockets, sk, hero_sk, ms, bms, vs)

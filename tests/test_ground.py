"""Ground: mmdx_ground_create / _destroy / _get_info, mmdx_ground_place and mmdx_ground_targets (include/mmdx.h).

There is no libmmd counterpart (the reference has no terrain): as for the springs, the aim and the reach, the contract is the
arithmetic the header states, held by three statements that must agree bit for bit, with no tolerance anywhere (a NaN only has to be
a NaN) --
  * csrc/ground_math.hpp and csrc/ground_table.hpp compiled for the host (tests/ground_math_driver.cpp, a stand-alone program, plain
    and sanitized),
  * the numpy restatement tests/ground_ref.py, written from the header's text,
  * the gfx950 kernels (the same header compiled for the device),
and the properties of h(x, z) are asserted on the restatement, on the CPU: exactly where the arithmetic is exact, within a tolerance
measured against a binary64 evaluation of the same formulas where it is not.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from simple_mmd_renderer_amd import _capi as api
from simple_mmd_renderer_amd import synth, vmd
from simple_mmd_renderer_amd.engine import DeformModel, DeviceBuffer, Ground, ReachSet, SocketSet, SpringSet, device_count
from tests import ground_ref as gr
from tests import host_program as hp
from tests import palette_place_ref as pp
from tests import palette_sockets_ref as ps
from tests.test_capi_symbols import declared_symbols

ENTRY_POINTS = ("mmdx_ground_create", "mmdx_ground_destroy", "mmdx_ground_get_info", "mmdx_ground_place", "mmdx_ground_targets")
ROOT = os.path.dirname(gr.HERE)
INVALID, NO_DEVICE, UNSUPPORTED = 1, 3, 6
F, U = np.float32, np.uint32
DEV = api.PALETTE_ON_DEVICE | api.OUT_ON_DEVICE
PLACE_DEV = DEV | api.PLACE_ON_DEVICE
# |h - h64| relative to max(1, max|H|): the worst of the binary32 restatement against the same formulas in binary64 over 200 000
# random points in and around each field of gr.fields() is 5.7e-7 (test_tolerance_... prints the figure); the header carries it
# rounded up as MMDX_GROUND_H_ERROR, the assertions take four times that, for points not seen.
H_ERROR = 6e-7
TOL = 4 * H_ERROR
GUARD, SENT = 256, 0xEE


@pytest.fixture(autouse=True)
def _lib(hip_lib):
    return hip_lib


def _close(*things):
    for t in things:
        for x in (t if isinstance(t, (list, tuple)) else [t]):
            (x.free if hasattr(x, "free") else x.close)()


def _ground(field):
    return Ground(field["H"], tuple(float(v) for v in field["origin"]), tuple(float(v) for v in field["cell"]))


# ---------------------------------------------------------------------------------------- CPU ----
def test_ground_entry_points_are_declared_exported_and_bound(hip_lib):
    syms = declared_symbols()
    for name in ENTRY_POINTS:
        assert name in syms and hasattr(hip_lib, name) and name in api.SIGNATURES, name
    hdr = open(os.path.join(ROOT, "include", "mmdx.h")).read()
    for text in ("typedef struct mmdx_ground_desc {", "typedef struct mmdx_ground_info {", "typedef struct mmdx_ground_place_args {",
                 "typedef struct mmdx_ground_targets_args {", "#define MMDX_ABI_VERSION 3u", "#define MMDX_GROUND_MAX_FEET 8",
                 "#define MMDX_GROUND_MAX_SAMPLES 8192", "#define MMDX_GROUND_H_ERROR 6e-7f",
                 "h = (h00*((1.0f - fu) - fv) + h10*fu) + h01*fv", "h = (h11*((fu + fv) - 1.0f) + h10*(1.0f - fv)) + h01*(1.0f - fu)",
                 "root motion -> GROUND PLACE -> tracks -> solve -> place -> sockets -> GROUND TARGETS -> aim -> reach",
                 "come from mmdx_ground_targets (the ground section below)"):
        assert text in hdr, text
    assert "ground\n *    queries are out of scope" not in hdr
    assert hip_lib.mmdx_abi_version() == 3
    desc, info, pa, ta, feet, lo, hi, pose = hp.c_values(
        ["sizeof(mmdx_ground_desc)", "sizeof(mmdx_ground_info)", "sizeof(mmdx_ground_place_args)", "sizeof(mmdx_ground_targets_args)",
         "MMDX_GROUND_MAX_FEET", "MMDX_GROUND_MIN_SAMPLES", "MMDX_GROUND_MAX_SAMPLES", "MMDX_POSE_FLOATS"])
    assert C.sizeof(api.GroundDesc) == desc == 8 * 4 + 8 + 8
    assert C.sizeof(api.GroundInfo) == info == 11 * 4
    assert C.sizeof(api.GroundPlaceArgs) == pa == 4 * 4 + 3 * 8
    assert C.sizeof(api.GroundTargetsArgs) == ta == 4 * 4 + 2 * 8 + 2 * 4 + 2 * 8 + 2 * 4 + 8
    assert (api.GROUND_MAX_FEET, gr.MAX_FEET) == (feet, feet) == (8, 8) and (gr.MIN_SAMPLES, gr.MAX_SAMPLES) == (lo, hi) == (2, 8192)
    assert pose == 8 and api.GROUND_H_ERROR == H_ERROR
    for m in ("place", "targets", "info", "close", "__enter__", "__exit__"):
        assert callable(getattr(Ground, m)), m
    poser = open(os.path.join(ROOT, "simple_mmd_renderer_amd", "host", "mmdx_poser.hpp")).read()
    for text in ("class Ground", "mmdx_ground_create(", "mmdx_ground_destroy(", "mmdx_ground_place(", "mmdx_ground_targets("):
        assert text in poser, text


def test_case_table_contains_every_branch_the_header_names():
    """From the numpy side alone: what the driver and the kernels are about to be compared on."""
    count, per_field = {}, {}
    for name, case in gr.case_table().items():
        per_field[name] = {}
        got = gr.run_calls(case, per_field[name])
        for k, v in per_field[name].items():
            count[k] = count.get(k, 0) + v
        f = case["field"]
        assert (f["nx"], f["nz"]) == dict([("2x2", (2, 2)), ("3x2", (3, 2)), ("33x17", (33, 17))])[name]
        assert f["cell"][0] != f["cell"][1] and f["origin"][0] < 0 and f["origin"][1] < 0
        pl, calls = case["placements"], case["calls"]
        placed = [g[0] for g, c in zip(got, calls) if c["kind"] == "place"]
        for p in placed:                                                    # only [i][1] is ever written; a refused instance keeps it
            assert np.delete(p, 1, axis=1).tobytes() == np.delete(pl, 1, axis=1).tobytes()
            assert p[:5, 1].tobytes() == pl[:5, 1].tobytes() and (p[24:, 1] != pl[24:, 1]).all()
        assert placed[0][8:11, 1].tobytes() == pl[8:11, 1].tobytes() and (placed[1][8:11, 1] != pl[8:11, 1]).all()      # the drop's NaN, inf
        for (tgt, drop), c in ((g, c) for g, c in zip(got, calls) if c["kind"] == "targets"):
            zero = np.zeros(4, F).tobytes()
            assert all(tgt[0, i].tobytes() == zero for i in (5, 6, 7, 11, 12, 13, 15, 17, 19))      # ty, every foot, foot 0: +0 four times
            assert (tgt[0, 24:, 3] == 1.0).all() and (tgt[0, 24:, 0] == case["points"][0, 24:, 0]).all()
            if c["max_step"] == 0.0:
                assert (tgt[0, 24:, 1] == case["points"][0, 24:, 1]).all()      # the animated height, untouched
            if drop is not None:
                assert (drop <= 0).all() and (drop >= -F(c["max_drop"])).all()
                assert (drop[:5] == 0).all() and (drop[11:13] == 0).all()     # h0 fails; no foot sampled
    missing = [k for k in gr.CASES if count.get(k, 0) < 1]
    assert not missing, (missing, count)
    for name in per_field:                                                  # both triangles and the clamp in every field
        assert all(per_field[name].get(k, 0) > 0 for k in ("lower", "upper", "diagonal", "outside -x", "outside +x+z", "last cell fu 1")), name


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_host_build_of_the_arithmetic_equals_the_numpy_restatement(sanitize):
    exe = gr.build_driver(sanitize)
    for name, case in gr.case_table().items():
        want = gr.run_calls(case)
        lo_hi, got = gr.run_driver(exe, case)
        assert lo_hi.tolist() == [case["field"]["H"].min(), case["field"]["H"].max()]
        changed = False
        for c, w, g in zip(case["calls"], want, got):
            for a, b in zip(w, g):
                assert (a is None) == (b is None)
                if a is not None:
                    gr.assert_same(b, a, f"{name}, {c}")
            changed = changed or (c["kind"] == "place" and w[0].tobytes() != case["placements"].tobytes())
        assert changed


def test_planner_swept_on_the_cpu():
    """plan_ground_launch through the sanitized driver: one wave of 64 lanes = 64 instances to a workgroup at every crowd size; the
    workgroups cover the cells exactly once."""
    cells = [1, 2, 63, 64, 65, 127, 128, 129, 257, 1000, 4095, 4096, 4097, 16384, 100000, (1 << 23) - 1, 1 << 23]
    got = gr.plan(cells, gr.build_driver(True))
    assert len(got) == len(cells)
    for c, (threads, nblocks) in zip(cells, got):
        assert threads == gr.THREADS == 64
        assert (nblocks - 1) * threads < c <= nblocks * threads


def _unit_field(heights):
    return gr.make_field(heights, (0.0, 0.0), (1.0, 1.0))


def test_exact_h_equals_the_stored_height_at_every_sample():
    """Origin 0, cell 1, so u and v are exact: at every sample of the 33 x 17 field -- reached as the first corner of its cell, and in
    the last row and column as fu == 1 / fv == 1 of the clamped cell -- h is the stored height, up to the sign of a zero; and so it
    is beyond the border, where the field continues flat."""
    H = gr.hills(33, 17, 3)
    H[4, 5], H[0, 0], H[16, 32] = 0.0, -0.0, 0.0
    f = _unit_field(H)
    x, z = np.meshgrid(np.arange(33, dtype=F), np.arange(17, dtype=F))
    ok, h = gr.height(f, x, z)
    assert ok.all() and (h == H).all() and h.dtype == F
    ok, h = gr.height(f, np.array([-3.0, 40.0, -3.0, 40.0, 7.0, 7.0], F), np.array([-2.0, -2.0, 99.0, 99.0, -1.0, 50.0], F))
    assert ok.all() and h.tolist() == [H[0, 0], H[0, 32], H[16, 0], H[16, 32], H[0, 7], H[16, 7]]
    ok, h = gr.height(f, np.array([np.nan, 1.0, np.inf, 1.0], F), np.array([1.0, np.nan, 1.0, -np.inf], F))
    assert not ok.any()


def test_exact_h_on_a_plane_is_the_plane():
    """Heights of a*x + b*z + c with small-integer coefficients on a unit grid: every product and sum of the barycentric form is
    exact for fractions that are multiples of 1/64, so h is the plane exactly, in both triangles and on the diagonal."""
    x, z = np.meshgrid(np.arange(33, dtype=np.float64), np.arange(17, dtype=np.float64))
    rng = np.random.RandomState(9)
    for a, b, c in ((3, -2, 5), (-7, 4, 0), (0, 0, -6), (1, 1, 1), (-5, -3, 11)):
        f = _unit_field(a * x + b * z + c)
        px = rng.randint(0, 32 * 64 + 1, 4000) / 64.0
        pz = rng.randint(0, 16 * 64 + 1, 4000) / 64.0
        count = {}
        ok, h = gr.height(f, px.astype(F), pz.astype(F), count=count)
        assert ok.all() and (h.astype(np.float64) == a * px + b * pz + c).all(), (a, b, c)
        assert count["lower"] > 500 and count["upper"] > 500 and count["diagonal"] > 5


def test_exact_place_then_targets_on_a_flat_field_returns_every_foot():
    """A flat field at 2.5 on the unit grid, positions at multiples of 1/64 in and around it (so the three barycentric weights and
    their products with 2.5 are exact): place puts every placement on 2.5 exactly, and targets with that placement returns each
    foot's own point, bit for bit, with weight 1 and a drop of +0; with a y_offset the feet move by -y_offset."""
    f = _unit_field(np.full((5, 4), 2.5, F))
    rng = np.random.RandomState(4)
    ni = 300
    pl = rng.uniform(-1, 1, (ni, 8)).astype(F)
    pl[:, 0], pl[:, 2] = rng.randint(-128, 6 * 64, ni) / 64.0, rng.randint(-128, 7 * 64, ni) / 64.0
    pts = np.ones((3, ni, 4), F)
    pts[:, :, 0], pts[:, :, 2] = rng.randint(-128, 6 * 64, (3, ni)) / 64.0, rng.randint(-128, 7 * 64, (3, ni)) / 64.0
    pts[:, :, 1] = rng.uniform(0, 5, (3, ni))
    for y_offset in (0.0, 0.25):
        stood = gr.place(f, pl, None, y_offset)
        assert (stood[:, 1] == F(2.5) + F(y_offset)).all() and np.delete(stood, 1, axis=1).tobytes() == np.delete(pl, 1, axis=1).tobytes()
        tgt, drop = gr.targets(f, stood, pts, max_step=10.0, max_drop=10.0)
        assert (drop == 0).all() and not np.signbit(drop).any()
        if y_offset == 0.0:
            assert tgt.tobytes() == pts.tobytes()
        else:
            assert (tgt[:, :, 3] == 1).all() and (tgt[:, :, [0, 2]] == pts[:, :, [0, 2]]).all()
            assert (tgt[:, :, 1] == pts[:, :, 1] + F(-0.25)).all()


def _random_points(field, n, seed):
    rng = np.random.RandomState(seed)
    uv = rng.uniform((-2.0, -2.0), (field["nx"] + 1.0, field["nz"] + 1.0), (n, 2))
    x = np.float64(field["origin"][0]) + uv[:, 0] * np.float64(field["cell"][0])
    z = np.float64(field["origin"][1]) + uv[:, 1] * np.float64(field["cell"][1])
    return x.astype(F), z.astype(F)


def test_tolerance_h_against_binary64_and_continuity_across_diagonal_and_edges():
    """h in binary32 against the same formulas in binary64 from the same x and z, 200 000 random points in and around each field,
    relative to max(1, max|H|); then continuity: points on the diagonals and on the cell edges of the 33 x 17 field (dyadic cells:
    they lie there exactly), stepped 1, 2 and 5 ulps to either side in x and in z -- what h changes by across the seam is what the
    binary64 surface changes by, to the same bound."""
    worst = 0.0
    for name, f in gr.fields().items():
        x, z = _random_points(f, 200000, 5)
        ok, h = gr.height(f, x, z)
        ok8, h8 = gr.height(f, x, z, ft=np.float64)
        assert ok.all() and ok8.all()
        scale = max(1.0, float(np.abs(f["H"]).max()))
        worst = max(worst, float(np.abs(h - h8).max()) / scale)
    print("worst |h - h64| / max(1, max|H|) = %.3g" % worst)
    assert worst <= TOL, (worst, TOL)
    f = gr.fields()["33x17"]
    scale = max(1.0, float(np.abs(f["H"]).max()))
    rng = np.random.RandomState(6)
    iu, iv = rng.randint(0, 32, 3000), rng.randint(0, 16, 3000)
    t = rng.randint(1, 64, 3000) / 64.0
    seams = {"diagonal": (iu + t, iv + (1 - t)), "edge in x": (iu + 0.0, iv + t), "edge in z": (iu + t, iv + 0.0)}
    jump = 0.0
    for what, (u, v) in seams.items():
        x = (np.float64(f["origin"][0]) + u * np.float64(f["cell"][0])).astype(F)
        z = (np.float64(f["origin"][1]) + v * np.float64(f["cell"][1])).astype(F)
        count = {}
        gr.height(f, x, z, count=count)
        assert count.get({"diagonal": "diagonal", "edge in x": "edge fu 0", "edge in z": "edge fv 0"}[what], 0) >= 2900, (what, count)
        for ulps in (1, 2, 5):
            for axis in (0, 1):
                lo, hi = [x.copy(), z.copy()], [x.copy(), z.copy()]
                for _ in range(ulps):
                    lo[axis], hi[axis] = np.nextafter(lo[axis], F(-np.inf)), np.nextafter(hi[axis], F(np.inf))
                (_, a), (_, b) = gr.height(f, *lo), gr.height(f, *hi)
                (_, a8), (_, b8) = gr.height(f, *lo, ft=np.float64), gr.height(f, *hi, ft=np.float64)
                excess = float(np.max(np.abs(b.astype(np.float64) - a) - np.abs(b8 - a8))) / scale
                jump = max(jump, excess)
                assert excess <= TOL, (what, ulps, axis, excess)
    print("worst jump across a seam beyond the binary64 surface's = %.3g" % jump)


def test_ground_create_refuses_what_the_header_lists_without_a_device(hip_lib):
    err = lambda: (hip_lib.mmdx_last_error_string() or b"").decode()          # noqa: E731
    out = C.c_void_p()
    keep = []

    def create(heights=None, nx=3, nz=2, origin=(0.0, 0.0), cell=(1.0, 1.0), struct_size=None, flags=0, reserved0=0, null=False):
        h = np.ascontiguousarray(np.zeros((nz, nx), F) if heights is None else heights, F)
        keep.append(h)
        d = api.GroundDesc(C.sizeof(api.GroundDesc) if struct_size is None else struct_size, flags, nx, nz, origin[0], origin[1], cell[0], cell[1],
                           None if null else h.ctypes.data, reserved0)
        return hip_lib.mmdx_ground_create(C.byref(d), C.byref(out))
    nan, inf = float("nan"), float("inf")
    assert hip_lib.mmdx_ground_create(None, C.byref(out)) == INVALID and "NULL" in err()
    assert hip_lib.mmdx_ground_create(None, None) == INVALID and "out_ground" in err()
    assert create(null=True) == INVALID and "heights is NULL" in err()
    assert create(struct_size=C.sizeof(api.GroundDesc) - 8) == INVALID and "struct_size" in err()
    assert create(reserved0=1) == INVALID and "reserved0" in err()
    for flags in (1, 2, 1 << 20, 1 << 31):
        assert create(flags=flags) == INVALID and "unknown flag bits" in err(), flags
    tiny = np.zeros((2, 2), F)
    for nx, nz in ((1, 2), (2, 1), (0, 2), (2, 0), (8193, 2), (2, 8193), (0xFFFFFFFF, 2)):
        assert create(heights=tiny, nx=nx, nz=nz) == INVALID and "2 to 8192" in err(), (nx, nz)
    for cell in ((0.0, 1.0), (1.0, 0.0), (-1.0, 1.0), (1.0, -0.5), (nan, 1.0), (1.0, nan), (inf, 1.0), (1.0, inf)):
        assert create(cell=cell) == INVALID and "cell_x / cell_z must be finite and > 0" in err(), cell
    for origin in ((nan, 0.0), (0.0, nan), (inf, 0.0), (0.0, -inf)):
        assert create(origin=origin) == INVALID and "origin_x / origin_z must be finite" in err(), origin
    for bad in (nan, inf, -inf):
        h = np.zeros((2, 3), F)
        h[1, 2] = bad
        assert create(heights=h) == INVALID and "heights[1][2] is not finite" in err(), bad
    assert out.value is None                                               # a refusal hands out nothing
    # what is allowed: the smallest and a tall field, a huge cell, a denormal cell, negative origins; and the ground reports itself
    assert create(heights=tiny, nx=2, nz=2, cell=(1e30, 1e-40), origin=(-1e30, 5.0)) == api.OK
    hip_lib.mmdx_ground_destroy(out)
    H = gr.hills(5, 8192, 1)
    with Ground(H, (-2.0, 3.0), (0.5, 0.25)) as g:
        assert g.info() == dict(nx=5, nz=8192, origin_x=-2.0, origin_z=3.0, cell_x=0.5, cell_z=0.25, min_height=float(H.min()),
                                max_height=float(H.max()), device_ordinal=-1)
        info = api.GroundInfo(8)
        assert hip_lib.mmdx_ground_get_info(g.h, C.byref(info)) == INVALID and "struct_size" in err()
        H[:] = 0                                                           # the ground copied what it needs
        assert g.info()["max_height"] > 1.0
    assert g.h is None
    hip_lib.mmdx_ground_destroy(None)                                      # like free(NULL)


def test_ground_calls_refuse_bad_arguments_before_any_device_call(hip_lib):
    """Every call here carries its defect AND a host list with an id that is no instance behind it (or is refused ahead of any
    pointer being looked at), so none of them can reach a device; the host-only model is refused behind every check of the arguments
    and ahead of the device."""
    g = _ground(gr.fields()["3x2"])
    err = lambda: (hip_lib.mmdx_last_error_string() or b"").decode()          # noqa: E731
    P = 0x100000                                                           # stands for device addresses; never dereferenced
    ids = np.array([0, 9], U)
    host_bad = vmd.instance_select(ids.ctypes.data, 2, None, on_device=False)          # id 9 >= 4: the refusal behind the others
    nan, inf = float("nan"), float("inf")

    def place(ground=g.h, struct_size=None, flags=0, ni=4, y_offset=0.0, placements=P, drop=None, select=host_bad, null_args=False, model=None):
        a = api.GroundPlaceArgs(C.sizeof(api.GroundPlaceArgs) if struct_size is None else struct_size, flags, ni, y_offset, placements, drop)
        if select is not None:
            a.select = C.pointer(select)
        return hip_lib.mmdx_ground_place(ground, model, None if null_args else C.byref(a))

    def targets(ground=g.h, struct_size=None, flags=0, ni=4, nf=2, placements=P, points=P + 0x1000, ps_=16, ss=64, out=P + 0x2000,
                out_drop=P + 0x3000, max_step=1.0, max_drop=1.0, select=host_bad, null_args=False, model=None):
        a = api.GroundTargetsArgs(C.sizeof(api.GroundTargetsArgs) if struct_size is None else struct_size, flags, ni, nf, placements, points,
                                  ps_, ss, out, out_drop, max_step, max_drop)
        if select is not None:
            a.select = C.pointer(select)
        return hip_lib.mmdx_ground_targets(ground, model, None if null_args else C.byref(a))
    for call in (place, targets):
        assert call() == INVALID and "ids[1] = 9 is not below n_instances" in err()          # the guard itself
        assert call(ground=None) == INVALID and "NULL" in err()
        assert call(null_args=True) == INVALID and "NULL" in err()
        assert call(struct_size=16) == INVALID and "struct_size" in err()
        for bad in (1, 2, 1 << 8, 1 << 19, 1 << 20, 1 << 31):
            assert call(flags=bad) == INVALID and "unknown flag bits" in err(), bad
        assert call(placements=None) == INVALID and "NULL" in err()
        assert call(placements=P + 2) == INVALID and "4-byte aligned" in err()
        assert call(ni=(1 << 23) + 1) == UNSUPPORTED and "2^23" in err()
        assert call(select=vmd.instance_select(P, (1 << 23) + 1)) == UNSUPPORTED and "2^23" in err()
        assert call(select=vmd.instance_select(P + 2, 2)) == INVALID and "4-byte aligned" in err()
        sel = vmd.instance_select(ids.ctypes.data, 2, None, on_device=False)
        sel.reserved0 = 1
        assert call(select=sel) == INVALID and "reserved0" in err()
        assert call(ni=0, placements=None, select=None) == api.OK          # nothing to do, nothing looked at
    assert place(drop=P + 0x1001) == INVALID and "4-byte aligned" in err()
    assert place(drop=P + 4) == INVALID and "drop overlaps placements" in err()
    assert place(drop=P + 4 * 32) == INVALID and "ids[1]" in err()         # right behind the placements: allowed
    for nf in (0, 9, 1 << 31):
        assert targets(nf=nf) == INVALID and "n_feet = %d" % nf in err()
    for ps_, ss in ((0, 64), (16, 0), (2, 64), (16, 1)):
        assert targets(ps_=ps_, ss=ss) == INVALID and "a point is three floats" in err(), (ps_, ss)
    for bad in (-1.0, -1e-30, nan, inf, -inf):
        assert targets(max_step=bad) == INVALID and "max_step / max_drop must be finite and >= 0" in err(), bad
        assert targets(max_drop=bad) == INVALID and "max_step / max_drop must be finite and >= 0" in err(), bad
    assert targets(max_step=0.0, max_drop=0.0) == INVALID and "ids[1]" in err()          # zero is allowed
    assert targets(points=None) == INVALID and "NULL" in err()
    assert targets(out=None) == INVALID and "NULL" in err()
    assert targets(points=P + 0x1002) == INVALID and "4-byte aligned" in err()
    assert targets(out_drop=P + 0x3001) == INVALID and "4-byte aligned" in err()
    for off in (4, 8, 12):
        assert targets(out=P + 0x2000 + off) == INVALID and "out_targets must be 16-byte aligned" in err(), off
    assert targets(out_drop=None) == INVALID and "ids[1]" in err()         # allowed
    # overlaps: points span (nf-1)*ss + (ni-1)*ps + 3 = 115 floats, placements 32, out_targets nf*ni*4 = 32, out_drop 4
    assert targets(out=P + 0x1000 + 448) == INVALID and "out_targets overlaps points or placements" in err()      # the last point's floats
    assert targets(out=P + 0x1000 + 464) == INVALID and "ids[1]" in err()                                           # right behind them
    assert targets(out=P + 0x1000 - 128) == INVALID and "ids[1]" in err()                                           # right in front
    assert targets(out=P + 0x1000 - 112) == INVALID and "overlaps points" in err()
    assert targets(out=P + 112) == INVALID and "out_targets overlaps points or placements" in err()
    assert targets(out=P + 128) == INVALID and "ids[1]" in err()
    for where, off in (("points", 0x1000 + 456), ("placements", 124), ("out_targets", 0x2000 + 124)):
        assert targets(out_drop=P + off) == INVALID and "out_drop overlaps points, placements or out_targets" in err(), where
    assert targets(out_drop=P + 0x2000 + 128) == INVALID and "ids[1]" in err()
    with DeformModel(synth.make_model(64, 8, 0, 0, seed=3), host_only=True) as hm:
        ok_list = vmd.instance_select(ids.ctypes.data, 1, None, on_device=False)
        for call in (place, targets):
            assert call(model=hm.h) == INVALID and "ids[1]" in err()       # behind the checks of the arguments ...
            assert call(model=hm.h, select=ok_list) == NO_DEVICE and "MMDX_CREATE_HOST_ONLY" in err()      # ... and ahead of any device
    assert g.info()["device_ordinal"] == -1                                # nothing of the above went to a device
    g.close()


def test_kernel_resources_no_spills_no_scratch():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), api.LIB_PATH, "ground_"],
                         capture_output=True, text=True, check=True).stdout.splitlines()
    names = {l.split(" vgpr ")[0].strip() for l in out}
    assert names == {"ground_place_kernel<true>", "ground_place_kernel<false>", "ground_targets_kernel<true>", "ground_targets_kernel<false>"}
    for l in out:
        f = l.split(" vgpr ")[1].split()
        res = dict(zip(["vgpr"] + f[1::2], (int(v) for v in f[0::2])))
        assert res["spill"] == 0 and res["scratch"] == 0 and res["lds"] == 0 and res["vgpr"] <= 64, l


# ---------------------------------------------------------------------------------------- GPU ----
@pytest.fixture
def gpu(hip_lib):
    assert device_count() >= 1, "no HIP device visible: the GPU tests must run on the MI355X box"
    return hip_lib


class Guarded:
    """A device array of `shape` floats with GUARD sentinel bytes on both sides.  The copies are synchronous copies of the null
    stream: upload and read synchronise the model's stream first, so no copy overtakes a call that is still running."""

    def __init__(self, shape, dm):
        self.shape, self.dm = tuple(shape), dm
        self.nbytes = int(np.prod(shape)) * 4
        self.buf = DeviceBuffer(self.nbytes + 2 * GUARD)
        self.ptr = self.buf.ptr + GUARD
        self.buf.memset(SENT)

    def upload(self, a):
        a = np.ascontiguousarray(a, F)
        assert a.nbytes == self.nbytes
        self.dm.sync()
        self.buf.upload(a, GUARD)

    def fill(self):
        self.dm.sync()
        self.buf.memset(SENT)

    def read(self, what):
        self.dm.sync()
        raw = self.buf.download((self.nbytes + 2 * GUARD,), np.uint8)
        assert (raw[:GUARD] == SENT).all() and (raw[GUARD + self.nbytes:] == SENT).all(), what + ": a guard byte changed"
        return raw[GUARD:GUARD + self.nbytes].view(F).reshape(self.shape)

    def free(self):
        self.buf.free()


SENT_F = np.frombuffer(bytes([SENT] * 4), F)[0]
NB = 41
FEET_BONES = [20, 38, 13, 17, 7, 32, 0, 25]           # eight bones of the 41-bone rig, the first two its feet
_rig = {}


def rig():
    """The 41-bone rig of the reach tests, computed once and shared, never modified: model-space palettes of 257 instances."""
    if not _rig:
        from tests import reach_ref as rr
        parent, rest = rr.reach_rig()
        _rig.update(parent=parent, rest=rest, pal=rr.fk_palettes(parent, rest, 257, step=5))
    return _rig


def big_model():
    return DeformModel(synth.make_model(64, NB, 0, 0, seed=31))


def _crowd(field, ni, seed):
    """gr.crowd with unit headings, so that the placements place a palette."""
    pl, pts = gr.crowd(field, ni, seed)
    yaw = 0.05 + 0.37 * np.arange(ni)
    pl[:, 3:] = 0
    pl[:, 5], pl[:, 7] = np.sin(yaw / 2), np.cos(yaw / 2)
    return pl, pts


@pytest.mark.gpu
@pytest.mark.parametrize("ni", [1, 63, 64, 65, 257])
def test_gpu_both_calls_equal_the_restatement(gpu, ni):
    """The 2 x 2 and the 33 x 17 field; 1, 2 and 8 feet, from a real mmdx_palette_sockets slab of the placed 41-bone rig (points =
    slab + 12, strides 16 and NI*16) and from a compact [NF][NI][4] array (strides 4 and NI*4); with and without out_drop / drop:
    placements, targets and drops between their sentinels equal the restatement's, byte for byte."""
    r = rig()
    with big_model() as dm:
        sk = vmd.Skeleton(r["rest"], r["parent"])
        sockets = SocketSet.from_skeleton(dm, sk, FEET_BONES)
        d_pal, d_slab = DeviceBuffer(ni * NB * 64), DeviceBuffer(8 * ni * 64)
        d_place, d_pts, d_tgt, d_drop = Guarded((ni, 8), dm), Guarded((8, ni, 4), dm), Guarded((8, ni, 4), dm), Guarded((ni,), dm)
        for name in ("2x2", "33x17"):
            field = gr.fields()[name]
            ground = _ground(field)
            assert ground.info()["device_ordinal"] == -1
            pl, pts = _crowd(field, ni, 40 + ni)
            drop_in = np.random.RandomState(ni).uniform(-0.3, 0.0, ni).astype(F)
            # place, with and without a drop
            for with_drop in (False, True):
                what = f"{name}, NI {ni}, place, drop {with_drop}"
                d_place.upload(pl)
                d_drop.upload(drop_in)
                ground.place(dm, d_place, ni, drop=d_drop if with_drop else None, y_offset=0.125)
                want = gr.place(field, pl, drop_in if with_drop else None, 0.125)
                gr.assert_same(d_place.read(what), want, what)
                assert want.tobytes() != pl.tobytes() and d_drop.read(what).tobytes() == drop_in.tobytes()
            stood = want
            # the feet of the placed rig
            dm.sync()
            d_pal.upload(pp.place_crowd(r["pal"][:ni], stood, False))
            sockets.sockets(d_pal, d_slab, n_instances=ni)
            dm.sync()
            slab = d_slab.download((8, ni, 16), F)
            assert (slab[:, :, 15] == 1.0).all()
            d_place.upload(stood)
            d_pts.upload(pts)
            for nf in (1, 2, 8):
                for source, ptr, ps_, points in (("sockets slab", d_slab.ptr + 48, 16, slab[:nf, :, 12:16]), ("compact", d_pts.ptr, 4, pts[:nf])):
                    for with_drop in (True, False):
                        what = f"{name}, NI {ni}, {nf} feet, {source}, drop {with_drop}"
                        d_tgt.fill()
                        d_drop.fill()
                        ground.targets(dm, d_place, ptr, d_tgt, ni, nf, point_stride=ps_, out_drop=d_drop if with_drop else None,
                                       max_step=0.35, max_drop=0.2)
                        want_t, want_d = gr.targets(field, stood, points, 0.35, 0.2, with_drop)
                        got_t, got_d = d_tgt.read(what), d_drop.read(what)
                        gr.assert_same(got_t[:nf], want_t, what)
                        assert (got_t[nf:].view(U) == SENT_F.view(U)).all(), what + ": a slab behind n_feet changed"
                        if with_drop:
                            gr.assert_same(got_d, want_d, what + ": drop")
                        else:
                            assert (got_d.view(U) == SENT_F.view(U)).all(), what + ": a drop nobody asked for"
                        assert (want_t[:, :, 3] == 1).all() and d_place.read(what).tobytes() == stood.tobytes()
            assert ground.info()["device_ordinal"] >= 0
            ground.close()
        _close(d_pal, d_slab, d_place, d_pts, d_tgt, d_drop, sockets, sk)


@pytest.mark.gpu
def test_gpu_case_table_through_the_kernels(gpu):
    """Every call of the case table of every field -- each branch the header names -- through the kernels: 150 and 260 instances,
    three and five workgroups."""
    with big_model() as dm:
        for name, case in gr.case_table().items():
            ground = _ground(case["field"])
            pl, pts, drop = case["placements"], case["points"], case["drop"]
            ni = pl.shape[0]
            d_place, d_pts, d_tgt, d_drop = Guarded((ni, 8), dm), Guarded((8, ni, 4), dm), Guarded((8, ni, 4), dm), Guarded((ni,), dm)
            d_pts.upload(pts)
            for c, want in zip(case["calls"], gr.run_calls(case)):
                what = f"{name}, {c}"
                d_place.upload(pl)
                if c["kind"] == "place":
                    d_drop.upload(drop)
                    ground.place(dm, d_place, ni, drop=d_drop if c["with_drop"] else None, y_offset=c["y_offset"])
                    gr.assert_same(d_place.read(what), want[0], what)
                else:
                    nf = c["n_feet"]
                    d_tgt.fill()
                    d_drop.fill()
                    ground.targets(dm, d_place, d_pts, d_tgt, ni, nf, point_stride=4, out_drop=d_drop if c["want_drop"] else None,
                                   max_step=c["max_step"], max_drop=c["max_drop"])
                    gr.assert_same(d_tgt.read(what)[:nf], want[0], what)
                    if c["want_drop"]:
                        gr.assert_same(d_drop.read(what), want[1], what + ": drop")
            _close(d_place, d_pts, d_tgt, d_drop, ground)


@pytest.mark.gpu
def test_gpu_a_nan_instance_stays_with_its_instance(gpu):
    """65 instances on the 33 x 17 field.  A NaN x of placement 20, an infinite foot of instance 21, a NaN drop of instance 22: their
    neighbours, lanes of the same wave, are the restatement's; placements 20 and 22 keep every byte; instance 21's other foot is
    right; instance 20 gets targets (its ty is finite) and no drop."""
    field = gr.fields()["33x17"]
    ni = 65
    pl, pts = _crowd(field, ni, 8)
    pl, pts = pl[:, :], pts[:2].copy()
    drop = np.full(ni, -0.05, F)
    pl[20, 0] = np.nan
    pts[0, 21, 2] = np.inf
    drop[22] = np.nan
    with big_model() as dm, _ground(field) as ground:
        d_place, d_pts, d_tgt, d_drop = Guarded((ni, 8), dm), Guarded((2, ni, 4), dm), Guarded((2, ni, 4), dm), Guarded((ni,), dm)
        d_place.upload(pl)
        d_drop.upload(drop)
        ground.place(dm, d_place, ni, drop=d_drop, y_offset=0.5)
        got, want = d_place.read("place"), gr.place(field, pl, drop, 0.5)
        gr.assert_same(got, want, "place")
        assert got[20].tobytes() == pl[20].tobytes() and got[22].tobytes() == pl[22].tobytes()
        assert all(got[i, 1] != pl[i, 1] and np.isfinite(got[i]).all() for i in (19, 21, 23))
        d_pts.upload(pts)
        d_tgt.fill()
        ground.targets(dm, d_place, d_pts, d_tgt, ni, 2, point_stride=4, out_drop=d_drop, max_step=0.4, max_drop=0.3)
        want_t, want_d = gr.targets(field, want, pts, 0.4, 0.3)
        got_t, got_d = d_tgt.read("targets"), d_drop.read("drop")
        gr.assert_same(got_t, want_t, "targets")
        gr.assert_same(got_d, want_d, "drop")
        assert got_t[0, 21].tobytes() == bytes(16) and got_t[1, 21, 3] == 1.0
        assert np.isfinite(np.delete(got_t, 21, axis=1)).all() and (np.delete(got_t, 21, axis=1)[:, :, 3] == 1).all()
        assert got_d[20] == 0 and np.isfinite(got_d).all()                  # h0 of instance 20 fails: no drop; its feet are fine
        _close(d_place, d_pts, d_tgt, d_drop)


SEL_IDS = np.array([3, 64, 0, 7, 33, 1, 12, 40, 16, 17, 63, 21, 22, 23, 24, 25, 26, 27], U)
SEL_IDS_DEV = np.array([3, 64, 0, 70, 7, 0xFFFFFFFF, 12, 40, 16, 17, 63, 21, 22, 23, 24, 25, 26, 27], U)     # 70 and 2^32-1: no instances of 65


@pytest.mark.gpu
@pytest.mark.parametrize("where", ["host list", "device list"])
def test_gpu_select_touches_the_listed_instances_only(gpu, where):
    """65 instances, 18 list positions, and a shuffle of all 65 with 40 in use (more than a workgroup).  Lists with count NULL, 0, 5,
    17 and 100 (above n_ids): listed placements, targets and drops are the restatement's, unlisted ones keep the sentinel pattern
    byte for byte; device ids that are no instance are skipped; a list of capacity 0; a host id that is no instance."""
    field = gr.fields()["33x17"]
    ni = 65
    pl, pts = _crowd(field, ni, 13)
    pts = pts[:2]
    drop_in = np.full(ni, -0.0625, F)
    keep_t, keep_d = np.full((2, ni, 4), SENT_F, F), np.full(ni, SENT_F, F)
    with big_model() as dm, _ground(field) as ground:
        d_place, d_pts, d_tgt, d_drop, d_din = (Guarded(s, dm) for s in ((ni, 8), (2, ni, 4), (2, ni, 4), (ni,), (ni,)))
        d_pts.upload(pts)
        d_din.upload(drop_in)
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
                used = [int(i) for i in (ids if count is None else ids[:min(count, ids.size)]) if i < ni]
                d_place.upload(pl)
                ground.place(dm, d_place, ni, drop=d_din, y_offset=0.25, select=sel)
                want = gr.place(field, pl, drop_in, 0.25, ids=used)
                unlisted = np.ones(ni, bool)
                unlisted[used] = False
                assert want[unlisted].tobytes() == pl[unlisted].tobytes() and (not used or want.tobytes() != pl.tobytes())
                gr.assert_same(d_place.read(what), want, what + ": place")
                d_tgt.fill()
                d_drop.fill()
                ground.targets(dm, d_place, d_pts, d_tgt, ni, 2, point_stride=4, out_drop=d_drop, max_step=0.4, max_drop=0.3, select=sel)
                want_t, want_d = gr.targets(field, want, pts, 0.4, 0.3, ids=used, out=keep_t, out_drop=keep_d)
                assert (want_t[:, unlisted].view(U) == SENT_F.view(U)).all() and (want_d[unlisted].view(U) == SENT_F.view(U)).all()
                gr.assert_same(d_tgt.read(what), want_t, what + ": targets")
                gr.assert_same(d_drop.read(what), want_d, what + ": drop")
            dm.sync()
            d_ids.free()
        d_ids = DeviceBuffer.from_numpy(SEL_IDS)
        d_place.upload(pl)
        d_tgt.fill()
        empty = vmd.instance_select(d_ids.ptr, 0)
        ground.place(dm, d_place, ni, y_offset=1.0, select=empty)
        ground.targets(dm, d_place, d_pts, d_tgt, ni, 2, point_stride=4, select=empty)
        assert d_place.read("n_ids 0").tobytes() == pl.tobytes() and d_tgt.read("n_ids 0").tobytes() == keep_t.tobytes()
        bad = np.array([1, 65], U)
        bad_sel = vmd.instance_select(bad.ctypes.data, 2, None, on_device=False)
        with pytest.raises(api.MmdxError, match="is not below n_instances"):
            ground.place(dm, d_place, ni, select=bad_sel)
        with pytest.raises(api.MmdxError, match="is not below n_instances"):
            ground.targets(dm, d_place, d_pts, d_tgt, ni, 2, point_stride=4, select=bad_sel)
        assert d_place.read("after the refusal").tobytes() == pl.tobytes() and d_tgt.read("after the refusal").tobytes() == keep_t.tobytes()
        _close(d_place, d_pts, d_tgt, d_drop, d_din, d_ids, d_cnt)


def _limbs(parent):
    """Two disjoint three-bone chains a -> b -> c by parent links, the second one's subtree outside the first's, and a leaf outside
    both for a spring chain: (limbs, leaf)."""
    from tests import reach_ref as rr
    nb = len(parent)
    chains = [(int(parent[parent[c]]), int(parent[c]), c) for c in range(nb) if parent[c] > 0 and parent[parent[c]] > 0]
    for first in chains:
        for second in chains:
            if rr.is_under(parent, first[0], second[0]) or rr.is_under(parent, second[0], first[0]):
                continue
            kids = set(int(p) for p in parent)
            for leaf in range(nb - 1, 0, -1):
                if leaf not in kids and parent[leaf] >= 0 and not rr.is_under(parent, first[0], leaf) and not rr.is_under(parent, second[0], leaf):
                    return [first, second], leaf
    raise AssertionError("the skeleton has no two disjoint limbs")


@pytest.mark.gpu
def test_gpu_recorded_frame_replayed_40_times_on_a_borrowed_stream(gpu):
    """[root motion (x and z), ground place (reading last replay's drop), advance, blend solve, place, sockets of the two feet, ground
    targets, reach for each of the two feet, spring step, palette bounds] recorded once on a stream of the test's that the model
    borrows, replayed 40 times; the placements are rewritten in place by every replay, dt is rewritten in device memory.  After every
    replay: ty is the restatement's of this replay's x and z and of LAST replay's drop; the sockets slab is the restatement's of the
    placed palettes; targets and drop are the restatement's of that slab; the palettes are the restatements' two reaches and spring
    step on them; the boxes those of the palettes.  Nothing runs before the first replay; a host list and a fresh ground are
    refused while recording; destroying the ground invalidates the graph."""
    from tests import animator_ref as ar
    from tests import hip_stream_util as hs
    from tests import palette_bounds_ref as pb
    from tests import reach_ref as rr
    from tests import spring_ref as sr
    from tests import test_animator as ta
    hs.hip()
    m = synth.make_model(2048, 64, 8, 200, 112)
    names = [f"bone{i}" for i in range(m.nb)]
    parent, rest = np.asarray(m.bone_parent, np.int32), np.asarray(m.bone_pos, F)
    nb, ni, n_replays = m.nb, 65, 40
    limbs, leaf = _limbs(parent)
    feet = [l[2] for l in limbs]
    reaches = [[rr.make_reach(*l, max_extension=0.97, pole=(0.0, 0.0, 1.0), flags=rr.KEEP_END_ROTATION)] for l in limbs]
    rtables = [rr.build_table(parent, rest, r) for r in reaches]
    chains, params = [[leaf]], [[20.0, 0.2, 1.0, 0.1]]
    stable = sr.build_table(parent, rest, chains, params, (0.0, -9.8, 0.0), None)
    field = gr.make_field(gr.hills(33, 17, 21, amplitude=2.0), (-24.0, -20.0), (1.5, 2.5))
    vs = [vmd.Vmd(d) for d in ta.scenario_vmds(names)]
    moving = [v.bind_bones(names) for v in vs]
    still = [b.in_place(0, api.ROOT_X | api.ROOT_Y | api.ROOT_Z) for b in moving]
    roots = [v.bind_bones(names[:1]) for v in vs]
    in_place_set, root_set = vmd.MotionSet(still), vmd.MotionSet(roots)
    start = ar.initial_state(ni)
    n_clips = len(ar.CLIP_FRAMES)
    start["clips_a"][:] = np.arange(ni) % n_clips
    start["times_a"][:] = (np.arange(ni) % 7) * 0.1
    rng = np.random.RandomState(3)
    place0 = np.zeros((ni, 8), F)
    place0[:, 0], place0[:, 1], place0[:, 2] = rng.uniform(-22, 22, ni), rng.uniform(-5, 5, ni), rng.uniform(-18, 18, ni)
    yaw = 0.3 * np.arange(ni)
    place0[:, 5], place0[:, 7] = np.sin(yaw / 2), np.cos(yaw / 2)
    dts = rng.uniform(1 / 144, 1 / 30, n_replays)
    max_step, max_drop, y_offset = 1.5, 0.75, 0.125
    with DeformModel(m) as dm, hs.Stream() as S:
        sk = vmd.Skeleton(rest, parent)
        an = vmd.Animator(in_place_set, ni, ta.rows_for_create())
        ground, fresh = _ground(field), _ground(field)
        sockets = SocketSet.from_skeleton(dm, sk, feet)
        rsets = [ReachSet(sk, [{k: v for k, v in r[0].items() if v is not None}]) for r in reaches]
        sset = SpringSet(sk, chains, params, ni)
        d_dt, d_dt32 = DeviceBuffer.from_numpy(np.array([0.0], np.float64)), DeviceBuffer.from_numpy(np.array([0.0], F))
        d_place, d_drop, d_tgt = Guarded((ni, 8), dm), Guarded((ni,), dm), Guarded((2, ni, 4), dm)
        d_pal0, d_pal, d_slab, d_box = DeviceBuffer(ni * nb * 64), Guarded((ni, nb, 16), dm), DeviceBuffer(2 * ni * 64), DeviceBuffer(ni * 24)
        d_ids = DeviceBuffer.from_numpy(np.arange(ni, dtype=U))

        def frame():
            an.root_motion(root_set, 0, api.ROOT_X | api.ROOT_Z, d_place.ptr, dt_ptr=d_dt.ptr, model=dm)
            ground.place(dm, d_place, ni, drop=d_drop, y_offset=y_offset)
            an.advance_device_dt(d_dt.ptr, dm)
            sk.solve_motion_set_blend_time_device(in_place_set, ni, *an.operand_ptrs(), d_pal0.ptr, dm)
            dm.place_palettes(ni, d_pal0.ptr, d_place.ptr, d_pal.ptr, PLACE_DEV)
            sockets.sockets(d_pal, d_slab, n_instances=ni)
            ground.targets(dm, d_place, d_slab.ptr + 48, d_tgt, ni, 2, point_stride=16, out_drop=d_drop, max_step=max_step, max_drop=max_drop,
                           select=vmd.instance_select(d_ids.ptr, ni))
            for f, rset in enumerate(rsets):
                rset.reach(dm, d_pal, d_tgt.ptr + f * ni * 16, stride=4, n_instances=ni)
            sset.step(d_pal, dt_ptr=d_dt32.ptr, n_instances=ni, model=dm)
            dm.palette_bounds_raw(ni, d_pal.ptr, d_box.ptr, DEV, 1.0, 1.0)
        try:
            dm.set_stream(S.ptr)
            an.set_state(dm, **start)
            d_place.upload(place0)
            d_drop.upload(np.zeros(ni, F))
            frame()                                                           # the run before recording: the sets go to the device
            S.synchronize()
            an.set_state(dm, **start)
            sset.set_state(sr.nan_state(ni, 1), dm)
            for g in (d_place, d_drop, d_tgt, d_pal):
                g.fill()
            S.synchronize()
            dm.graph_begin()
            try:
                assert S.capture_status() == hs.CAPTURE_ACTIVE
                frame()
                host_ids = np.arange(3, dtype=U)
                host_sel = vmd.instance_select(host_ids.ctypes.data, 3, None, on_device=False)
                with pytest.raises(api.MmdxError, match="instance list must be in device memory"):
                    ground.place(dm, d_place, ni, select=host_sel)
                with pytest.raises(api.MmdxError, match="instance list must be in device memory"):
                    ground.targets(dm, d_place, d_slab.ptr + 48, d_tgt, ni, 2, select=host_sel)
                with pytest.raises(api.MmdxError, match="must have run on this device before"):
                    fresh.place(dm, d_place, ni)
                assert S.capture_status() == hs.CAPTURE_ACTIVE
            finally:
                graph = dm.graph_end()
            try:
                S.synchronize()
                for g in (d_place, d_drop, d_tgt, d_pal):
                    assert (g.buf.download((g.nbytes + 2 * GUARD,), np.uint8) == SENT).all(), "recording ran something"
                d_place.upload(place0)
                d_drop.upload(np.zeros(ni, F))
                state, prev_place, prev_drop = sr.nan_state(ni, 1), place0, np.zeros(ni, F)
                dropped = 0
                for k in range(n_replays):
                    d_dt.upload(dts[k:k + 1])
                    d_dt32.upload(dts[k:k + 1].astype(F))
                    graph.launch()
                    S.synchronize()
                    now = d_place.read(f"replay {k}")
                    assert (now[:, [0, 2]] != prev_place[:, [0, 2]]).any(), f"replay {k}: root motion moved nobody"      # (a held clip stands)
                    walked = prev_place.copy()
                    walked[:, [0, 2]] = now[:, [0, 2]]                         # root motion's part, its own tests hold it
                    gr.assert_same(now, gr.place(field, walked, prev_drop, y_offset), f"replay {k}: placements, with replay {k - 1}'s drop")
                    placed = pp.place_crowd(d_pal0.download((ni, nb, 16), F), now, False)
                    slab = d_slab.download((2, ni, 16), F)
                    gr.assert_same(slab, ps.sockets(placed, feet, rest[feet]), f"replay {k}: the feet")
                    want_t, want_d = gr.targets(field, now, slab[:, :, 12:16], max_step, max_drop)
                    gr.assert_same(d_tgt.read(f"replay {k}"), want_t, f"replay {k}: targets")
                    gr.assert_same(d_drop.read(f"replay {k}"), want_d, f"replay {k}: drop")
                    assert (want_t[:, :, 3] == 1).all()
                    reached = rr.reach(rtables[1], rr.reach(rtables[0], placed, want_t[0]), want_t[1])
                    assert reached.tobytes() != placed.tobytes()
                    wp, state = sr.step(stable, reached, state, F(dts[k]))
                    gr.assert_same(d_pal.read(f"replay {k}"), wp, f"replay {k}: palettes")
                    if k in (0, 11, 39):
                        gr.assert_same(d_box.download((ni, 6), F), pb.palette_bounds(dm.bone_boxes(), wp, 1.0, 1.0), f"replay {k}: boxes")
                    dropped += int((want_d < 0).sum())
                    prev_place, prev_drop = now, want_d
                assert dropped > n_replays                                   # (the one-frame-late drop is not a row of zeros)
                assert (prev_place[:, [0, 2]] != place0[:, [0, 2]]).any(axis=1).sum() > ni // 2      # the crowd walked
                ground.close()                                               # took part in the recording
                with pytest.raises(api.MmdxError, match="destroyed"):
                    graph.launch()
            finally:
                graph.close()
        finally:
            dm.set_stream(None)
        _close(d_dt, d_dt32, d_place, d_drop, d_tgt, d_pal0, d_pal, d_slab, d_box, d_ids, fresh, rsets, sset, sockets, an, sk)
    _close(root_set, in_place_set, roots, still, moving, vs)

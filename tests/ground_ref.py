"""The ground section of include/mmdx.h, restated in numpy from the header's text: h(x, z), mmdx_ground_place and mmdx_ground_targets,
every operation in binary32 in the order written (ft=np.float64: the same formulas in binary64, for the tolerances); the fields and
the case table of tests/test_ground.py; and the exchange with the CPU driver (tests/ground_math_driver.cpp).  No GPU, no reference tree.
"""
import os
import struct

import numpy as np

from tests import host_program as hp
from tests.aim_ref import assert_same  # noqa: F401  (bit for bit, a NaN only has to be a NaN)

HERE = os.path.dirname(os.path.abspath(__file__))
F, U = np.float32, np.uint32
MAX_FEET, MIN_SAMPLES, MAX_SAMPLES = 8, 2, 8192
THREADS = 64                                     # kGroundThreads: lanes = instances per workgroup
SENT_WORD = 0xCDCDCDCD

# every branch the header names: what case_table() must contain (test_case_table_contains_every_branch_the_header_names)
CASES = ("lower", "upper", "diagonal", "edge fu 0", "edge fu 1", "edge fv 0", "edge fv 1", "corner 00", "corner 10", "corner 01", "corner 11",
         "outside -x", "outside +x", "outside -z", "outside +z", "outside -x-z", "outside +x-z", "outside -x+z", "outside +x+z",
         "last cell fu 1", "last cell fv 1", "sample nan", "sample inf", "place fails", "place drop nan", "place drop inf", "place with drop",
         "place without drop", "foot x nan", "foot x inf", "foot z nan", "foot z inf", "foot y nan", "foot y inf", "ty nan", "ty inf",
         "dy clamped up", "dy clamped down", "dy free", "max_step 0", "drop no foot", "drop one foot fails", "drop h0 fails",
         "drop clamped", "drop free", "drop zero", "max_drop 0", "feet 1", "feet 2", "feet 8")


def _bump(count, key, n):
    if count is not None and n:
        count[key] = count.get(key, 0) + int(n)


# ------------------------------------------------------------------------------------------------ fields -----------------------
def make_field(heights, origin=(0.0, 0.0), cell=(1.0, 1.0)):
    h = np.ascontiguousarray(heights, F)
    assert h.ndim == 2
    return dict(H=h, nx=h.shape[1], nz=h.shape[0], origin=(F(origin[0]), F(origin[1])), cell=(F(cell[0]), F(cell[1])))


def hills(nx, nz, seed, amplitude=3.0):
    """Heights [nz][nx]: two sines and noise, no symmetry, both signs."""
    rng = np.random.RandomState(seed)
    x, z = np.meshgrid(np.arange(nx), np.arange(nz))
    return (amplitude * np.sin(0.37 * x + 0.2) * np.cos(0.23 * z - 0.4) + rng.uniform(-0.5, 0.5, (nz, nx))).astype(F)


def fields():
    """The three fields of the tests: one cell, 3 x 2 with cells that are no binary fractions, 33 x 17 with dyadic cells (so that a
    point meant to lie on a diagonal, an edge or a sample does).  Unequal cells and negative origins."""
    return {"2x2": make_field(hills(2, 2, 1), (-1.0, -2.0), (2.0, 0.5)),
            "3x2": make_field(hills(3, 2, 2), (-0.7, -2.9), (0.3, 1.7)),
            "33x17": make_field(hills(33, 17, 3), (-4.0, -1.5), (0.5, 0.25))}


# ------------------------------------------------------------------------------------------------ h(x, z) ----------------------
def axis(x, origin, cell, n, ft=F):
    """Cell and fraction -> (ok, raw u, i, f)."""
    x = np.asarray(x, ft)
    with np.errstate(all="ignore"):
        raw = (x - ft(origin)) / ft(cell)
        ok = np.isfinite(raw)
        u = np.where(ok, raw, ft(0))
        top = ft(n - 1)
        u = np.where(u < 0, ft(0), u)
        u = np.where(u > top, top, u)
        i = np.minimum(u.astype(np.int64), n - 2)
        f = (u - i.astype(ft)).astype(ft)
    return ok, raw, i, f


def height(field, x, z, ft=F, count=None):
    """h(x, z) -> (ok, h); h is 0 where the sample fails."""
    H = field["H"].astype(ft)
    nx, nz = field["nx"], field["nz"]
    oku, ru, iu, fu = axis(x, field["origin"][0], field["cell"][0], nx, ft)
    okv, rv, iv, fv = axis(z, field["origin"][1], field["cell"][1], nz, ft)
    ok = oku & okv
    with np.errstate(all="ignore"):
        h00, h10, h01, h11 = H[iv, iu], H[iv, iu + 1], H[iv + 1, iu], H[iv + 1, iu + 1]
        one = ft(1)
        s = fu + fv
        lower = s <= one
        lo = (h00 * ((one - fu) - fv) + h10 * fu) + h01 * fv
        up = (h11 * (s - one) + h10 * (one - fv)) + h01 * (one - fu)
        h = np.where(ok, np.where(lower, lo, up), ft(0)).astype(ft)
    if count is not None:
        raw_bad = ~ok
        xs, zs = np.broadcast_to(np.asarray(x, ft), ok.shape), np.broadcast_to(np.asarray(z, ft), ok.shape)
        _bump(count, "sample nan", (raw_bad & (np.isnan(xs) | np.isnan(zs))).sum())
        _bump(count, "sample inf", (raw_bad & (np.isinf(xs) | np.isinf(zs))).sum())
        inside = ok & (ru >= 0) & (ru <= nx - 1) & (rv >= 0) & (rv <= nz - 1)
        _bump(count, "lower", (inside & lower & (s < one)).sum())
        _bump(count, "upper", (inside & ~lower).sum())
        _bump(count, "diagonal", (inside & (s == one) & (fu > 0) & (fv > 0)).sum())
        for key, m in (("edge fu 0", (fu == 0) & (fv > 0) & (fv < 1)), ("edge fu 1", (fu == 1) & (fv > 0) & (fv < 1)),
                       ("edge fv 0", (fv == 0) & (fu > 0) & (fu < 1)), ("edge fv 1", (fv == 1) & (fu > 0) & (fu < 1)),
                       ("corner 00", (fu == 0) & (fv == 0)), ("corner 10", (fu == 1) & (fv == 0)), ("corner 01", (fu == 0) & (fv == 1)),
                       ("corner 11", (fu == 1) & (fv == 1)), ("last cell fu 1", (iu == nx - 2) & (fu == 1)),
                       ("last cell fv 1", (iv == nz - 2) & (fv == 1))):
            _bump(count, key, (inside & m).sum())
        lx, hx, lz, hz = ok & (ru < 0), ok & (ru > nx - 1), ok & (rv < 0), ok & (rv > nz - 1)
        mx, mz = ok & ~lx & ~hx, ok & ~lz & ~hz
        for key, m in (("outside -x", lx & mz), ("outside +x", hx & mz), ("outside -z", lz & mx), ("outside +z", hz & mx),
                       ("outside -x-z", lx & lz), ("outside +x-z", hx & lz), ("outside -x+z", lx & hz), ("outside +x+z", hx & hz)):
            _bump(count, key, m.sum())
    return ok, h


# ------------------------------------------------------------------------------------------------ the two calls ----------------
def _listed(ni, ids):
    live = np.zeros(ni, bool)
    if ids is None:
        live[:] = True
    else:
        live[[int(i) for i in ids if int(i) < ni]] = True
    return live


def place(field, placements, drop=None, y_offset=0.0, ids=None, ft=F, count=None):
    """mmdx_ground_place -> the placements after the call (a copy; only [i][1] of a listed, unrefused instance differs)."""
    p = np.array(placements, ft).reshape(-1, 8)
    live = _listed(p.shape[0], ids)
    ok, h0 = height(field, p[:, 0], p[:, 2], ft, count)
    with np.errstate(all="ignore"):
        ty = h0 + ft(y_offset)
        if drop is not None:
            d = np.asarray(drop, ft).reshape(-1)
            _bump(count, "place drop nan", (ok & np.isnan(d)).sum())
            _bump(count, "place drop inf", (ok & np.isinf(d)).sum())
            ok = ok & np.isfinite(d)
            ty = ty + d
            _bump(count, "place with drop", ok.sum())
        else:
            _bump(count, "place without drop", ok.sum())
    _bump(count, "place fails", (~ok).sum())
    w = ok & live
    p[w, 1] = ty[w]
    return p


def targets(field, placements, points, max_step, max_drop, want_drop=True, ids=None, out=None, out_drop=None, ft=F, count=None):
    """mmdx_ground_targets.  points [NF, NI, >= 3] -> (targets [NF, NI, 4], drop [NI] or None).  out / out_drop: what the arrays held
    before the call (unlisted instances keep it); default: the sentinel word."""
    p = np.asarray(placements, ft).reshape(-1, 8)
    pts = np.asarray(points, ft)
    nf, ni = pts.shape[0], pts.shape[1]
    live = _listed(ni, ids)
    sent = np.array([SENT_WORD], U).view(F)[0]
    tgt = np.full((nf, ni, 4), sent, ft) if out is None else np.array(out, ft).reshape(nf, ni, 4)
    drp = (np.full(ni, sent, ft) if out_drop is None else np.array(out_drop, ft).reshape(ni)) if want_drop else None
    _bump(count, "feet %d" % nf, 1)
    ty = p[:, 1]
    ms, md = ft(max_step), ft(max_drop)
    _bump(count, "max_step 0", int(ms == 0))
    if want_drop:
        _bump(count, "max_drop 0", int(md == 0))
        h0_ok, h0 = height(field, p[:, 0], p[:, 2], ft, count)
        m, have = np.zeros(ni, ft), np.zeros(ni, bool)
        n_ok = np.zeros(ni, np.int64)
    with np.errstate(all="ignore"):
        for f in range(nf):
            px, py, pz = pts[f, :, 0], pts[f, :, 1], pts[f, :, 2]
            sampled, hf = height(field, px, pz, ft, count)
            good = sampled & np.isfinite(px) & np.isfinite(py) & np.isfinite(pz) & np.isfinite(ty)
            dy = hf - ty
            lo, hi = dy < -ms, None
            dy = np.where(lo, -ms, dy)
            hi = dy > ms
            dy = np.where(hi, ms, dy)
            t = np.stack([px, py + dy, pz, np.ones(ni, ft)], axis=1)
            t = np.where(good[:, None], t, ft(0))
            tgt[f, live] = t[live]
            if count is not None:
                for key, m_ in (("foot x nan", np.isnan(px)), ("foot x inf", np.isinf(px)), ("foot z nan", np.isnan(pz)),
                                ("foot z inf", np.isinf(pz)), ("foot y nan", sampled & np.isnan(py)), ("foot y inf", sampled & np.isinf(py)),
                                ("ty nan", sampled & np.isnan(ty)), ("ty inf", sampled & np.isinf(ty)), ("dy clamped up", good & hi & (ms > 0)),
                                ("dy clamped down", good & lo & (ms > 0)), ("dy free", good & ~lo & ~hi)):
                    _bump(count, key, m_.sum())
            if want_drop:
                use = sampled & h0_ok
                d = hf - h0
                take = use & (d < m)                                        # m starts at 0: a NaN d is never taken
                m = np.where(take, d, m)
                have |= use
                n_ok += sampled
        if want_drop:
            r = np.where(m < 0, m, ft(0))
            clamped = r < -md
            r = np.where(clamped, -md, r)
            drp[live] = r[live]
            _bump(count, "drop no foot", (h0_ok & (n_ok == 0)).sum())
            _bump(count, "drop one foot fails", (h0_ok & (n_ok > 0) & (n_ok < nf)).sum())
            _bump(count, "drop h0 fails", (~h0_ok & (n_ok > 0)).sum())
            _bump(count, "drop clamped", (clamped & (md > 0)).sum())
            _bump(count, "drop free", (have & ~clamped & (r < 0)).sum())
            _bump(count, "drop zero", (have & (m >= 0)).sum())
    return tgt, drp


# ------------------------------------------------------------------------------------------------ the case table ---------------
def probe_points(field, seed, n_random=24):
    """(x, z) [N, 2]: every sample-relative position the header distinguishes, in the first cell, an inner cell and the last cell,
    outside on every side and at every corner, then random points in and around the field."""
    nx, nz = field["nx"], field["nz"]

    def coords(n):
        base = [-1.5, 0.0, 0.25, 0.5, 0.75, 1.0, n - 1.5, n - 1.25, n - 1.0, n + 1.0]
        if n > 4:
            base += [n // 2 + f for f in (0.0, 0.25, 0.5, 0.75)]
        return base
    uv = np.array([(u, v) for u in coords(nx) for v in coords(nz)], np.float64)
    rng = np.random.RandomState(seed)
    uv = np.concatenate([uv, rng.uniform((-1.0, -1.0), (nx, nz), (n_random, 2))])
    x = np.float64(field["origin"][0]) + uv[:, 0] * np.float64(field["cell"][0])
    z = np.float64(field["origin"][1]) + uv[:, 1] * np.float64(field["cell"][1])
    return np.stack([x, z], axis=1).astype(F)


def crowd(field, ni, seed, spread=0.6):
    """(placements [NI, 8], points [8, NI, 4]): placements standing on probe points and beyond, ty near the ground there, eight feet
    around each, at animated heights; the fourth float of a point is 1 (as a sockets translation row has it)."""
    rng = np.random.RandomState(seed)
    xz = probe_points(field, seed)
    xz = xz[np.arange(ni) % len(xz)] if ni <= len(xz) else np.concatenate([xz, xz[rng.randint(0, len(xz), ni - len(xz))]])
    pl = rng.uniform(-1, 1, (ni, 8)).astype(F)
    pl[:, 0], pl[:, 2] = xz[:, 0], xz[:, 1]
    _, h0 = height(field, pl[:, 0], pl[:, 2])
    pl[:, 1] = h0 + rng.uniform(-0.3, 0.3, ni).astype(F)
    pts = np.ones((MAX_FEET, ni, 4), F)
    cx, cz = float(field["cell"][0]), float(field["cell"][1])
    for f in range(MAX_FEET):
        other = xz[(np.arange(ni) * 3 + 7 * f + 1) % ni]                    # half the feet on probe points of their own
        near = np.stack([pl[:, 0] + rng.uniform(-spread, spread, ni) * cx, pl[:, 2] + rng.uniform(-spread, spread, ni) * cz], axis=1)
        pick = (np.arange(ni) + f) % 2 == 0
        pts[f, :, 0] = np.where(pick, other[:, 0], near[:, 0])
        pts[f, :, 2] = np.where(pick, other[:, 1], near[:, 1])
        pts[f, :, 1] = pl[:, 1] + rng.uniform(0.0, 0.4, ni)
    return pl, pts


def case_table():
    """Per field of fields(): dict(field, placements [NI,8], points [8,NI,4], drop [NI], calls): the crowd of crowd() with special
    instances in front -- NaN and +-inf in x, z, P.y, ty and the drop; targets far above and below; every foot failing, one foot
    failing, h0 failing -- and the calls to run on it (dicts for run_calls / run_driver)."""
    nan, inf = np.nan, np.inf
    out = {}
    for n, (name, field) in enumerate(fields().items()):
        ni = 150 if name != "33x17" else 260
        pl, pts = crowd(field, ni, 11 + n)
        drop = np.random.RandomState(70 + n).uniform(-0.3, 0.0, ni).astype(F)
        drop[5::11] = 0.0
        pl[0, 0], pl[1, 0], pl[2, 2], pl[3, 2], pl[4, 0] = nan, inf, nan, -inf, -inf      # the placement's sample fails (h0 fails)
        pl[5, 1], pl[6, 1], pl[7, 1] = nan, inf, -inf                                      # ty
        drop[8], drop[9], drop[10] = nan, inf, -inf
        pts[:, 11, 0] = nan                                                # every foot fails
        pts[:, 12, 2] = inf
        pts[0, 13, 0], pts[1, 14, 2], pts[0, 15, 0], pts[1, 16, 2] = nan, nan, -inf, inf   # one foot fails (of 2 and of 8; of 1: all)
        pts[0, 17, 1], pts[1, 18, 1], pts[0, 19, 1] = nan, inf, -inf       # P.y: the sample succeeds, the target is zero
        pl[20, 1] -= 50.0                                                  # the ground far above the placement: dy clamped up
        pl[21, 1] += 50.0
        pts[:, 22, 1] += 1e30                                              # (a huge animated height stays itself)
        pl[23, 1] = 0.0
        calls = []
        for nf in (1, 2, 8):
            calls.append(dict(kind="targets", n_feet=nf, max_step=0.35, max_drop=0.2, want_drop=True))
            calls.append(dict(kind="targets", n_feet=nf, max_step=0.0, max_drop=0.0, want_drop=True))
            calls.append(dict(kind="targets", n_feet=nf, max_step=100.0, max_drop=100.0, want_drop=nf == 2))
        calls.append(dict(kind="place", with_drop=True, y_offset=0.125))
        calls.append(dict(kind="place", with_drop=False, y_offset=-0.3))
        out[name] = dict(field=field, placements=pl, points=pts, drop=drop, calls=calls)
    return out


def run_calls(case, count=None, ids=None):
    """Every call of a case through the restatement -> per call (placements,) or (targets, drop or None)."""
    got = []
    for c in case["calls"]:
        if c["kind"] == "place":
            got.append((place(case["field"], case["placements"], case["drop"] if c["with_drop"] else None, c["y_offset"], ids=ids, count=count),))
        else:
            got.append(targets(case["field"], case["placements"], case["points"][:c["n_feet"]], c["max_step"], c["max_drop"], c["want_drop"],
                               ids=ids, count=count))
    return got


# ------------------------------------------------------------------------------------------------ the CPU driver ---------------
def build_driver(sanitize=False):
    return hp.build("ground_math_driver", [os.path.join(hp.TESTS, "ground_math_driver.cpp"), os.path.join(hp.CSRC, "error.cpp")],
                    sanitize=sanitize)


def run_driver(exe, case):
    """Every call of a case through the host build -> ((min_height, max_height), per call what run_calls gives)."""
    field, calls = case["field"], case["calls"]
    pl, ni = np.ascontiguousarray(case["placements"], F), case["placements"].shape[0]

    def write(f):
        f.write(struct.pack("<3I", field["nx"], field["nz"], len(calls)))
        f.write(np.array([field["origin"][0], field["origin"][1], field["cell"][0], field["cell"][1]], F).tobytes())
        f.write(field["H"].tobytes())
        for c in calls:
            if c["kind"] == "place":
                f.write(struct.pack("<4I2f", 0, ni, 0, int(c["with_drop"]), c["y_offset"], 0.0))
                f.write(pl.tobytes())
                if c["with_drop"]:
                    f.write(np.ascontiguousarray(case["drop"], F).tobytes())
            else:
                f.write(struct.pack("<4I2f", 1, ni, c["n_feet"], int(c["want_drop"]), c["max_step"], c["max_drop"]))
                f.write(pl.tobytes())
                f.write(np.ascontiguousarray(case["points"][:c["n_feet"]], F).tobytes())

    def read(f):
        take = lambda *shape: np.frombuffer(f.read(int(np.prod(shape)) * 4), F).reshape(shape).copy()      # noqa: E731
        lo_hi = take(2)
        got = []
        for c in calls:
            if c["kind"] == "place":
                got.append((take(ni, 8),))
            else:
                got.append((take(c["n_feet"], ni, 4), take(ni) if c["want_drop"] else None))
        return lo_hi, got
    return hp.run_files(exe, write, read)


def plan(cells, exe):
    """The planner of csrc/ground_table.hpp through the driver: [cells] -> [(threads, nblocks)]."""
    out = hp.run(exe, ["plan"], stdin="".join("%d\n" % c for c in cells)).stdout
    return [tuple(int(v) for v in line.split()) for line in out.splitlines()]

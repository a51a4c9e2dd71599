"""mmdx_palette_reach restated in numpy from the text of include/mmdx.h (steps 0-6), binary32 throughout, one operation per line of
the header; the table builder of mmdx_reach_set_create; the rig and the generated case table the CPU driver
(tests/reach_math_driver.cpp) and the gfx950 kernel are held to, bit for bit.  Nothing here needs a GPU or the library."""
import os
import struct

import numpy as np

from tests import host_program as hp
from tests.aim_ref import aim_rig, assert_same, finite, fk_palettes, is_under, mul, pt  # noqa: F401  (the aim section's notation)
from tests.aim_ref import direction as dir_

HERE = os.path.dirname(os.path.abspath(__file__))
F = np.float32
U = np.uint32
MAX_REACHES, KEEP_END_ROTATION = 16, 1
# every branch of the header's steps 0-6 and every kind of input the issue names: what a case table must contain
CASES = ("w_zero", "w_negative", "w_nan", "w_above_1", "w_fraction", "target_not_finite", "target_on_a", "beyond_lmax", "inside_lmin",
         "within_range", "lmin_above_lmax", "y2_not_positive", "y2_positive", "pole_taken", "pole_along_dh", "u1_equals_v1",
         "antiparallel_step_3", "antiparallel_step_4", "flag_keep", "flag_plain", "indirect_b", "indirect_c", "tip_off_pivot",
         "nan_row_a", "nan_row_b", "nan_row_c", "scaled_placement", "applied", "not_applied", "row_written", "row_not_written")


# ------------------------------------------------------------------------------------------------ the table -------------------
def make_reach(a, b, c, tip_point=None, pole=(0.0, 0.0, -1.0), max_extension=1.0, flags=0):
    return dict(bones=(int(a), int(b), int(c)), tip_point=tip_point, pole=np.asarray(pole, F), max_extension=F(max_extension),
                flags=int(flags))


def build_table(parent, rest, reaches):
    """What mmdx_reach_set_create builds (csrc/reach_table.hpp), for valid input: a list of dict(a, b, c, ha, hb, hc, e, pole,
    max_extension, flags, rows = [(bone, depth)] in ascending bone order)."""
    parent = np.asarray(parent, np.int64)
    rest = np.asarray(rest, F).reshape(-1, 3)
    out = []
    for r in reaches:
        a, b, c = r["bones"]
        rows = []
        for s in range(len(parent)):
            if is_under(parent, a, s):
                rows.append((s, 2 if is_under(parent, c, s) else 1 if is_under(parent, b, s) else 0))
        e = rest[c] if r["tip_point"] is None else np.asarray(r["tip_point"], F)
        out.append(dict(a=a, b=b, c=c, ha=rest[a].copy(), hb=rest[b].copy(), hc=rest[c].copy(), e=e.astype(F), pole=np.asarray(r["pole"], F),
                        max_extension=F(r["max_extension"]), flags=r["flags"], rows=rows,
                        indirect_b=parent[b] != a, indirect_c=parent[c] != b))
    return out


# ------------------------------------------------------------------------------------------------ the arithmetic --------------
def length(d):
    s = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    return np.sqrt(s.astype(np.float64)).astype(d.dtype)


def dot(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def _bump(count, key, n):
    count[key] = count.get(key, 0) + int(n)


def rot(u, v, hh):
    """rot(u, v, H) for N instances: -> (matrix [N,16], ok [N], m [N])."""
    ft = u.dtype.type
    n = u.shape[0]
    same = (u == v).all(axis=1)
    cs = dot(u, v)
    k0 = u[:, 1] * v[:, 2] - u[:, 2] * v[:, 1]
    k1 = u[:, 2] * v[:, 0] - u[:, 0] * v[:, 2]
    k2 = u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]
    m = ft(1.0) + cs
    ok = same | (m > ft(F(1e-6)))
    q00, q01, q02, q11, q12, q22 = (k0 * k0) / m, (k0 * k1) / m, (k0 * k2) / m, (k1 * k1) / m, (k1 * k2) / m, (k2 * k2) / m
    r = [[cs + q00, q01 + k2, q02 - k1], [q01 - k2, cs + q11, q12 + k0], [q02 + k1, q12 - k0, cs + q22]]
    ml = np.zeros((n, 16), u.dtype)
    for i in range(3):
        for j in range(3):
            ml[:, 4 * i + j] = r[i][j]
    for j in range(3):
        ml[:, 12 + j] = hh[:, j] - ((hh[:, 0] * r[0][j] + hh[:, 1] * r[1][j]) + hh[:, 2] * r[2][j])
    ml[:, 15] = 1.0
    ident = np.tile(np.eye(4, dtype=u.dtype).reshape(16), (n, 1))
    return np.where(same[:, None], ident, ml), ok, np.where(same, ft(2.0), m)


def solve(ra, rb, rc, k, g, w, count, trace=None):
    """Steps 1-5 for reach k of N instances at once.  ra, rb, rc [N,16]; g [N,3]; w [N] (after step 0).  -> (c0, c1, c2 [N,16],
    ok [N])."""
    ft = ra.dtype.type
    keep = bool(k["flags"] & KEEP_END_ROTATION)
    ha, hb, hc, e, pole = (k[x].astype(ft) for x in ("ha", "hb", "hc", "e", "pole"))
    A, B, K, T = pt(ha, ra), pt(hb, rb), pt(hc, rc), pt(e, rc)                                       # 1. points
    _bump(count, "nan_row_a", np.isnan(ra).any(axis=1).sum())
    _bump(count, "nan_row_b", np.isnan(rb).any(axis=1).sum())
    _bump(count, "nan_row_c", np.isnan(rc).any(axis=1).sum())
    if keep:
        G = g - (T - K)
        T = K
    else:
        G = g
    Gw = np.where((w >= 1)[:, None], G, T + (G - T) * w[:, None])
    ba, tb, dv = B - A, T - B, Gw - A
    l1, l2, d = length(ba), length(tb), length(dv)
    ok = (l1 > 0) & (l2 > 0) & (d > 0) & finite(l1) & finite(l2) & finite(d)
    _bump(count, "target_on_a", ((l1 > 0) & (l2 > 0) & (d == 0)).sum())
    s = l1 + l2                                                                                      # 2. clamp
    lmax = s * ft(k["max_extension"])
    lmin = np.abs(l1 - l2) + (s - lmax)
    bad = ok & ~(lmin <= lmax)
    _bump(count, "lmin_above_lmax", bad.sum())
    ok &= ~bad
    _bump(count, "inside_lmin", (ok & (d < lmin)).sum())
    _bump(count, "beyond_lmax", (ok & (d > lmax)).sum())
    _bump(count, "within_range", (ok & ~(d < lmin) & ~(d > lmax)).sum())
    dc = np.where(d < lmin, lmin, d)
    dc = np.where(dc > lmax, lmax, dc)
    dh = dv / d[:, None]
    Gc = A + dh * dc[:, None]
    x = ((l1 * l1 - l2 * l2) + dc * dc) / (ft(2.0) * dc)                                             # 3. elbow
    y2 = l1 * l1 - x * x
    y = np.where(y2 > 0, np.sqrt(np.where(y2 > 0, y2, 0).astype(np.float64)).astype(ra.dtype), ft(0.0))
    _bump(count, "y2_not_positive", (ok & ~(y2 > 0)).sum())
    _bump(count, "y2_positive", (ok & (y2 > 0)).sum())
    p = ba - dh * dot(ba, dh)[:, None]
    lp = length(p)
    straight = ~(lp > ft(F(1e-4)) * l1)
    _bump(count, "pole_taken", (ok & straight).sum())
    b2 = dir_(pole, ra)
    p2 = b2 - dh * dot(b2, dh)[:, None]
    lp2 = length(p2)
    p, lp = np.where(straight[:, None], p2, p), np.where(straight, lp2, lp)
    bad = ok & straight & ~(lp > 0)
    _bump(count, "pole_along_dh", bad.sum())
    ok &= ~bad
    nb = dh * x[:, None] + (p / lp[:, None]) * y[:, None]
    v1 = nb / length(nb)[:, None]
    u1 = ba / l1[:, None]
    _bump(count, "u1_equals_v1", (ok & (u1 == v1).all(axis=1)).sum())
    c0, ok_a, m_a = rot(u1, v1, A)
    _bump(count, "antiparallel_step_3", (ok & ~ok_a).sum())
    ok &= ok_a
    B1 = pt(hb, mul(rb, c0))                                                                         # 4. forearm
    T1 = pt(hc if keep else e, mul(rc, c0))
    t1, g1 = T1 - B1, Gc - B1
    lt, lg = length(t1), length(g1)
    ok &= (lt > 0) & (lg > 0) & finite(lt) & finite(lg)
    u2, v2 = t1 / lt[:, None], g1 / lg[:, None]
    mb, ok_b, m_b = rot(u2, v2, B1)
    _bump(count, "antiparallel_step_4", (ok & ~ok_b).sum())
    ok &= ok_b
    c1 = mul(c0, mb)
    c1[:, [3, 7, 11]], c1[:, 15] = 0.0, 1.0
    if keep:                                                                                         # 5. end bone
        K1 = pt(hc, mul(rc, c1))
        c2 = np.tile(np.eye(4, dtype=ra.dtype).reshape(16), (ra.shape[0], 1))
        c2[:, 12:15] = K1 - K
    else:
        c2 = c1.copy()
    _bump(count, "applied", ok.sum())
    _bump(count, "not_applied", (~ok).sum())
    with np.errstate(all="ignore"):
        det = np.linalg.det(ra[:, [0, 1, 2, 4, 5, 6, 8, 9, 10]].reshape(-1, 3, 3).astype(np.float64))
    _bump(count, "scaled_placement", (ok & (np.abs(det - 1.0) > 0.2)).sum())
    if trace is not None:
        trace.append(dict(ok=ok, A=A, Gc=Gc, l1=l1, l2=l2, dh=dh, bend=p / lp[:, None], m_a=m_a, m_b=m_b, c0=c0, c1=c1))
    return c0, c1, c2, ok


def reach(table, pal, targets, ids=None, count=None, ft=F, trace=None):
    """One mmdx_palette_reach: pal f32 [NI,NB,16], targets f32 [NI,4] or [4] (one for everyone) -> the new pal (binary32, or ft);
    the inputs are left alone.  ids: the instances reached (None = all).  count: a dict that collects how often every case of CASES
    was taken.  trace: a list that receives, per reach, the intermediate values of the live instances."""
    count = {} if count is None else count
    pal = np.array(pal, F)
    rows = np.arange(pal.shape[0]) if ids is None else np.asarray(ids, np.int64)
    out = pal.astype(ft)
    if rows.size == 0:
        return out
    tgt = np.broadcast_to(np.asarray(targets, F).reshape(-1, 4), (pal.shape[0], 4))[rows]
    with np.errstate(all="ignore"):
        w = tgt[:, 3]
        dead = ~(w > 0) | ~finite(tgt).all(axis=1)
        _bump(count, "w_zero", (w == 0).sum())
        _bump(count, "w_negative", (w < 0).sum())
        _bump(count, "w_nan", np.isnan(w).sum())
        _bump(count, "w_above_1", (w > 1).sum())
        _bump(count, "w_fraction", (~dead & (w < 1)).sum())
        _bump(count, "target_not_finite", (~finite(tgt[:, :3]).all(axis=1)).sum())
        live = np.nonzero(~dead)[0]
        if live.size == 0:
            return out
        src = pal[rows[live]].astype(ft)
        g, w = tgt[live, :3].astype(ft), np.minimum(tgt[live, 3], F(1.0)).astype(ft)
        new = src.copy()
        for k in table:
            c0, c1, c2, ok = solve(src[:, k["a"]], src[:, k["b"]], src[:, k["c"]], k, g, w, count, trace)
            _bump(count, "flag_keep" if k["flags"] & KEEP_END_ROTATION else "flag_plain", 1)
            _bump(count, "indirect_b", k["indirect_b"])
            _bump(count, "indirect_c", k["indirect_c"])
            _bump(count, "tip_off_pivot", (k["e"] != k["hc"]).any())
            cs = (c0, c1, c2)
            for b, depth in k["rows"]:
                new[:, b] = np.where(ok[:, None], mul(src[:, b], cs[depth]), src[:, b])
                _bump(count, "row_written", ok.sum())
                _bump(count, "row_not_written", (~ok).sum())
        out[rows[live]] = new
    return out


def live_rows(pal, targets):
    """The instances step 0 lets through, as reach() orders its trace."""
    tgt = np.broadcast_to(np.asarray(targets, F).reshape(-1, 4), (pal.shape[0], 4))
    with np.errstate(all="ignore"):
        return np.nonzero((tgt[:, 3] > 0) & finite(tgt).all(axis=1))[0]


# ------------------------------------------------------------------------------------------------ rigs and palettes ------------
def reach_rig():
    """The 41-bone humanoid of aim_ref.aim_rig with three limbs on exact coordinates, so that identity rows give exact cases:
      10 -> 11 -> 12 -> 13 (+ 32..35 fingers below 13)  a straight right arm along +x, 11 a twist bone: non-contiguous subtree of 8
      14 -> 15 -> 16 -> 17                              a straight left arm along -x, upper bone 1, forearm 3.5 to the tip
      18 -> 19 -> 20                                    a leg with a bent knee
      36 -> 37 -> 38                                    a leg whose foot is very short
    -> (parent i32 [41], rest f32 [41,3])."""
    parent, rest = aim_rig()
    rest = rest.copy()
    rest[10], rest[11], rest[12], rest[13] = (1, 5, 0), (2, 5, 0), (3, 5, 0), (5, 5, 0)
    for b in (32, 33, 34, 35):
        rest[b] = rest[13] + np.array([0.25, 0.05 * (b - 33), 0.0], F)
    rest[14], rest[15], rest[16], rest[17] = (-1, 5, 0), (-2, 5, 0), (-3, 5, 0), (-5, 5, 0)
    rest[18], rest[19], rest[20] = (0.5, 3, 0), (0.5, 1.75, -0.25), (0.5, 0, 0)
    rest[36], rest[37], rest[38] = (-0.5, 3, 0), (-0.5, 0, 0), (-0.5, -0.25, 0)
    return parent, rest.astype(F)


def rig_sets():
    """The reach sets of the rig the tests use: name -> reaches.  Subtrees of 3 (a, b, c alone), 4, 8, 11, 26 and 37 rows."""
    _, rest = reach_rig()
    return {
        "arm": [make_reach(10, 12, 13, max_extension=0.98)],                                                 # a twist bone between a and b, 8 rows
        "leg3": [make_reach(18, 19, 20, tip_point=rest[20] + np.array([0.0, -0.1, -0.2], F), pole=(0, 0, -1), max_extension=0.95,
                            flags=KEEP_END_ROTATION)],                                                        # a, b, c alone
        "arm4": [make_reach(14, 15, 17, tip_point=(-5.5, 5, 0), pole=(0, -1, 0))],                            # 4 rows, c no direct child
        "head11": [make_reach(7, 24, 26, max_extension=0.9)],                                                 # 11 rows
        "body26": [make_reach(4, 5, 10, pole=(1, 0, 0), max_extension=0.97)],                                 # 26 rows
        "all37": [make_reach(1, 3, 18, pole=(0, 0, 1), flags=KEEP_END_ROTATION)],                             # 37 rows
        "limbs": [make_reach(10, 12, 13, max_extension=0.98), make_reach(14, 15, 17, tip_point=(-5.5, 5, 0), pole=(0, -1, 0)),
                  make_reach(18, 19, 20, tip_point=rest[20] + np.array([0.0, -0.1, -0.2], F), max_extension=0.95, flags=KEEP_END_ROTATION),
                  make_reach(36, 37, 38)],                                                                    # 4 reaches
    }


def tip_now(k, pal):
    """The solved point of reach k under palettes pal [N,NB,16], in float64: the tip, or the pivot of c with the flag."""
    x = k["hc"] if k["flags"] & KEEP_END_ROTATION else k["e"]
    return pt(x.astype(np.float64), pal[:, k["c"]].astype(np.float64))


def near_targets(k, pal, seed, spread=1.5, weight=1.0):
    """[N,4]: a target per instance around where the tip of reach k is under pal: some in reach, some beyond, some very close."""
    rng = np.random.RandomState(seed)
    n = pal.shape[0]
    off = rng.uniform(-1.0, 1.0, (n, 3)) * (spread * rng.uniform(0.05, 1.0, (n, 1)) ** 2)
    return np.concatenate([pt(k["e"].astype(np.float64), pal[:, k["c"]].astype(np.float64)) + off, np.full((n, 1), weight)], axis=1).astype(F)


def circling_targets(k, ni, radius_lo=0.05, radius_hi=1.3):
    """[NI,4]: step s of a target circling the rest pivot of a of reach k, its distance sweeping from inside lmin to beyond lmax of
    the rest limb, weight 1."""
    s = np.arange(ni)
    full = float(np.linalg.norm(k["hb"] - k["ha"]) + np.linalg.norm(k["e"] - k["hb"]))
    rad = full * (radius_lo + (radius_hi - radius_lo) * (0.5 + 0.5 * np.sin(0.0171 * s)))
    ang, tilt = 0.013 * s, 0.9 * np.sin(0.0047 * s)
    dirs = np.stack([np.cos(ang) * np.cos(tilt), np.sin(tilt), np.sin(ang) * np.cos(tilt)], axis=1)
    return np.concatenate([k["ha"].astype(np.float64) + dirs * rad[:, None], np.ones((ni, 1))], axis=1).astype(F)


def placed(pal, scale=1.0, seed=3):
    """pal [N,NB,16] times one placement per instance: a turn about y, a uniform scale, a translation; float64 rounded once."""
    rng = np.random.RandomState(seed)
    n = pal.shape[0]
    ang = rng.uniform(-3, 3, n)
    m = np.zeros((n, 4, 4))
    m[:, 0, 0], m[:, 0, 2], m[:, 2, 0], m[:, 2, 2], m[:, 1, 1] = np.cos(ang), -np.sin(ang), np.sin(ang), np.cos(ang), 1.0
    m[:, :3, :3] *= scale
    m[:, 3, :3], m[:, 3, 3] = rng.uniform(-20, 20, (n, 3)), 1.0
    return (pal.reshape(n, -1, 4, 4).astype(np.float64) @ m[:, None]).reshape(pal.shape).astype(F), m


# ------------------------------------------------------------------------------------------------ the case table ---------------
def case_table(ni=32):
    """dict(parent, rest, reaches, table, pal [NI,NB,16], targets [NI,4]) on the rig, four reaches:
      R0 (10, 12, 13)  straight along +x, l1 = l2 = 2, no limit on the extension, b no direct child
      R1 (18, 19, 20)  a bent leg, KEEP_END_ROTATION, a toe point off the pivot, extension 0.9
      R2 (14, 15, 17)  straight along -x, l1 = 1, l2 = 3.5 to a tip off the pivot, c no direct child
      R3 (36, 37, 38)  l1 = 3, l2 = 0.25, extension 0.5: lmin > lmax, never written
    Every branch CASES names is taken by some instance:
      0..7    swaying rows, targets near the hand of weight 1, 0.5, 2 (above 1), 0, -1, NaN, and with an infinite and a NaN coordinate
      8..17   identity rows (every pivot on its rest position exactly): R0's target on A; far along +x (beyond lmax, y2 = 0, the pole
              taken, u1 == v1 and u2 == v2: the identity); along +x in range (the pole bends the elbow); the same with row a turned
              so that the pole lies along dh; R2's target inside lmin along the upper bone (x = -l1: antiparallel in step 3) and on
              the other side of A (v1 == u1, then antiparallel in step 4); R1's target inside lmin; a target within R1's range
      18..21  a NaN in the row of a, of b, of c, and in the fourth column of the row of a (no point reads it: the rows of a's
              depth get it)
      22..    swaying rows of other steps under scaled placements, weights in (0, 1)"""
    parent, rest = reach_rig()
    reaches = [make_reach(10, 12, 13), make_reach(18, 19, 20, tip_point=rest[20] + np.array([0.0, -0.125, -0.25], F), max_extension=0.9,
                                                  flags=KEEP_END_ROTATION),
               make_reach(14, 15, 17, tip_point=(-5.5, 5, 0)), make_reach(36, 37, 38, max_extension=0.5)]
    table = build_table(parent, rest, reaches)
    nb = len(parent)
    pal = fk_palettes(parent, rest, ni, step=3)
    targets = near_targets(table[0], pal, 5)
    targets[1, 3], targets[2, 3], targets[3, 3], targets[4, 3], targets[5, 3] = 0.5, 2.0, 0.0, -1.0, np.nan
    targets[6, 0], targets[7, 1] = np.inf, np.nan
    ident = np.tile(np.eye(4, dtype=F).reshape(16), (nb, 1))
    pal[8:18] = ident
    targets[8] = [1, 5, 0, 1]                                           # R0: on A
    targets[9] = [9, 5, 0, 1]                                           # R0: far along the limb
    targets[10] = [4, 5, 0, 1]                                          # R0: along the limb, in range: the pole
    targets[11] = [4, 5, 0, 1]                                          # R0: ... and the pole along dh
    turn = np.array([[0, 0, 1], [0, 1, 0], [-1, 0, 0]], F)              # row vectors: (0, 0, -1) -> (1, 0, 0)
    pal[11, 10, [0, 1, 2, 4, 5, 6, 8, 9, 10]] = turn.reshape(9)
    pal[11, 10, 12:15] = rest[10] - rest[10] @ turn
    targets[12] = [-1.5, 5, 0, 1]                                       # R2: inside lmin, along the upper bone
    targets[13] = [-0.5, 5, 0, 1]                                       # R2: inside lmin, on the other side of A
    targets[14] = [0.5, 2.875, 0.0625, 1]                               # R1: inside lmin
    targets[15] = [0.75, 1.0, -1.0, 1]                                  # R1: within its range
    targets[16] = [3.0, 6.0, -1.0, 0.75]                                # R0 within its range, a weight in (0, 1)
    targets[17] = [-2.0, 3.0, 1.0, 1]                                   # R2 within its range
    pal[18, 10, 1], pal[19, 12, 13], pal[20, 13, 6], pal[21, 10, 7] = np.nan, np.nan, np.nan, np.nan
    sway = fk_palettes(parent, rest, ni - 22, step=40, amplitude=0.9)
    scales = np.linspace(0.5, 2.0, ni - 22)
    pal[22:], _ = placed(sway, scale=scales[:, None, None], seed=9)
    for i in range(22, ni):                                             # a target near the hand or foot of R0, R1, R2 in turn
        t = tip_now(table[(i - 22) % 3], pal[i:i + 1])[0] + np.array([0.3, -0.2, 0.25]) * scales[i - 22]
        targets[i] = [*t, 1.0]
    targets[22:27, 3] = np.linspace(0.1, 0.9, 5).astype(F)
    return dict(parent=parent, rest=rest, reaches=reaches, table=table, pal=pal, targets=targets)


# ------------------------------------------------------------------------------------------------ the CPU driver ---------------
def build_driver(sanitize=False):
    return hp.build("reach_math_driver", [os.path.join(hp.TESTS, "reach_math_driver.cpp"), os.path.join(hp.CSRC, "error.cpp")],
                    sanitize=sanitize)


def desc_arrays(reaches, rest):
    """The arrays of an mmdx_reach_set_desc for `reaches`: (bones [NR,3], tip_point, pole [NR,3], max_extension, flags [NR])."""
    rest = np.asarray(rest, F).reshape(-1, 3)
    bones = np.array([r["bones"] for r in reaches], U).reshape(-1, 3)
    tip = np.stack([rest[r["bones"][2]] if r["tip_point"] is None else np.asarray(r["tip_point"], F) for r in reaches]).astype(F)
    pole = np.stack([np.asarray(r["pole"], F) for r in reaches]).astype(F)
    ext = np.array([r["max_extension"] for r in reaches], F)
    flags = np.array([r["flags"] for r in reaches], U)
    return tuple(np.ascontiguousarray(a) for a in (bones, tip, pole, ext, flags))


def run_driver(exe, parent, rest, reaches, calls):
    """calls = [(pal [NI,NB,16], targets [NI,4])] -> (table as the driver built it: per reach dict(h [3,3], rows), [pal after each
    call])."""
    parent, rest = np.asarray(parent, np.int32), np.asarray(rest, F)
    arrays = desc_arrays(reaches, rest)
    nb, nr, ni = parent.size, len(reaches), calls[0][0].shape[0]

    def write(f):
        f.write(struct.pack("<4I", nb, nr, ni, len(calls)))
        for a in (parent, rest) + arrays:
            f.write(np.ascontiguousarray(a).tobytes())
        for pal, tgt in calls:
            f.write(np.ascontiguousarray(pal, F).tobytes())
            f.write(np.ascontiguousarray(np.broadcast_to(np.asarray(tgt, F).reshape(-1, 4), (ni, 4))).tobytes())

    def read(f):
        take = lambda dt, *shape: np.frombuffer(f.read(int(np.prod(shape)) * 4), dt).reshape(shape).copy()      # noqa: E731
        tb = []
        for _ in reaches:
            n_rows = int(take(U, 1)[0])
            tb.append(dict(h=take(F, 3, 3), rows=[tuple(r) for r in take(U, n_rows, 2).tolist()]))
        return tb, [take(F, ni, nb, 16) for _ in calls]
    return hp.run_files(exe, write, read)


def plan(cells, exe):
    """The planner of csrc/reach_table.hpp through the driver: [cells] -> [(block, threads, nblocks, lds)]."""
    out = hp.run(exe, ["plan"], stdin="".join("%d\n" % c for c in cells)).stdout
    return [tuple(int(v) for v in line.split()) for line in out.splitlines()]

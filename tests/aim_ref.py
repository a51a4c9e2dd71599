"""mmdx_palette_aim restated in numpy from the text of include/mmdx.h (steps 0-2), binary32 throughout, one operation per line of the
header (ft=np.float64 evaluates the same formulas in binary64, for the tolerances); the table builder of mmdx_aim_set_create; the
rigs and the generated case table the CPU driver (tests/aim_math_driver.cpp) and the gfx950 kernel are held to, bit for bit.  Nothing
here needs a GPU or the library."""
import os
import struct

import numpy as np

from tests import host_program as hp

HERE = os.path.dirname(os.path.abspath(__file__))
F = np.float32
U = np.uint32
MAX_AIMS, MAX_LINKS = 16, 4
# every branch of the header's steps 0-2: what a case table must contain
CASES = ("w_zero", "w_negative", "w_nan", "w_above_1", "target_not_finite", "la_degenerate", "target_on_eye", "u_equals_v", "t_ge_1",
         "t_lt_1", "blend_degenerate", "limit_hit", "limit_not_hit", "lp_degenerate", "antiparallel", "applied",
         "first_skipped_later_applied", "every_link_skipped", "eye_below_last_link", "indirect_link", "row_written", "row_not_written")


# ------------------------------------------------------------------------------------------------ the table -------------------
def is_under(parent, a, b):
    """b is a or below it, by the parent array alone (a value outside [0, NB) ends the walk; at most NB steps)."""
    nb, c = len(parent), int(b)
    for _ in range(nb + 1):
        if c == a:
            return True
        p = int(parent[c])
        if p < 0 or p >= nb:
            return False
        c = p
    return False


def make_aim(links, eye_bone=None, eye_point=None, forward=(0.0, 0.0, -1.0), shares=None, cos_limits=None):
    n = len(links)
    return dict(links=[int(b) for b in links], eye_bone=int(links[-1] if eye_bone is None else eye_bone), eye_point=eye_point,
                forward=np.asarray(forward, F), shares=np.asarray([1.0] * n if shares is None else shares, F),
                cos_limits=np.asarray([-1.0] * n if cos_limits is None else cos_limits, F))


def build_table(parent, rest, aims):
    """What mmdx_aim_set_create builds (csrc/aim_table.hpp), for valid input: a list of dict(bone [L], h [L,3], share, cos_limit,
    sin_limit [L], eye_bone, e, f, rows = [(bone, depth)] in ascending bone order)."""
    parent = np.asarray(parent, np.int64)
    rest = np.asarray(rest, F).reshape(-1, 3)
    out = []
    for a in aims:
        links = a["links"]
        cl = np.asarray(a["cos_limits"], F)
        sin = np.sqrt((F(1.0) - cl * cl).astype(np.float64)).astype(F)
        rows = []
        for b in range(len(parent)):
            if is_under(parent, links[0], b):
                rows.append((b, max(l for l, k in enumerate(links) if is_under(parent, k, b))))
        e = rest[a["eye_bone"]] if a["eye_point"] is None else np.asarray(a["eye_point"], F)
        out.append(dict(bone=np.asarray(links, U), h=rest[links].copy(), share=np.asarray(a["shares"], F), cos_limit=cl, sin_limit=sin,
                        eye_bone=a["eye_bone"], e=e.astype(F), f=np.asarray(a["forward"], F), rows=rows,
                        indirect=any(parent[links[l]] != links[l - 1] for l in range(1, len(links)))))
    return out


# ------------------------------------------------------------------------------------------------ the arithmetic --------------
def pt(x, s):
    """pt(x, S)[c] = ((x0*S[c] + x1*S[4+c]) + x2*S[8+c]) + 1.0f*S[12+c]: x [3], s [N,16] -> [N,3]."""
    one = s.dtype.type(1.0)
    return ((x[0] * s[:, 0:3] + x[1] * s[:, 4:7]) + x[2] * s[:, 8:11]) + one * s[:, 12:15]


def direction(x, s):
    return (x[0] * s[:, 0:3] + x[1] * s[:, 4:7]) + x[2] * s[:, 8:11]


def length(d):
    s = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    return np.sqrt(s.astype(np.float64)).astype(d.dtype)


def finite(x):
    return (x - x) == 0


def mul(a, b):
    """Matrix4x4::operator* per instance: a, b [N,16] -> [N,16], every element ((a1*b[c] + a2*b[4+c]) + a3*b[8+c]) + a4*b[12+c]."""
    o = np.empty_like(a)
    for r in range(4):
        for c in range(4):
            o[:, 4 * r + c] = ((a[:, 4 * r] * b[:, c] + a[:, 4 * r + 1] * b[:, 4 + c]) + a[:, 4 * r + 2] * b[:, 8 + c]) + a[:, 4 * r + 3] * b[:, 12 + c]
    return o


def _bump(count, key, n):
    count[key] = count.get(key, 0) + int(n)


def link(p_in, q_in, lk, l, e, f, g, w, c, is_set, count, trace=None):
    """Step 1 for link l of N instances at once.  p_in, q_in [N,16]; g [N,3]; w [N]; c [N,16] and is_set [N]: the cumulative matrix.
    -> (c, applied [N])."""
    ft = p_in.dtype.type
    p = np.where(is_set[:, None], mul(p_in, c), p_in)
    q = np.where(is_set[:, None], mul(q_in, c), q_in)
    hh, ee = pt(lk["h"][l].astype(ft), p), pt(e.astype(ft), q)
    a = direction(f.astype(ft), q)
    la = length(a)
    d = g - ee
    ld = length(d)
    skip = ~(la > 0) | ~(ld > 0) | ~finite(la) | ~finite(ld)
    _bump(count, "la_degenerate", (~(la > 0)).sum())
    _bump(count, "target_on_eye", ((la > 0) & (ld == 0)).sum())
    u, v = a / la[:, None], d / ld[:, None]
    same = (u == v).all(axis=1) & ~skip
    _bump(count, "u_equals_v", same.sum())
    skip |= same
    t = ft(lk["share"][l]) * w
    n = u + (v - u) * t[:, None]
    ln = length(n)
    full = t >= 1
    _bump(count, "t_ge_1", (full & ~skip).sum())
    _bump(count, "t_lt_1", (~full & ~skip).sum())
    blend_bad = ~full & ~(ln > 0) & ~skip
    _bump(count, "blend_degenerate", blend_bad.sum())
    skip |= blend_bad
    v2 = np.where(full[:, None], v, n / ln[:, None])
    cs = (u[:, 0] * v2[:, 0] + u[:, 1] * v2[:, 1]) + u[:, 2] * v2[:, 2]
    cl, sl = ft(lk["cos_limit"][l]), ft(lk["sin_limit"][l])
    hit = (cs < cl) & ~skip
    _bump(count, "limit_hit", hit.sum())
    _bump(count, "limit_not_hit", (~(cs < cl) & ~skip).sum())
    s = v2 - u * cs[:, None]
    lp = length(s)
    lp_bad = hit & ~(lp > 0)
    _bump(count, "lp_degenerate", lp_bad.sum())
    skip |= lp_bad
    v2 = np.where(hit[:, None], u * cl + (s / lp[:, None]) * sl, v2)
    cs = np.where(hit, (u[:, 0] * v2[:, 0] + u[:, 1] * v2[:, 1]) + u[:, 2] * v2[:, 2], cs)
    k0 = u[:, 1] * v2[:, 2] - u[:, 2] * v2[:, 1]
    k1 = u[:, 2] * v2[:, 0] - u[:, 0] * v2[:, 2]
    k2 = u[:, 0] * v2[:, 1] - u[:, 1] * v2[:, 0]
    m = ft(1.0) + cs
    anti = ~(m > ft(F(1e-6))) & ~skip
    _bump(count, "antiparallel", anti.sum())
    skip |= anti
    q00, q01, q02, q11, q12, q22 = (k0 * k0) / m, (k0 * k1) / m, (k0 * k2) / m, (k1 * k1) / m, (k1 * k2) / m, (k2 * k2) / m
    r = [[cs + q00, q01 + k2, q02 - k1], [q01 - k2, cs + q11, q12 + k0], [q02 + k1, q12 - k0, cs + q22]]
    ml = np.zeros_like(p_in)
    for i in range(3):
        for j in range(3):
            ml[:, 4 * i + j] = r[i][j]
    for j in range(3):
        ml[:, 12 + j] = hh[:, j] - ((hh[:, 0] * r[0][j] + hh[:, 1] * r[1][j]) + hh[:, 2] * r[2][j])
    ml[:, 15] = 1.0
    prod = mul(c, ml)
    prod[:, [3, 7, 11]], prod[:, 15] = 0.0, 1.0
    new = np.where(is_set[:, None], prod, ml)
    applied = ~skip
    _bump(count, "applied", applied.sum())
    if trace is not None:
        trace.append(dict(u=u, v=v, v2=v2, r=np.stack([np.stack(x, axis=1) for x in r], axis=1), hh=hh, applied=applied, m=m))
    return np.where(applied[:, None], new, c), applied


def aim(table, pal, targets, ids=None, count=None, ft=F, trace=None):
    """One mmdx_palette_aim: pal f32 [NI,NB,16], targets f32 [NI,4] or [4] (one for everyone) -> the new pal (binary32, or ft); the
    inputs are left alone.  ids: the instances aimed (None = all).  count: a dict that collects how often every case of CASES was
    taken.  trace: a list that receives, per (aim, link), the intermediate vectors."""
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
        _bump(count, "target_not_finite", (~finite(tgt[:, :3]).all(axis=1)).sum())
        live = np.nonzero(~dead)[0]
        if live.size == 0:
            return out
        src = pal[rows[live]].astype(ft)
        g, w = tgt[live, :3].astype(ft), np.minimum(tgt[live, 3], F(1.0)).astype(ft)
        new = src.copy()
        for a in table:
            c, is_set, cs = np.zeros((live.size, 16), ft), np.zeros(live.size, bool), []
            for l in range(len(a["bone"])):
                c, applied = link(src[:, a["bone"][l]], src[:, a["eye_bone"]], a, l, a["e"], a["f"], g, w, c, is_set, count, trace)
                _bump(count, "first_skipped_later_applied", (applied & ~is_set).sum() if l > 0 else 0)
                is_set = is_set | applied
                cs.append((c, is_set))
            _bump(count, "every_link_skipped", (~is_set).sum())
            _bump(count, "eye_below_last_link", a["eye_bone"] != a["bone"][-1])
            _bump(count, "indirect_link", a["indirect"])
            for b, depth in a["rows"]:
                cd, sd = cs[depth]
                new[:, b] = np.where(sd[:, None], mul(src[:, b], cd), src[:, b])
                _bump(count, "row_written", sd.sum())
                _bump(count, "row_not_written", (~sd).sum())
        out[rows[live]] = new
    return out


def forward_now(a, pal):
    """The unit forward direction of aim `a` under palettes pal [N,NB,16], in float64."""
    q = pal[:, a["eye_bone"]].astype(np.float64)
    d = direction(a["f"].astype(np.float64), q)
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def to_target(a, pal, targets):
    """The unit direction from the eye of aim `a` under pal to the targets [N,4], in float64."""
    q = pal[:, a["eye_bone"]].astype(np.float64)
    d = np.asarray(targets, np.float64)[:, :3] - pt(a["e"].astype(np.float64), q)
    return d / np.linalg.norm(d, axis=1, keepdims=True)


# ------------------------------------------------------------------------------------------------ rigs and palettes ------------
def aim_rig():
    """A 41-bone humanoid: 0 root; 1 centre (its subtree: 1 and 3..38, 37 bones, bone 2 is not in it); 2 a stray bone with the one
    child 39; 40 a leaf of the root.  4 upper body, 5 upper body 2, 6 neck, 7 head, 8-9 eyes, 24-31 a hair chain on the head: the
    head's subtree {7, 8, 9, 24..31} has non-contiguous indices.  -> (parent i32 [41], rest f32 [41,3])."""
    parent = [-1, 0, 0, 1, 1, 4, 5, 6, 7, 7, 5, 10, 11, 12, 5, 14, 15, 16, 3, 18, 19, 3, 21, 22, 7, 24, 25, 26, 27, 28, 29, 30, 13, 13,
              13, 13, 3, 36, 37, 2, 0]
    rng = np.random.RandomState(41)
    rest = np.zeros((41, 3))
    rest[0] = [0.0, 0.0, 0.0]
    for b in range(1, 41):
        rest[b] = rest[parent[b]] + rng.uniform(-0.6, 0.6, 3) + [0.0, 0.9 if b in (1, 4, 5, 6, 7) else 0.1, 0.0]
    rest[8], rest[9] = rest[7] + [0.3, 0.4, -0.8], rest[7] + [-0.3, 0.4, -0.8]
    return np.array(parent, np.int32), rest.astype(F)


# the aim sets of the rig the tests use: name -> aims
def rig_sets():
    return {
        "head": [make_aim([7], eye_bone=8, shares=[1.0], cos_limits=[0.5])],                                     # L = 1, 11 rows
        "neck_head": [make_aim([5, 7], shares=[0.5, 1.0], cos_limits=[0.8, 0.3])],                               # L = 2, 5 -> 6 -> 7
        "spine": [make_aim([4, 5, 6, 7], eye_bone=9, shares=[0.2, 0.3, 0.5, 1.0], cos_limits=[0.9, 0.9, 0.7, 0.0],
                           forward=(0.1, 0.0, -2.0))],                                                         # L = 4
        "sizes": [make_aim([1], eye_bone=7, shares=[0.7]), make_aim([2], eye_bone=39, forward=(1.0, 0.0, 0.0)),
                  make_aim([40], forward=(0.0, 1.0, 0.0), cos_limits=[0.6])],                                    # subtrees of 37, 2 and 1
        "mixed": [make_aim([4, 5, 6, 7], eye_bone=8, shares=[0.25, 0.25, 0.5, 1.0], cos_limits=[0.95, 0.9, 0.8, 0.5]),
                  make_aim([18, 20], shares=[0.5, 1.0], forward=(0.0, -1.0, 0.0)), make_aim([40], eye_point=(0.0, 0.0, 0.0))],
    }


def rigid_rows(rng, n, spread=3.0, scale=None):
    """n skinning-like rows: a rotation (times a per-row scale), a translation, last column 0 0 0 1."""
    q = rng.normal(size=(n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    x, y, z, w = q.T
    r = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y + z * w), 2 * (x * z - y * w),
                  2 * (x * y - z * w), 1 - 2 * (x * x + z * z), 2 * (y * z + x * w),
                  2 * (x * z + y * w), 2 * (y * z - x * w), 1 - 2 * (x * x + y * y)], axis=1).reshape(n, 3, 3)
    if scale is not None:
        r = r * scale[:, None, None]
    m = np.zeros((n, 4, 4))
    m[:, :3, :3], m[:, 3, :3], m[:, 3, 3] = r, rng.uniform(-spread, spread, (n, 3)), 1.0
    return m.reshape(n, 16).astype(F)


def _rot(axis, ang):
    """Row-vector rotation matrices [N,3,3] about unit axes [N,3] by angles [N]."""
    x, y, z = axis.T
    c, s = np.cos(ang), np.sin(ang)
    k = np.zeros((len(ang), 3, 3))
    k[:, 0, 1], k[:, 0, 2], k[:, 1, 0], k[:, 1, 2], k[:, 2, 0], k[:, 2, 1] = z, -y, -z, x, y, -x
    outer = axis[:, :, None] * axis[:, None, :]
    return c[:, None, None] * np.eye(3) + s[:, None, None] * k + (1 - c)[:, None, None] * outer


def fk_palettes(parent, rest, ni, step=0, amplitude=0.4, seed=7):
    """Skinning palettes [NI,NB,16] of a swaying pose, by forward kinematics in float64 rounded to binary32: every bone turns about
    its own rest position by an angle that depends on instance, bone and step, the root also moves.  (parent[b] < b.)"""
    rest = np.asarray(rest, np.float64)
    nb = len(parent)
    rng = np.random.RandomState(seed)
    axis = rng.normal(size=(nb, 3))
    axis /= np.linalg.norm(axis, axis=1, keepdims=True)
    world = np.zeros((ni, nb, 4, 4))
    out = np.zeros((ni, nb, 16), F)
    inst = np.arange(ni)
    for b in range(nb):
        ang = amplitude * np.sin(0.21 * step + 0.37 * inst + 0.11 * b)
        local = np.zeros((ni, 4, 4))
        local[:, :3, :3] = _rot(np.tile(axis[b], (ni, 1)), ang)
        local[:, 3, 3] = 1.0
        p = parent[b]
        local[:, 3, :3] = rest[b] - (rest[p] if p >= 0 else 0.0)
        if p < 0:
            local[:, 3, :3] += 0.3 * np.sin(0.2 * step + inst[:, None] + np.arange(3)[None, :])
            world[:, b] = local
        else:
            world[:, b] = local @ world[:, p]
        skin = world[:, b].copy()
        skin[:, 3, :3] -= rest[b] @ world[:, b, :3, :3]
        out[:, b] = skin.reshape(ni, 16)
    return out


def circling_targets(ni, step, radius=6.0, weight=1.0):
    """[NI,4]: a target per instance on a circle around the rig's head height, plus a slow bob; the weight in column 3."""
    ang = 0.013 * step + 0.5 * np.arange(ni)
    t = np.stack([radius * np.cos(ang), 4.0 + 2.0 * np.sin(0.007 * step + np.arange(ni)), radius * np.sin(ang), np.full(ni, weight)], axis=1)
    return t.astype(F)


# ------------------------------------------------------------------------------------------------ the case table ---------------
def case_table(ni=32):
    """dict(parent, rest, aims, table, pal [NI,NB,16], targets [NI,4]) on the 41-bone rig, four aims (4 links with the eye below the
    last one, 2 links that are no direct parents, and two of 1 link); every branch CASES names is taken by some instance:
      0..7    swaying rows, circling targets of weight 1, 0.5, 2 (above 1), 0, -1, NaN, and a target with an infinite and a NaN coordinate
      8..15   identity rows (u = f exactly): the target straight ahead (u == v), straight behind with share 1 and no limit
              (antiparallel), straight behind with a limit (lp degenerate), straight behind at half weight (the blend degenerate),
              exactly on the eye, and a zero-scale eye row (la degenerate)
      16..    swaying rows of other steps, scaled rows, small weights (t < 1), tight limits (hit) and none (not hit)"""
    parent, rest = aim_rig()
    aims = [make_aim([4, 5, 6, 7], eye_bone=8, shares=[0.25, 0.25, 0.5, 1.0], cos_limits=[0.95, 0.9, 0.8, 0.5]),
            make_aim([18, 20], shares=[1.0, 0.5], cos_limits=[-1.0, 0.2], forward=(0.0, -1.0, 0.0)),
            make_aim([40], cos_limits=[0.3]),
            make_aim([2], eye_bone=39, shares=[1.0], cos_limits=[-1.0], eye_point=rest[39])]
    table = build_table(parent, rest, aims)
    nb = len(parent)
    pal = fk_palettes(parent, rest, ni, step=3)
    targets = circling_targets(ni, 5)
    targets[:, 3] = 1.0
    targets[1, 3], targets[2, 3], targets[3, 3], targets[4, 3], targets[5, 3] = 0.5, 2.0, 0.0, -1.0, np.nan
    targets[6, 0], targets[7, 1] = np.inf, np.nan
    ident = np.tile(np.eye(4, dtype=F).reshape(16), (nb, 1))
    pal[8:16] = ident
    # identity rows: the eye of every aim stands at its rest point e, the forward direction is f itself
    e40, e20, e2 = rest[40], rest[20], rest[39]
    targets[8] = [*(e40 + np.array([0.0, 0.0, -5.0], F)), 1.0]          # aim 2 (f = -z): u == v; the others turn
    targets[9] = [*(e40 + np.array([0.0, 0.0, 5.0], F)), 1.0]           # aim 2: straight behind, limit 0.3 -> lp degenerate
    targets[10] = [*(e2 + np.array([0.0, 0.0, 5.0], F)), 1.0]           # aim 3 (no limit, share 1): antiparallel
    targets[11] = [*(e2 + np.array([0.0, 0.0, 5.0], F)), 0.5]           # aim 3: t = 0.5, n = 0 -> the blend degenerate
    targets[12] = [*e20, 1.0]                                           # aim 1: the target exactly on the eye
    pal[13, 39, :12] = 0.0                                              # aim 3: a zero-scale eye row, la = 0
    pal[14, 18, :12] = 0.0                                              # aim 1: a zero-scale FIRST link row: H is its translation, still applied
    # aim 1 (f = -y), almost straight behind: link 0 (share 1, no limit) has 1 + cs <= 1e-6 and is skipped; link 1 (share 0.5) blends
    # to a direction across, hits its limit and is the first link applied
    targets[15] = [*(e20 + np.array([1e-3, 5.0, 0.0], F)), 1.0]
    rng = np.random.RandomState(77)
    pal[16:24] = fk_palettes(parent, rest, 8, step=40, amplitude=0.9)
    pal[24:28] = rigid_rows(rng, 4 * nb, scale=rng.uniform(0.5, 2.0, 4 * nb)).reshape(4, nb, 16)
    targets[16:24, 3] = np.linspace(0.05, 0.95, 8).astype(F)
    pal[28, 5, 1] = np.nan                                              # a NaN in a link row: this instance's rows, nobody else's
    return dict(parent=parent, rest=rest, aims=aims, table=table, pal=pal, targets=targets)


# ------------------------------------------------------------------------------------------------ the CPU driver ---------------
def build_driver(sanitize=False):
    return hp.build("aim_math_driver", [os.path.join(hp.TESTS, "aim_math_driver.cpp"), os.path.join(hp.CSRC, "error.cpp")],
                    sanitize=sanitize)


def desc_arrays(aims, rest):
    """The arrays of an mmdx_aim_set_desc for `aims`: (link_offset, link_bone, link_params [NL,2], eye_bone, eye_point, forward)."""
    rest = np.asarray(rest, F).reshape(-1, 3)
    off = np.zeros(len(aims) + 1, U)
    off[1:] = np.cumsum([len(a["links"]) for a in aims])
    bones = np.concatenate([np.asarray(a["links"], U) for a in aims]).astype(U)
    prm = np.concatenate([np.stack([a["shares"], a["cos_limits"]], axis=1) for a in aims]).astype(F)
    eye = np.array([a["eye_bone"] for a in aims], U)
    point = np.stack([rest[a["eye_bone"]] if a["eye_point"] is None else np.asarray(a["eye_point"], F) for a in aims]).astype(F)
    fwd = np.stack([a["forward"] for a in aims]).astype(F)
    return off, bones, np.ascontiguousarray(prm), eye, np.ascontiguousarray(point), np.ascontiguousarray(fwd)


def run_driver(exe, parent, rest, aims, calls):
    """calls = [(pal [NI,NB,16], targets [NI,4])] -> (table as the driver built it: per aim dict(bone, h, sin_limit, rows), [pal after
    each call])."""
    parent, rest = np.asarray(parent, np.int32), np.asarray(rest, F)
    off, bones, prm, eye, point, fwd = desc_arrays(aims, rest)
    nb, na, nl, ni = parent.size, len(aims), bones.size, calls[0][0].shape[0]

    def write(f):
        f.write(struct.pack("<5I", nb, na, nl, ni, len(calls)))
        for a in (parent, rest, off, bones, prm, eye, point, fwd):
            f.write(np.ascontiguousarray(a).tobytes())
        for pal, tgt in calls:
            f.write(np.ascontiguousarray(pal, F).tobytes())
            f.write(np.ascontiguousarray(np.broadcast_to(np.asarray(tgt, F).reshape(-1, 4), (ni, 4))).tobytes())

    def read(f):
        take = lambda dt, *shape: np.frombuffer(f.read(int(np.prod(shape)) * 4), dt).reshape(shape).copy()      # noqa: E731
        tb = []
        for a in aims:
            n_links = len(a["links"])
            n_rows = int(take(U, 1)[0])
            tb.append(dict(bone=take(U, n_links), h=take(F, n_links, 3), sin_limit=take(F, n_links),
                           rows=[tuple(r) for r in take(U, n_rows, 2).tolist()]))
        return tb, [take(F, ni, nb, 16) for _ in calls]
    return hp.run_files(exe, write, read)


def plan(cells, max_links, env, exe):
    """The planner of csrc/aim_table.hpp through the driver: [(cells, max_links, env)] -> [(block, threads, nblocks, lds)]."""
    rows = list(zip(cells, max_links, env))
    out = hp.run(exe, ["plan"], stdin="".join("%d %d %d\n" % r for r in rows)).stdout
    return [tuple(int(v) for v in line.split()) for line in out.splitlines()]


def assert_same(got, want, what):
    """Bit for bit, except that a NaN only has to be a NaN."""
    got, want = np.asarray(got, F), np.asarray(want, F)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    gn, wn = np.isnan(got), np.isnan(want)
    bad = (gn != wn) | (~gn & (got.view(U) != want.view(U)))
    if bad.any():
        at = tuple(int(v[0]) for v in np.nonzero(bad))
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} words differ, first at {at}: got {got[at]!r} "
                             f"({got.view(U)[at]:08x}), want {want[at]!r} ({want.view(U)[at]:08x})")

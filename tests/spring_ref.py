"""mmdx_spring_step restated in numpy from the text of include/mmdx.h (steps 1-7), binary32 throughout, one operation per line of
the header; the table builder of mmdx_spring_set_create; the rigs and the generated case table the CPU driver
(tests/spring_math_driver.cpp) and the gfx950 kernel are held to, bit for bit.  Nothing here needs a GPU or the library."""
import os
import struct

import numpy as np

from tests import host_program as hp

HERE = os.path.dirname(os.path.abspath(__file__))
F = np.float32
U = np.uint32
ONE, EPS = F(1.0), F(1e-6)
MAX_JOINTS, MAX_COLLIDERS = 32, 16
# every branch of the header's steps: what a case table must contain
CASES = ("degenerate", "heal", "reset", "dt_positive", "dt_zero", "dt_negative", "dt_nan", "rigid", "antiparallel", "rotated",
         "collider_hit", "collider_miss", "collider_centre", "tail_on_h", "nan_anchor", "healed_after_nan_anchor", "chain_of_1",
         "chain_of_32")


# ------------------------------------------------------------------------------------------------ the table -------------------
def build_table(parent, rest, chains, params, gravity=(0.0, -9.8, 0.0), colliders=None, tails=None):
    """What mmdx_spring_set_create builds (csrc/spring_table.hpp), for valid input: dict(bone u32 [NJ], h, t f32 [NJ,3], chains =
    [(first, count, anchor)], params f32 [NC,4], col_bone, col_sphere, gravity)."""
    parent = np.asarray(parent, np.int64)
    rest = np.asarray(rest, F).reshape(-1, 3)
    bone = np.concatenate([np.asarray(c, np.int64) for c in chains])
    h = rest[bone].copy()
    t = np.empty_like(h)
    rows, j = [], 0
    for c in chains:
        rows.append((j, len(c), int(parent[c[0]])))
        for k, b in enumerate(c):
            t[j] = rest[c[k + 1]] if k + 1 < len(c) else h[j] + (h[j] - rest[parent[b]])
            j += 1
    if tails is not None:
        t = np.asarray(tails, F).reshape(-1, 3).copy()
    cb, cs = (np.zeros(0, U), np.zeros((0, 4), F)) if colliders is None else (np.asarray(colliders[0], U), np.asarray(colliders[1], F).reshape(-1, 4))
    prm = np.ascontiguousarray(np.broadcast_to(np.asarray(params, F).reshape(-1, 4), (len(chains), 4)))
    return dict(bone=bone.astype(U), h=h, t=t, chains=rows, params=prm, col_bone=cb, col_sphere=cs, gravity=np.asarray(gravity, F))


# ------------------------------------------------------------------------------------------------ the arithmetic --------------
def pt(x, s):
    """pt(x, S)[c] = ((x0*S[c] + x1*S[4+c]) + x2*S[8+c]) + 1.0f*S[12+c]: x f32 [3], s f32 [N,16] -> [N,3]."""
    return ((x[0] * s[:, 0:3] + x[1] * s[:, 4:7]) + x[2] * s[:, 8:11]) + ONE * s[:, 12:15]


def length(d):
    s = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    return np.sqrt(s.astype(np.float64)).astype(F)


def finite(x):
    return (x - x) == 0


def _constrain(n, hh, t0, la, count=None):
    """Step 4.  -> the constrained n; count (a dict) gets the lanes whose tail sat on H."""
    stays = (n == t0).all(axis=1)
    d = n - hh
    l = length(d)
    back = ~(l > 0) | ~finite(l)
    out = hh + (d / l[:, None]) * la[:, None]
    out = np.where(back[:, None], t0, out)
    if count is not None:
        count["tail_on_h"] = count.get("tail_on_h", 0) + int((~stays & (l == 0)).sum())
    return np.where(stays[:, None], n, out)


def joint(row, h, t, c, p, prm, g, dt, reset, centres, count):
    """Steps 1-7 for one joint of N instances at once.  row f32 [N,16] (P); c, p f32 [N,3]; centres = [(C [N,3], r)].
    -> (row, c, p) after the step."""
    stiffness, drag, gscale, radius = (F(v) for v in prm)
    hh, t0 = pt(h, row), pt(t, row)
    a = t0 - hh
    la = length(a)
    deg = ~(la > 0) | ~finite(la)                                                               # step 1
    heal = ~(finite(c).all(axis=1) & finite(p).all(axis=1))                                     # step 2
    count["heal"] = count.get("heal", 0) + int((heal & ~deg).sum())
    count["nan_anchor"] = count.get("nan_anchor", 0) + int((~finite(row[:, :15]).all(axis=1)).sum())
    if not reset:                                                                               # (c = p = T0 = NaN is what a NaN anchor leaves)
        count["healed_after_nan_anchor"] = count.get("healed_after_nan_anchor", 0) + int((heal & ~deg & np.isnan(c).all(axis=1)).sum())
    if reset:
        heal = np.ones_like(heal)
        count["reset"] = count.get("reset", 0) + int((~deg).sum())
    c = np.where(heal[:, None], t0, c)
    p = np.where(heal[:, None], t0, p)
    if dt > 0:                                                                                  # step 3
        keep, sd, gd = ONE - drag, stiffness * dt, gscale * dt
        n = c + (c - p) * keep
        n = n + (t0 - c) * sd
        n = n + g[None, :] * gd
        count["dt_positive"] = count.get("dt_positive", 0) + 1
    else:
        n = c.copy()
        k = "dt_nan" if dt != dt else ("dt_zero" if dt == 0 else "dt_negative")
        count[k] = count.get(k, 0) + 1
    n = _constrain(n, hh, t0, la, count)                                                        # step 4
    for cc, r in centres:                                                                       # step 5
        rr = F(r) + radius
        d = n - cc
        l = length(d)
        hit = (l > 0) & (l < rr)
        pushed = _constrain(cc + (d / l[:, None]) * rr, hh, t0, la)
        n = np.where(hit[:, None], pushed, n)
        count["collider_hit"] = count.get("collider_hit", 0) + int((hit & ~deg).sum())
        count["collider_miss"] = count.get("collider_miss", 0) + int((~hit & (l > 0) & ~deg).sum())
        count["collider_centre"] = count.get("collider_centre", 0) + int(((l == 0) & ~deg).sum())
    p, c = c, n                                                                                 # step 6
    rigid = (n == t0).all(axis=1)                                                               # step 7
    u = a / la[:, None]
    v = (n - hh) / la[:, None]
    k0 = u[:, 1] * v[:, 2] - u[:, 2] * v[:, 1]
    k1 = u[:, 2] * v[:, 0] - u[:, 0] * v[:, 2]
    k2 = u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]
    cs = (u[:, 0] * v[:, 0] + u[:, 1] * v[:, 1]) + u[:, 2] * v[:, 2]
    m = ONE + cs
    anti = ~(m > EPS) & ~rigid & ~deg
    q00, q01, q02, q11, q12, q22 = (k0 * k0) / m, (k0 * k1) / m, (k0 * k2) / m, (k1 * k1) / m, (k1 * k2) / m, (k2 * k2) / m
    r = [[cs + q00, q01 + k2, q02 - k1], [q01 - k2, cs + q11, q12 + k0], [q02 + k1, q12 - k0, cs + q22]]
    o = np.zeros_like(row)
    for i in range(3):
        for j in range(3):
            o[:, 4 * i + j] = (row[:, 4 * i] * r[0][j] + row[:, 4 * i + 1] * r[1][j]) + row[:, 4 * i + 2] * r[2][j]
    for j in range(3):
        o[:, 12 + j] = hh[:, j] - ((h[0] * o[:, j] + h[1] * o[:, 4 + j]) + h[2] * o[:, 8 + j])
    o[:, 15] = ONE
    same = deg | rigid | anti
    back = deg | anti
    count["degenerate"] = count.get("degenerate", 0) + int(deg.sum())
    count["rigid"] = count.get("rigid", 0) + int((rigid & ~deg).sum())
    count["antiparallel"] = count.get("antiparallel", 0) + int(anti.sum())
    count["rotated"] = count.get("rotated", 0) + int((~same).sum())
    c = np.where(back[:, None], t0, c)
    p = np.where(back[:, None], t0, p)
    return np.where(same[:, None], row, o), c, p


def step(table, pal, state, dt, reset=False, ids=None, count=None):
    """One mmdx_spring_step: pal f32 [NI,NB,16], state f32 [NI,NJ,6] -> new (pal, state); the inputs are left alone.  ids: the
    instances stepped (None = all).  count: a dict that collects how often every case of CASES was taken."""
    count = {} if count is None else count
    pal, state = np.array(pal, F), np.array(state, F)
    rows = np.arange(pal.shape[0]) if ids is None else np.asarray(ids, np.int64)
    if rows.size == 0:
        return pal, state
    dt = F(dt)
    with np.errstate(all="ignore"):
        sub = pal[rows]
        centres = [(pt(table["col_sphere"][j, :3], sub[:, table["col_bone"][j]]), table["col_sphere"][j, 3]) for j in range(len(table["col_bone"]))]
        for ci, (first, n, anchor) in enumerate(table["chains"]):
            count["chain_of_%d" % n] = count.get("chain_of_%d" % n, 0) + 1
            row = sub[:, anchor].copy()
            for j in range(first, first + n):
                row, c, p = joint(row, table["h"][j], table["t"][j], state[rows, j, :3], state[rows, j, 3:], table["params"][ci],
                                  table["gravity"], dt, reset, centres, count)
                state[rows, j, :3], state[rows, j, 3:] = c, p
                sub[:, table["bone"][j]] = row
        pal[rows] = sub
    return pal, state


def nan_state(ni, nj):
    return np.full((ni, nj, 6), np.nan, F)


# ------------------------------------------------------------------------------------------------ rigs and palettes ------------
def chain_rig(lengths=(2, 1, 32), extra=2, seed=3):
    """A synthetic skeleton: bone 0 the root, bones 1..extra its children (anchors and collider bones), then one chain per entry of
    `lengths`, chain k hanging off bone k % (extra + 1).  -> (parent i32 [NB], rest f32 [NB,3], chains)."""
    rng = np.random.RandomState(seed)
    parent, rest, chains = [-1], [[0.0, 10.0, 0.0]], []
    for k in range(extra):
        parent.append(0)
        rest.append([0.5 * (k + 1), 11.0, 0.25 * k])
    for k, n in enumerate(lengths):
        at, pos, chain = k % (extra + 1), np.array(rest[k % (extra + 1)]), []
        for _ in range(n):
            pos = pos + np.array([0.05, -0.4, 0.1]) + rng.uniform(-0.15, 0.15, 3)
            parent.append(at)
            rest.append(pos.tolist())
            at = len(parent) - 1
            chain.append(at)
        chains.append(chain)
    return np.array(parent, np.int32), np.array(rest, F), chains


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


def sway_palettes(ni, nb, n_steps, seed=5, amplitude=0.35):
    """[n_steps, NI, NB, 16]: every bone of every instance follows its instance's swaying rigid motion (what a solve of a clip with
    unkeyed chain bones gives), plus a small per-bone wobble so that no two rows agree."""
    rng = np.random.RandomState(seed)
    phase, rate = rng.uniform(0, 6.28, (ni, 3)), rng.uniform(0.05, 0.4, (ni, 3))
    out = np.zeros((n_steps, ni, nb, 16), F)
    for s in range(n_steps):
        ang = amplitude * np.sin(phase + rate * s)
        cx, sx, cy, sy, cz, sz = np.cos(ang[:, 0]), np.sin(ang[:, 0]), np.cos(ang[:, 1]), np.sin(ang[:, 1]), np.cos(ang[:, 2]), np.sin(ang[:, 2])
        m = np.zeros((ni, 4, 4))
        m[:, 0, 0], m[:, 0, 1], m[:, 0, 2] = cy * cz, cy * sz, -sy
        m[:, 1, 0], m[:, 1, 1], m[:, 1, 2] = sx * sy * cz - cx * sz, sx * sy * sz + cx * cz, sx * cy
        m[:, 2, 0], m[:, 2, 1], m[:, 2, 2] = cx * sy * cz + sx * sz, cx * sy * sz - sx * cz, cx * cy
        m[:, 3, :3] = 0.5 * np.sin(phase * 0.7 + rate * s * 1.3)
        m[:, 3, 3] = 1.0
        out[s] = m.reshape(ni, 1, 16)
    return out


# ------------------------------------------------------------------------------------------------ the case table ---------------
CASE_LENGTHS = (2, 1, 32, 1)
CASE_DTS = (1 / 60, 1 / 60, 0.0, -0.25, float("nan"), 1 / 30, 1 / 60, 1 / 60)
CASE_RESET = (True, False, False, False, False, False, False, True)


def case_table(ni=24, seed=11):
    """dict(parent, rest, chains, params, colliders, gravity, tails, state0, dts, resets, pals [n_steps, NI, NB, 16]): four chains
    (2, 1, 32 joints and a 1-joint chain whose tail is its own rest position), three colliders (one whose centre IS the tail of
    chain 0's first joint, one large sphere around the long chain, one far away), steps with every kind of dt, an initial state with
    NaN and infinite rows, a tail on H and a tail opposite its rest direction, and a NaN anchor for one frame."""
    parent, rest, chains = chain_rig(CASE_LENGTHS)
    nb = len(parent)
    t = build_table(parent, rest, chains, np.zeros(4, F))
    tails = t["t"].copy()
    tails[t["chains"][3][0]] = t["h"][t["chains"][3][0]]                    # degenerate: la == 0
    params = np.array([[30.0, 0.2, 1.0, 0.05], [0.0, 0.1, 1.0, 0.0], [8.0, 0.4, 0.5, 0.1], [5.0, 0.5, 1.0, 0.0]], F)
    mid = t["h"][t["chains"][2][0] + 12]
    colliders = (np.array([0, 0, 1], U),
                 np.array([[*tails[0], 0.01], [*mid, 0.9], [50.0, 50.0, 50.0, 0.5]], F))
    rng = np.random.RandomState(seed)
    n_steps = len(CASE_DTS)
    pals = sway_palettes(ni, nb, n_steps, seed)
    pals[:, :, 1] = pals[:, :, 0]                                           # the collider bone moves with the root
    pals[:, ni // 2:, :, :] = rigid_rows(rng, n_steps * (ni - ni // 2) * nb, scale=rng.uniform(0.5, 2.0, n_steps * (ni - ni // 2) * nb)
                                         ).reshape(n_steps, ni - ni // 2, nb, 16)      # the other half: unrelated rows, scaled
    pals[5, 3, 0, :] = np.nan                                               # a NaN anchor for one frame (the step after is finite)
    pals[5, 4, 0, 13] = np.inf
    state0 = nan_state(ni, len(tails))
    table = build_table(parent, rest, chains, params, (0.0, -9.8, 0.0), colliders, tails)
    return dict(parent=parent, rest=rest, chains=chains, params=params, colliders=colliders, gravity=np.array([0.0, -9.8, 0.0], F),
                tails=tails, state0=state0, dts=CASE_DTS, resets=CASE_RESET, pals=pals, table=table)


def plant(case, state, pal_next):
    """Tails planted into `state` (what the first step left) for the step that reads pal_next with dt = 0: instance 0's first joint of
    chain 0 opposite its rest direction (antiparallel), instance 1's on H, instances 2 and 5 non-finite."""
    t = case["table"]
    first, _, anchor = t["chains"][0]
    row = pal_next[:, anchor]
    with np.errstate(all="ignore"):
        hh, t0 = pt(t["h"][first], row), pt(t["t"][first], row)
    state = state.copy()
    state[0, first, :3] = state[0, first, 3:] = (hh - (t0 - hh))[0]
    state[1, first, :3] = state[1, first, 3:] = hh[1]
    state[2, first, 0] = np.inf
    state[5, first + 1, 4] = np.nan
    return state


def run_case(case):
    """The restatement over the case table -> ([(pal, state) after every step], counts).  The planted tails go in before step 2
    (dt = 0), as run_driver's `plant_at` does for the driver."""
    count, out = {}, []
    state = case["state0"]
    for s, (dt, reset) in enumerate(zip(case["dts"], case["resets"])):
        if s == PLANT_AT:
            state = plant(case, state, case["pals"][s])
        pal, state = step(case["table"], case["pals"][s], state, dt, reset, count=count)
        out.append((pal, state))
    return out, count


PLANT_AT = 2


# ------------------------------------------------------------------------------------------------ the CPU driver ---------------
def build_driver(sanitize=False):
    return hp.build("spring_math_driver", [os.path.join(hp.TESTS, "spring_math_driver.cpp"), os.path.join(hp.CSRC, "error.cpp")],
                    sanitize=sanitize)


def run_driver(exe, parent, rest, chains, params, colliders, gravity, tails, segments):
    """segments = [(state0 or None, [(dt, reset, pal [NI,NB,16]), ...])]: each segment starts from its state (None = NaN, or the
    previous segment's last state when it is not the first) -> (table dict as the driver built it, [(pal, state) per step])."""
    parent, rest = np.asarray(parent, np.int32), np.asarray(rest, F)
    off = np.zeros(len(chains) + 1, U)
    off[1:] = np.cumsum([len(c) for c in chains])
    bones = np.concatenate([np.asarray(c, U) for c in chains]).astype(U)
    nb, nj, ni = parent.size, bones.size, segments[0][1][0][2].shape[0]
    cb, cs = (np.zeros(0, U), np.zeros((0, 4), F)) if colliders is None else (np.asarray(colliders[0], U), np.asarray(colliders[1], F))
    n_steps = sum(len(s[1]) for s in segments)

    def write(f):
        f.write(struct.pack("<8I", nb, len(chains), nj, cb.size, int(tails is not None), ni, n_steps, len(segments)))
        for a in (parent, rest, off, bones) + ((np.asarray(tails, F),) if tails is not None else ()) + \
                (np.asarray(params, F).reshape(len(chains), 4), cb, cs, np.asarray(gravity, F)):
            f.write(np.ascontiguousarray(a).tobytes())
        for state0, steps in segments:
            f.write(struct.pack("<2I", len(steps), int(state0 is not None)))
            if state0 is not None:
                f.write(np.ascontiguousarray(state0, F).tobytes())
            for dt, reset, pal in steps:
                f.write(struct.pack("<fI", dt, int(reset)))
                f.write(np.ascontiguousarray(pal, F).tobytes())

    def read(f):
        take = lambda dt, *shape: np.frombuffer(f.read(int(np.prod(shape)) * 4), dt).reshape(shape).copy()      # noqa: E731
        tb = dict(bone=take(U, nj), h=take(F, nj, 3), t=take(F, nj, 3), chains=[tuple(r) for r in take(U, len(chains), 3).tolist()])
        return tb, [(take(F, ni, nb, 16), take(F, ni, nj, 6)) for _ in range(n_steps)]
    return hp.run_files(exe, write, read)


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

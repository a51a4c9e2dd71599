"""Steered physics-seam cases: a crowd whose strict bones invert every kind of 4x4 matrix, read off the oracle's inverse trace.

physics_override_kernel's Fix (csrc/rig_kernels.hip) multiplies a strict bone with a parent by inverse(parent_local): a hand-unrolled
Gauss-Jordan with scaled partial pivoting that exchanges rows by value -- 24 pivot orders, two exits to the zero matrix, a tie
rule, divisions by a zero pivot.  Oracle.trace_inverse records every call of the oracle's inverse (input bits, the pivot row chosen
at columns 0..2, the exit, ties, zero pivots, non-finite input / output); this module builds ONE small rig and a crowd of NI
instances and CHECKS the classes on the trace, not on what the builder meant to build.

The lever.  A ROOT bone P that is strict and listed before its strict child C is left by Fix with the local matrix
G^-1 * X_P, row 3 xyz replaced by total_translation + rest: rows 0..2 are the override's, row 3 xyz is P's pose, [3][3] is
rest . X_P[0:3, 3] + X_P[3][3].  So every element of the matrix C's Fix inverts is the test's, per instance.  With rest at the
origin (P0 / C0) the target matrix arrives bit for bit; under P (rest off the origin) the translation is target - rest, rounded.

The rig (8 bones, one per row of BONES; * = post-physics):

    P -> C -> E -> F*          P0 -> C0
         C -> D* -> Q

Q is a PRE-physics bone whose parent D is post-physics: its Fix reads a local matrix the pre step did not write (the identity
PrePhysicsPosing's reset left, in libmmd, the oracle and on the device alike).

Override lists (LISTS; bones, strict flags; the skinning rows of one list are xf[name] [NI, K, 16]):

    L1   [P, C]      strict, strict     the steered inverse under a rest off the origin
    L1z  [P0, C0]    strict, strict     the same matrices, bit for bit (zero row 3 included)
    L2   [P, C, E]   all strict         E inverts a local matrix that was itself produced with an inverse
    L3   [C, P]      strict, strict     the child first: it reads P's PRE-physics local; P's pose quaternion is a unit one, twice a
                                        unit one, zero or half a unit one by instance % 4 -- a scaled or identity-like local with no
                                        override at all
    L4   [P, C]      Synchronize, strict  the local matrix is untouched while P's palette row changes
    L5   [P, C, C]   all strict         the second Fix of C reads the first one's skinning row
    L6   [P, C, Q]   all strict         Q under the post-physics D

The crowd (_cases(); the same target matrix M_i steers P and P0 of instance i): two permuted diagonally dominant matrices per pivot
order, random normal(16) matrices, zero rows 0..3 (+0.0 and -0.0), singular matrices that reach the zero last pivot through a zero
fourth column or a duplicated row under different row orders, ties at columns 0, 1 and 2, zero pivots at columns 0, 1 and 2 with
no zero row, NaN and +-inf entries, rigid * 2^-130 (denormals), rows scaled 2^-130 / 1 / 2^100 (and 2^-40 / 1 / 2^40, whose
inverses stay finite), entries near 1e30, and plain rigid matrices.  crowd() interleaves them (STRIDE: a fixed step through the list) so
that consecutive instances -- lanes of one wave -- take different pivot orders and exits; the tests assert that on the trace.

tests/golden/seam_fix_classes.json lists the classes that must occur and pins the histogram; tests/golden/seam_fix_expect.npz holds
libmmd's palettes for every list (tests/gen_seam_fix_golden.py writes both)."""
import itertools
import json
import os

import numpy as np

from oracle.pyoracle import Oracle

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CLASSES = os.path.join(GOLDEN_DIR, "seam_fix_classes.json")
EXPECT = os.path.join(GOLDEN_DIR, "seam_fix_expect.npz")
F_POST = 0x1000
P, C, E, D, F, P0, C0, Q = range(8)
BONES = (  # name, parent, rest, flags
    ("P", -1, (1.5, 2.0, -0.5), 0), ("C", P, (1.5, 3.25, -0.25), 0), ("E", C, (2.0, 4.0, 0.0), 0),
    ("D", C, (1.0, 3.5, 0.5), F_POST), ("F", E, (2.5, 4.5, 0.25), F_POST),
    ("P0", -1, (0.0, 0.0, 0.0), 0), ("C0", P0, (0.0, 1.0, 0.5), 0), ("Q", D, (1.0, 4.0, 1.0), 0))
NB = len(BONES)
LISTS = {  # name: (bones, strict)
    "L1": ((P, C), (1, 1)), "L1z": ((P0, C0), (1, 1)), "L2": ((P, C, E), (1, 1, 1)), "L3": ((C, P), (1, 1)),
    "L4": ((P, C), (0, 1)), "L5": ((P, C, C), (1, 1, 1)), "L6": ((P, C, Q), (1, 1, 1))}
# the bone whose Fix runs each traced inverse of a list, in call order (root bones and Synchronize-only ones call none)
INVERTING = {"L1": (C,), "L1z": (C0,), "L2": (C, E), "L3": (C,), "L4": (C,), "L5": (C, C), "L6": (C, Q)}
ORDERS = tuple(itertools.permutations(range(4)))            # the row that is pivot at column 0, 1, 2 (and the one left over)
T = dict(zip(Oracle.INVERSE_TRACE_FIELDS, range(len(Oracle.INVERSE_TRACE_FIELDS))))
STRIDE = 73                                                 # coprime with NI: crowd() walks the case list with this step
CUTS = (1, 63, 64, 65, 130)                                 # one lane per instance, 64 lanes per workgroup


def rig():
    """(rest, parent, level, flags, append_parent, append_ratio, ik) as vmd.Skeleton and the oracle take them."""
    rest = np.asarray([b[2] for b in BONES], np.float32)
    parent = np.asarray([b[1] for b in BONES], np.int64)
    flags = np.asarray([b[3] for b in BONES], np.uint16)
    return rest, parent, np.zeros(NB, np.int32), flags, None, None, None


def _rot(rng):
    q = rng.normal(size=4)
    x, y, z, w = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y + z * w), 2 * (x * z - y * w)],
                     [2 * (x * y - z * w), 1 - 2 * (x * x + z * z), 2 * (y * z + x * w)],
                     [2 * (x * z + y * w), 2 * (y * z - x * w), 1 - 2 * (x * x + y * y)]])


def _rigid(rng, shear=0.0):
    m = np.eye(4)
    m[:3, :3] = _rot(rng) + rng.normal(size=(3, 3)) * shear
    m[3, :3] = rng.uniform(-3, 3, 3)
    return m


def _placed(rows, order):
    """The matrix whose row order[k] is rows[k]: with dominant diagonals in `rows`, the pivot order is `order`."""
    m = np.zeros((4, 4))
    for k in range(4):
        m[order[k]] = rows[k]
    return m


def _cases():
    """[(kind, M f32 [4, 4])]: what the builder MEANT; classify() says what the oracle did."""
    rng = np.random.RandomState(20240607)
    out = []
    add = lambda kind, m: out.append((kind, np.asarray(m, np.float64).astype(np.float32)))        # noqa: E731
    for rep in range(2):                                    # a dominant diagonal, rows placed for every pivot order
        for order in ORDERS:
            a = np.diag(rng.uniform(2, 5, 4) * rng.choice([-1, 1], 4)) + rng.normal(size=(4, 4)) * 0.4
            if rep:
                a *= rng.uniform(0.1, 10, (4, 1))           # rows of different scale: the scaled pivoting sees through it
            add("placed", _placed(a, order))
    for _ in range(20):
        add("normal", rng.normal(size=(4, 4)))
    for r in range(4):                                      # zero rows: +0.0, then -0.0 (scale == 0 must catch both)
        for zero in (0.0, -0.0):
            m = rng.normal(size=(4, 4))
            if np.signbit(zero):
                m = -np.abs(m)                              # G^-1 * X adds 0 * x of the other rows: only -0.0 keeps the sign
            m[r] = zero
            add("zero_row", m)
    for order in ORDERS[1::4]:                              # a zero fourth column: the last pivot is exactly zero
        a = np.diag(rng.uniform(2, 5, 4)) + rng.normal(size=(4, 4)) * 0.4
        a[:, 3] = 0
        add("zero_column3", _placed(a, order))
    for order in ORDERS[2::6]:                              # the last two pivot rows are one row twice
        a = np.diag(rng.uniform(2, 5, 4)) + rng.normal(size=(4, 4)) * 0.4
        a[3] = a[2]
        add("duplicate_row", _placed(a, order))
    # ties: candidates whose largest element stands in the pivot column (|s / scale| == 1 for each); the rows above have zeros
    # below their pivots so that the elimination subtracts 0 * x and leaves the tied rows as they are
    tie_rows = {0: [[4, 1, -2, 1], [-2, 1, 0.5, 1], [1, 0.5, 0.25, -1], [0.5, 0.25, 3, 1]],
                1: [[4, 1, -2, 1], [0, 2, 1, 0.5], [0, -2, 0.5, 1.5], [0, 0.5, 1, 3]],
                2: [[4, 1, -2, 1], [0, 2, 1, 0.5], [0, 0, -3, 1], [0, 0, 3, 2]]}
    for col, rows in tie_rows.items():
        for order in ((0, 1, 2, 3), (3, 2, 1, 0), (1, 3, 0, 2)):
            add("tie", _placed(np.asarray(rows, np.float64), order))
    # a zero pivot at column c: the whole column is zero below the rows chosen before it, no row is zero
    zero_pivot_rows = {0: [[0, 1, 2, 1], [0, 2, -1, 3], [0, 1, 1, -2], [0, -3, 1, 1]],
                       1: [[4, 1, -2, 1], [0, 0, 1, 0.5], [0, 0, 0.5, 1.5], [0, 0, 1, 3]],
                       2: [[4, 1, -2, 1], [0, 2, 1, 0.5], [0, 0, 0, 1], [0, 0, 0, 2]]}
    for col, rows in zero_pivot_rows.items():
        for order in ((1, 0, 2, 3), (2, 0, 3, 1)):
            add("zero_pivot", _placed(np.asarray(rows, np.float64), order))
    for at in ((1, 2), (3, 3)):
        m = _rigid(rng, 0.02)
        m[at] = np.nan
        add("nan", m)
    for at, v in (((0, 0), np.inf), ((2, 1), -np.inf)):
        m = _rigid(rng, 0.02)
        m[at] = v
        add("inf", m)
    for order in ((0, 1, 2, 3), (2, 3, 1, 0)):              # denormals: a flush to zero turns these into zero rows
        a = np.diag(rng.uniform(2, 5, 4)) + rng.normal(size=(4, 4)) * 0.4
        add("denormal", _placed(a, order) * 2.0 ** -130)
    add("denormal", _rigid(rng) * 2.0 ** -130)
    for exps in ((-130, 0, 100, 0), (100, -130, 0, 0), (0, 100, 0, -130), (-40, 0, 40, 0), (40, 0, -40, 0), (0, 40, -40, 0)):
        add("mixed_scale", rng.normal(size=(4, 4)) * (2.0 ** np.asarray(exps, np.float64))[:, None])
    add("huge", _rigid(rng, 0.02) * 1e30)
    for _ in range(2):                                      # 1e30 next to 1: a multiplier times a row element passes FLT_MAX
        add("huge", rng.normal(size=(4, 4)) * np.where(rng.uniform(size=(4, 4)) < 0.5, 1e30, 1.0))
    while len(out) < NI:
        add("rigid", _rigid(rng, 0.0 if len(out) % 2 else 0.02))
    return out


NI = 136
assert NI % STRIDE and NI > max(CUTS)


class Crowd:
    """kinds [NI] (what the builder meant), targets f32 [NI, 4, 4], poses f32 [NI, NB, 8], xf {list: f32 [NI, K, 16]}."""


_CROWD = None


def crowd():
    """The case crowd (deterministic; built once per process and never modified)."""
    global _CROWD
    if _CROWD is not None:
        return _CROWD
    cases = _cases()
    assert len(cases) == NI, len(cases)
    order = [(i * STRIDE) % NI for i in range(NI)]
    cw = Crowd()
    cw.kinds = [cases[k][0] for k in order]
    cw.targets = np.stack([cases[k][1] for k in order])
    rest = rig()[0]
    rng = np.random.RandomState(77)
    poses = np.zeros((NI, NB, 8), np.float32)
    poses[..., 0:3] = rng.uniform(-1, 1, (NI, NB, 3))
    q = rng.normal(size=(NI, NB, 4))
    poses[..., 4:8] = q / np.linalg.norm(q, axis=-1, keepdims=True)
    with np.errstate(invalid="ignore", over="ignore"):
        poses[:, P, 0:3] = cw.targets[:, 3, 0:3] - rest[P]                  # total_translation + rest == the target's row 3
        poses[:, P0, 0:3] = cw.targets[:, 3, 0:3]
        poses[:, P, 4:8] *= np.asarray([1.0, 2.0, 0.0, 0.5], np.float32)[np.arange(NI) % 4, None]      # L3 / L4 read this local
        x_p = cw.targets.copy()
        x_p[:, 3, 0:3] = rng.uniform(-3, 3, (NI, 3))                        # (Fix replaces these)
        x_p0 = x_p.copy()
        # [3][3] of G^-1 * X is rest . X[0:3, 3] + X[3][3]: aim it at the target's
        x_p[:, 3, 3] = cw.targets[:, 3, 3] - (cw.targets[:, 0:3, 3].astype(np.float64) * rest[P].astype(np.float64)).sum(1)

    def free(n):                                            # the other bones' overrides: rigid with shear, or anything
        m = np.stack([_rigid(rng, 0.02) if (i + n) % 2 else rng.normal(size=(4, 4)) for i in range(NI)])
        return m.astype(np.float32)
    x = {P: x_p, P0: x_p0, C: free(0), C0: free(1), E: free(0), Q: free(1)}
    second_c = free(1)
    cw.xf = {}
    for name, (bones, _) in LISTS.items():
        rows = [x[b] for b in bones]
        if name == "L5":
            rows[2] = second_c
        cw.xf[name] = np.ascontiguousarray(np.stack(rows, 1).reshape(NI, len(bones), 16))
    cw.poses = poses
    for a in (cw.targets, cw.poses, *cw.xf.values()):
        a.setflags(write=False)
    _CROWD = cw
    return cw


def over(name):
    bones, strict = LISTS[name]
    return np.asarray(bones, np.int64), np.asarray(strict, np.uint8)


def oracle_solve(oracle, name, i, cw=None):
    """(palette [NB, 16], inverse trace records [n, 24]) of instance i under list `name`."""
    cw = cw or crowd()
    rest, parent, level, flags, ap, ar, ik = rig()
    bones, strict = over(name)
    got = []
    rec = oracle.trace_inverse(lambda: got.append(
        oracle.bone_solve_physics(rest, parent, cw.poses[i], bones, strict, cw.xf[name][i], level, flags, ap, ar, ik)[0]))
    assert rec.shape[0] == len(INVERTING[name]), (name, i, rec.shape)
    return got[0], rec


_WANT = {}


def oracle_palettes(oracle, name):
    """(palettes f32 [NI, NB, 16], records u32 [NI, n, 24]) of the whole crowd under list `name`: computed once, shared, read-only."""
    if name not in _WANT:
        res = [oracle_solve(oracle, name, i) for i in range(NI)]
        pal, rec = np.stack([r[0] for r in res]), np.stack([r[1] for r in res])
        pal.setflags(write=False)
        rec.setflags(write=False)
        _WANT[name] = (pal, rec)
    return _WANT[name]


def pivot_order(rec):
    """The four original row indices in pivot order, or None where the call left before column 2 was decided."""
    p = [int(rec[T["pivot0"]]), int(rec[T["pivot1"]]), int(rec[T["pivot2"]])]
    if Oracle.INVERSE_NONE in p:
        return None
    return tuple(p) + tuple(r for r in range(4) if r not in p)


def classify(rec):
    """The classes one inverse-trace record belongs to (names as in seam_fix_classes.json)."""
    m = np.asarray(rec[:16], np.uint32).view(np.float32).reshape(4, 4)
    kind = Oracle.INVERSE_EXITS[int(rec[T["exit"]])]
    order = pivot_order(rec)
    tag = "".join(map(str, order)) if order else ""
    out = set()
    if kind == "inverted":
        out.add("inverted/" + tag)
    elif kind == "zero_row":
        r = int(rec[T["zero_row"]])
        out.add("zero_row/%d" % r)
        if np.signbit(m[r]).any():
            out.add("zero_row/negative_zero")
    else:
        out.add("zero_last_pivot/" + tag)
    for c in range(3):
        if rec[T["ties"]] >> c & 1:
            out.add("tie/column%d" % c)
        if rec[T["zero_pivots"]] >> c & 1:
            out.add("zero_pivot/column%d" % c)
    a = np.abs(m)
    if np.isnan(m).any():
        out.add("input/nan")
    if np.isinf(m).any():
        out.add("input/inf")
    finite = not (int(rec[T["nonfinite"]]) & 1)
    if ((a > 0) & (a < np.float32(2.0 ** -126))).any():
        out.add("input/denormal")
    if finite and kind != "zero_row":
        scale = a.max(1).astype(np.float64)
        if scale.max() >= 2.0 ** 60 * scale.min() and order[0] != int(np.argmax(a[:, 0])):
            out.add("mixed_scale/scaled_pivot_differs_from_plain")
        if a.max() >= 1e29 and int(rec[T["nonfinite"]]) & 2:
            out.add("input/huge_overflows")
        r3 = m[:3, :3].astype(np.float64)
        if np.array_equal(m[:, 3], np.asarray([0, 0, 0, 1], np.float32)) and np.abs(r3 @ r3.T - np.eye(3)).max() < 1e-5:
            out.add("input/rigid")
    return out


def required():
    with open(CLASSES) as f:
        return json.load(f)


def histogram(oracle):
    """{list: {class: inversions of the whole crowd in it}}: what seam_fix_classes.json pins."""
    out = {}
    for name in LISTS:
        h = {}
        for recs in oracle_palettes(oracle, name)[1]:
            for rec in recs:
                for c in classify(rec):
                    h[c] = h.get(c, 0) + 1
        out[name] = dict(sorted(h.items()))
    return out


def reference_palettes(name):
    """libmmd's own palettes f32 [NI, NB, 16] of the whole crowd under list `name` (needs the reference build)."""
    from oracle.pyoracle import Reference
    cw = crowd()
    rest, parent, level, flags, ap, ar, ik = rig()
    ref = Reference.skeleton(rest, parent, level, flags, ap, ar, ik)
    bones, strict = over(name)
    out = np.stack([ref.solve_physics(cw.poses[i], bones, strict, cw.xf[name][i])[0] for i in range(NI)])
    ref.close()
    return out

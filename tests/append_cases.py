"""Steered append (inherit) bones: crowds in which every append topology is present, read off the oracle's append trace.

An append bone's transform (transform_at in csrc/rig_kernels.hip) reads its append parent's total rotation / translation AS THEY
STAND at that moment and runs the rotation through q_slerp_from_identity.  The round schedule (schedule_rounds / solve_event_sets in
csrc/rig.cpp) treats that read as a dependency, the LDS-window eligibility test excludes chains with an append bone inside, the
stores in transform_at are ordered for the bone that names itself, and the physics seam's Fix reads the augmented translation.
Oracle.trace_append records every execution of the append branch (bone, parent, kind, ratio, context, nesting depth, the parent's
state, the SLerp branch, NaN); this module builds rigs whose append bones realise every class below and CHECKS the classes on the
trace and the rig tables, not on what the builder meant to build.

Rigs.  A rig is a row of independent islands of a few bones (3 apart along x), so many islands share a round and the slots of a
workgroup run different topologies.  Every append bone has a child.  R = a plain root, S = a plain posed bone whose rotation is
steered (below), A = an append bone, C = its child.  Islands (name: what it realises):

  t1_rot, t1_tr, t1_rottr      T1 parent transformed earlier in the same list, one per kind; the rot ones are `mixing`
  t2_rot, t2_tr, t2_rottr      T2 by index: A has the lower index, S the higher, same level
  t2_level                     T2 by level: S has the lower index and transform level 2, A level 0
  t3_pre_post                  T3 a pre-physics A reads a post-physics bone (the reset state: always omega <= 1e-7)
  t3_post_pre                  T3 a post-physics A reads a pre-physics S (mixing)
  t4_rot, t4_tr, t4_rottr      T4 A names itself (A is its own steered bone)
  t5_minus1, t5_past           T5 flag set, parent -1 / nb + 5: no trace record, palettes of the rig with the flag cleared
  t6_depth3                    T6 S <- A1 <- A2 <- A3 in evaluation order (rot+tr each)
  t6_against                   T6 A1 <- A2 <- S against it: A1 (rot) reads A2 (tr) before A2 has read S
  t6_cycle                     T6 A <-> B (rot+tr each): A reads the reset B, B reads the written A
  t6_tr_through_rot            T6 A (tr) <- P (rot only) <- S: P's translation is NOT augmented, so S's never reaches A
  t7_own_parent, t7_own_child  T7 the append parent is the bone's parent / its child (the child has the lower index: it is
                               evaluated first, under the reset matrix of its parent, and A reads it written)
  ratios                       one S, six rot+tr bones with ratio 0, 1, -1, 0.5, 2 and 1e-8 (mixing)
  i1_rootward, i1_tipward      I1 link 0 appends from link 2 of its own chain / link 2 from link 0 (3 links, off the window)
  i2_rot, i2_tr                I2 the TARGET appends: rotation from link 1 of its own chain / translation from an outside S; it
                               is re-evaluated after every link step (one loop_target record per step, asserted)
  i3_tr, i3_rot                I3 the IK bone itself appends (its translation moves ik_pos); these chains stay window chains
  i4                           I4 the append parent is link 1 of a window chain: one A before the IK bone, one after it
  i5                           I5 one A reads a window chain's target, one reads its IK bone
  i6                           I6 the parent of a window chain's root-most link is an append bone (mixing)
  i7                           I7 the nested pair of ik_exits with link q1 of the INNER chain appending from an outside S:
                               records at depth 2 (rig "nested" only)

Rigs: "topo" (every T island and the ratios, FK only, post-physics bones: the physics-seam and bone-morph rig), "ik" (I1, I2, I3
and two T1 islands; chains on the HBM state), "window" (I3 - I6, T1, T4 and the ratios; every chain is a window chain and the
plan runs them sixteen lanes per solve), "nested" (I7, I1, I2 and T islands; the NESTED kernel variant).

Instances.  The SLerp input is steered through the append parent's pose.  A seeded pool of POOL candidates per rig gives every
steered bone of island k one of the POSE_KINDS -- regular; flipped (w < 0); identity (omega <= 1e-7 on a WRITTEN parent); w = the
largest float below 1; w = 0; un-normalised with w > 1 (acos -> NaN -> identity); norm 0.5; norm 1.5; NaN (rotation and translation:
a NaN rotation alone takes the NaN-omega branch and leaves the append bone finite) -- and every other posed
bone a small random rotation and translation.  The pool is solved and traced on the whole rig; the islands are independent, so each
island then picks its own NI = 96 candidates, greedily: in every aligned group of 16 instances as many SLerp branches of its mixing
bone as it can get, then the pose kind used least.  Candidates whose island holds a NaN palette go to ik_exits.NAN_ROWS and nothing
else does.  ik_exits.select_ids() maps aligned groups of 16 onto aligned groups of 16, so the neighbour condition (>= 4 different
SLerp branches -- all four -- in every aligned 16, per mixing bone) holds in list order too.

Unreachable classes: none.  Every class of REQUIRED is realised in at least ik_exits.MIN_PER_CLASS evaluations (the per-bone classes
in 96 each, one per instance), so no search had to be widened.  Pool candidates replaced because of a device libm difference: none.

tests/golden/append_classes.json pins the histogram of the chosen cases."""
import json
import os

import numpy as np

from oracle.pyoracle import Oracle
from tests import ik_exits as ix

NI = ix.NI
POOL = 288
SEG = 0.5
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "append_classes.json")
ROT, TR, ROTTR = 1, 2, 3
F_IK, F_ROT, F_TR, F_POST = 0x0020, 0x0100, 0x0200, 0x1000
RATIOS = (0.0, 1.0, -1.0, 0.5, 2.0, 1e-8)
POSE_KINDS = ("regular", "flipped", "identity", "w_below_1", "w_zero", "w_above_1", "norm_0.5", "norm_1.5", "nan")
F = dict(zip(Oracle.APPEND_TRACE_FIELDS, range(len(Oracle.APPEND_TRACE_FIELDS))))
SEQ, FIRST, LOOP = 0, 1, 2                      # context
UNWRITTEN, WRITTEN, SELF = 0, 1, 2              # parent state
S_NONE, S_REGULAR, S_FLIP, S_SMALL, S_NAN = range(5)


class Builder:
    """Collects bones; an island is the bones added between island() calls."""

    def __init__(self):
        self.rest, self.parent, self.level, self.flags, self.ap, self.ar, self.ik = [], [], [], [], [], [], {}
        self.islands = []
        self.t5_past = []

    def island(self, name):
        self.x = 3.0 * len(self.islands)
        self.cur = dict(name=name, bones=[], steer=[], mixing=[], chains=[])
        self.islands.append(self.cur)
        return self.cur

    def bone(self, y, parent=-1, level=0, post=False, dx=0.0, steer=False):
        self.rest.append((self.x + dx, y, 0.0)); self.parent.append(parent); self.level.append(level)
        self.flags.append(F_POST if post else 0); self.ap.append(-1); self.ar.append(0.0)
        b = len(self.rest) - 1
        self.cur["bones"].append(b)
        if steer:
            self.cur["steer"].append(b)
        return b

    def append(self, b, parent, ratio, kind, mixing=False):
        self.flags[b] |= kind << 8
        self.ap[b], self.ar[b] = parent, ratio
        if mixing:
            self.cur["mixing"].append(b)

    def chain(self, n_links, loop, angle, root=None, dx=0.0):
        """ik_exits' line chain: root, n links SEG apart along +y, the target as child of link 0, the IK bone as child of the root
        resting on the target.  links[0] = the one next to the target."""
        root = self.bone(0.0, dx=dx) if root is None else root
        line = [root]
        for k in range(1, n_links + 1):
            line.append(self.bone(SEG * k, line[-1], dx=dx))
        links = line[:0:-1]
        y = SEG * (n_links + 1)
        target = self.bone(y, links[0], dx=dx)
        ikb = self.bone(y, root, dx=dx)
        self.flags[ikb] |= F_IK
        self.ik[ikb] = dict(target=target, loop=loop, angle=angle, links=list(links))
        ch = dict(root=root, links=links, target=target, ik=ikb)
        self.cur["chains"].append(ch)
        return ch

    def finish(self):
        nb = len(self.rest)
        for b in self.t5_past:
            self.ap[b] = nb + 5
        ik = None
        if self.ik:
            tgt, loop, ang, off, lb = [], [], [], [0], []
            for b in range(nb):
                d = self.ik.get(b)
                tgt.append(-1 if d is None else d["target"]); loop.append(0 if d is None else d["loop"])
                ang.append(0.0 if d is None else d["angle"])
                lb += [] if d is None else d["links"]
                off.append(len(lb))
            ik = dict(target=np.asarray(tgt, np.int32), loop=np.asarray(loop, np.int32), angle=np.asarray(ang, np.float32),
                      link_off=np.asarray(off, np.uint32), link_bone=np.asarray(lb, np.int32), link_limited=np.zeros(len(lb), np.uint8),
                      link_lo=np.zeros((len(lb), 3), np.float32), link_hi=np.zeros((len(lb), 3), np.float32))
        return (np.asarray(self.rest, np.float32), np.asarray(self.parent, np.int32), np.asarray(self.level, np.int32),
                np.asarray(self.flags, np.uint16), np.asarray(self.ap, np.int32), np.asarray(self.ar, np.float32), ik)


# ---- islands -------------------------------------------------------------------------------------------------------------------------
def _kind_name(kind):
    return {ROT: "rot", TR: "tr", ROTTR: "rottr"}[kind]


def t1(B, kind):
    B.island("t1_" + _kind_name(kind))
    r = B.bone(0)
    s = B.bone(0.5, r, steer=True)
    a = B.bone(0.5, r, dx=0.5)
    B.bone(1.0, a, dx=0.5)
    B.append(a, s, 0.5, kind, mixing=bool(kind & ROT))


def t2(B, kind):
    B.island("t2_" + _kind_name(kind))
    r = B.bone(0)
    a = B.bone(0.5, r, dx=0.5)
    B.bone(1.0, a, dx=0.5)
    s = B.bone(0.5, r, steer=True)
    B.append(a, s, 0.5, kind)


def t2_level(B):
    B.island("t2_level")
    r = B.bone(0)
    s = B.bone(0.5, r, level=2, steer=True)
    a = B.bone(0.5, r, dx=0.5)
    B.bone(1.0, a, dx=0.5)
    B.append(a, s, 1.0, ROTTR)


def t3(B):
    B.island("t3_pre_post")
    r = B.bone(0)
    a = B.bone(0.5, r, dx=0.5)
    B.bone(1.0, a, dx=0.5)
    p = B.bone(0.5, r, post=True, steer=True)
    B.append(a, p, 0.5, ROTTR)
    B.island("t3_post_pre")
    r = B.bone(0)
    s = B.bone(0.5, r, steer=True)
    a = B.bone(0.5, r, post=True, dx=0.5)
    B.bone(1.0, a, post=True, dx=0.5)
    B.append(a, s, 0.5, ROTTR, mixing=True)


def t4(B, kind):
    B.island("t4_" + _kind_name(kind))
    r = B.bone(0)
    a = B.bone(0.5, r, steer=True)
    B.bone(1.0, a)
    B.append(a, a, 0.5, kind)


def t5(B):
    B.island("t5_minus1")
    r = B.bone(0)
    a = B.bone(0.5, r, steer=True)
    B.bone(1.0, a)
    B.append(a, -1, 0.5, ROTTR)
    B.island("t5_past")
    r = B.bone(0)
    a = B.bone(0.5, r, steer=True)
    B.bone(1.0, a)
    B.append(a, -1, 0.5, ROTTR)
    B.t5_past.append(a)


def t6(B):
    B.island("t6_depth3")
    r = B.bone(0)
    s = B.bone(0.5, r, steer=True)
    prev = s
    for k in range(3):
        a = B.bone(0.5, r, dx=0.4 * (k + 1), steer=True)
        B.bone(1.0, a, dx=0.4 * (k + 1))
        B.append(a, prev, (0.5, 1.0, 2.0)[k], ROTTR)
        prev = a
    B.island("t6_against")
    r = B.bone(0)
    a1 = B.bone(0.5, r, dx=0.4, steer=True)
    B.bone(1.0, a1, dx=0.4)
    a2 = B.bone(0.5, r, dx=0.8, steer=True)
    B.bone(1.0, a2, dx=0.8)
    s = B.bone(0.5, r, steer=True)
    B.append(a1, a2, 0.5, ROT)
    B.append(a2, s, 1.0, TR)
    B.island("t6_cycle")
    r = B.bone(0)
    a = B.bone(0.5, r, dx=0.4, steer=True)
    B.bone(1.0, a, dx=0.4)
    b = B.bone(0.5, r, dx=0.8, steer=True)
    B.bone(1.0, b, dx=0.8)
    B.append(a, b, 0.5, ROTTR)
    B.append(b, a, 0.5, ROTTR)
    B.island("t6_tr_through_rot")
    r = B.bone(0)
    s = B.bone(0.5, r, steer=True)
    p = B.bone(0.5, r, dx=0.4, steer=True)
    B.bone(1.0, p, dx=0.4)
    a = B.bone(0.5, r, dx=0.8)
    B.bone(1.0, a, dx=0.8)
    B.append(p, s, 1.0, ROT)
    B.append(a, p, 1.0, TR)


def t7(B):
    B.island("t7_own_parent")
    r = B.bone(0)
    p = B.bone(0.5, r, steer=True)
    a = B.bone(1.0, p)
    B.bone(1.5, a)
    B.append(a, p, 0.5, ROTTR)
    B.island("t7_own_child")
    r = B.bone(0)
    c = B.bone(1.0, -1, steer=True)                               # the child first; its parent is set below
    a = B.bone(0.5, r)
    B.parent[c] = a
    B.append(a, c, 0.5, ROTTR)


def ratios(B):
    B.island("ratios")
    r = B.bone(0)
    s = B.bone(0.5, r, steer=True)
    for k, ratio in enumerate(RATIOS):
        a = B.bone(0.5, r, dx=0.3 * (k + 1))
        B.bone(1.0, a, dx=0.3 * (k + 1))
        B.append(a, s, ratio, ROTTR, mixing=True)


def i1(B):
    B.island("i1_rootward")
    ch = B.chain(3, 15, 0.5)
    B.cur["steer"] += ch["links"]
    B.append(ch["links"][0], ch["links"][2], 0.5, ROT)
    B.island("i1_tipward")
    ch = B.chain(3, 8, 2.0)
    B.cur["steer"] += ch["links"]
    B.append(ch["links"][2], ch["links"][0], 0.5, ROT)


def i2(B):
    B.island("i2_rot")
    ch = B.chain(3, 8, 0.5)
    B.bone(SEG * 5, ch["target"])
    B.cur["steer"] += ch["links"]
    B.append(ch["target"], ch["links"][1], 0.5, ROT)
    B.island("i2_tr")
    s = B.bone(0, dx=1.0, steer=True)
    ch = B.chain(2, 15, 2.0)
    B.bone(SEG * 4, ch["target"])
    B.append(ch["target"], s, 0.25, TR)


def i3(B):
    B.island("i3_tr")
    s = B.bone(0, dx=1.0, steer=True)
    ch = B.chain(3, 15, 0.5)
    B.bone(SEG * 5, ch["ik"])
    B.append(ch["ik"], s, 0.5, TR)
    B.island("i3_rot")
    s = B.bone(0, dx=1.0, steer=True)
    ch = B.chain(2, 8, 2.0)
    B.bone(SEG * 4, ch["ik"])
    B.append(ch["ik"], s, 0.5, ROT)


def i4(B):
    B.island("i4")
    r = B.bone(0, dx=1.0)
    before = B.bone(0.5, r, dx=1.0)
    B.bone(1.0, before, dx=1.0)
    ch = B.chain(3, 15, 0.5)
    B.cur["steer"] += ch["links"]
    after = B.bone(0.5, r, dx=1.5)
    B.bone(1.0, after, dx=1.5)
    B.append(before, ch["links"][1], 0.5, ROTTR)
    B.append(after, ch["links"][1], 0.5, ROTTR)


def i5(B):
    B.island("i5")
    r = B.bone(0, dx=1.0)
    from_ik = B.bone(0.5, r, dx=1.0)
    B.bone(1.0, from_ik, dx=1.0)
    ch = B.chain(2, 8, 2.0)
    B.cur["steer"] += [ch["target"], ch["ik"]]
    from_target = B.bone(0.5, r, dx=1.5)
    B.bone(1.0, from_target, dx=1.5)
    B.append(from_ik, ch["ik"], 0.5, ROTTR)
    B.append(from_target, ch["target"], 0.5, ROTTR)


def i6(B):
    B.island("i6")
    s = B.bone(0, dx=1.0, steer=True)
    root = B.bone(0)
    B.chain(3, 15, 2.0, root=root)
    B.append(root, s, 0.5, ROTTR, mixing=True)


def i7(B):
    """ik_exits' nested pair: IK bone b_, with a two-link chain of its own, is the only link of IK bone a_."""
    B.island("i7")
    s = B.bone(0, dx=1.0, steer=True)
    q0 = B.bone(0)
    q1 = B.bone(0.4, q0)
    q2 = B.bone(0.8, q1)
    tb = B.bone(1.2, q2)
    b_ = B.bone(1.2, q0, dx=0.1)
    ta = B.bone(1.6, b_, dx=0.1)
    a_ = B.bone(1.5, q0, dx=0.3)
    B.flags[b_] |= F_IK
    B.flags[a_] |= F_IK
    B.ik[b_] = dict(target=tb, loop=3, angle=1.0, links=[q2, q1])
    B.ik[a_] = dict(target=ta, loop=2, angle=1.0, links=[b_])
    B.cur["chains"] += [dict(root=q0, links=[q2, q1], target=tb, ik=b_), dict(root=q0, links=[b_], target=ta, ik=a_)]
    B.cur["steer"] += [q1, q2]
    B.append(q1, s, 0.5, ROT)
    B.cur["inner_link"] = q1


def _topo(B):
    for k in (ROT, TR, ROTTR):
        t1(B, k)
    for k in (ROT, TR, ROTTR):
        t2(B, k)
    t2_level(B); t3(B)
    for k in (ROT, TR, ROTTR):
        t4(B, k)
    t5(B); t6(B); t7(B); ratios(B)


def _ik(B):
    i1(B); t1(B, ROT); i2(B); i3(B); t1(B, ROTTR)


def _window(B):
    t1(B, ROT); i3(B); i4(B); t4(B, ROTTR); i5(B); i6(B); ratios(B); t1(B, ROTTR)


def _nested(B):
    i7(B); t1(B, ROT); i1(B); t4(B, ROT); i2(B); t1(B, ROTTR); t7(B)


RIGS = {"topo": _topo, "ik": _ik, "window": _window, "nested": _nested}
ALL_RIGS = sorted(RIGS)


def build_rig(name):
    """(rig = (rest, parent, level, flags, append_parent, append_ratio, ik), islands)."""
    B = Builder()
    RIGS[name](B)
    return B.finish(), B.islands


def flag_cleared(rig):
    """The rig with the append flags of the bones whose append parent is out of range cleared (T5's comparison)."""
    rest, parent, level, flags, ap, ar, ik = rig
    out = flags.copy()
    out[(ap < 0) | (ap >= rest.shape[0])] &= np.uint16(~(F_ROT | F_TR) & 0xFFFF)
    return rest, parent, level, out, ap, ar, ik


def sequence(rig):
    """seq[b] = position of bone b in the evaluation sequence (pre-physics list, then post-physics; each by level, then index)."""
    _, _, level, flags, _, _, _ = rig
    nb = flags.size
    order = sorted(range(nb), key=lambda b: (int(flags[b] >> 12 & 1), int(level[b]), b))
    seq = np.zeros(nb, int)
    seq[order] = np.arange(nb)
    return seq


def window_chain(rig, b):
    """Whether IK bone b's chain may run on the LDS window, by the rule csrc/rig.cpp states: link j's parent is link j + 1, the
    target hangs off link 0 and is no append bone, no append bone among the links, all bones distinct, at most 6 links, the
    root-most link's parent outside the chain (nested solves: none in the rigs this is asked of)."""
    _, parent, _, flags, ap, _, ik = rig
    nb = flags.size
    l0, l1 = int(ik["link_off"][b]), int(ik["link_off"][b + 1])
    links, tgt = [int(x) for x in ik["link_bone"][l0:l1]], int(ik["target"][b])

    def appends(x):
        return bool(flags[x] & (F_ROT | F_TR)) and 0 <= ap[x] < nb
    ok = 1 <= len(links) <= 6 and tgt != b and parent[tgt] == links[0] and not appends(tgt)
    ok = ok and len(set(links + [tgt, b])) == len(links) + 2 and not any(appends(x) for x in links)
    ok = ok and all(parent[links[j]] == links[j + 1] for j in range(len(links) - 1))
    return bool(ok and parent[links[-1]] not in links + [tgt])


# ---- candidate poses -----------------------------------------------------------------------------------------------------------------
BELOW_1 = np.nextafter(np.float32(1), np.float32(0))


def steered_quat(rng, kind):
    axis = rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    if kind in ("regular", "flipped"):
        a = rng.uniform(0.2, 1.5)
        q = np.concatenate([np.sin(a / 2) * axis, [np.cos(a / 2)]])
        return q if kind == "regular" else -q
    if kind == "identity":
        return np.array([0, 0, 0, 1.0])
    if kind == "w_below_1":
        return np.concatenate([np.sqrt(1 - float(BELOW_1) ** 2) * axis, [float(BELOW_1)]])
    if kind == "w_zero":
        return np.concatenate([axis, [0.0]])
    if kind == "w_above_1":
        return np.concatenate([0.2 * axis, [rng.uniform(1.05, 1.5)]])
    if kind in ("norm_0.5", "norm_1.5"):
        a = rng.uniform(2.0, 2.6)                                 # w in 0.27 .. 0.54: w * 1.5 stays below 1
        return float(kind[5:]) * np.concatenate([np.sin(a / 2) * axis, [np.cos(a / 2)]])
    return np.full(4, np.nan)


def pose_kind(q):
    """The POSE_KINDS class of a pose rotation, from its values (f32 [4])."""
    q = np.asarray(q, np.float32)
    if np.isnan(q).any():
        return "nan"
    n = float(np.sqrt(np.sum(q.astype(np.float64) ** 2)))
    if q[3] == 1 and not q[:3].any():
        return "identity"
    if q[3] == BELOW_1:
        return "w_below_1"
    if q[3] == 0:
        return "w_zero"
    if q[3] > 1:
        return "w_above_1"
    if abs(n - 0.5) < 1e-3:
        return "norm_0.5"
    if abs(n - 1.5) < 1e-3:
        return "norm_1.5"
    assert abs(n - 1) < 1e-3, q
    return "flipped" if q[3] < 0 else "regular"


def pool_poses(rig, islands, seed):
    """POOL candidate poses of the whole rig; island k's steered bones hold POSE_KINDS[(c + k) % 9] in candidate c."""
    nb = rig[0].shape[0]
    rng = np.random.RandomState(seed)
    poses = np.zeros((POOL, nb, 8), np.float32)
    iks = {ch["ik"] for isl in islands for ch in isl["chains"]}
    for c in range(POOL):
        for k, isl in enumerate(islands):
            kind = POSE_KINDS[(c + k) % len(POSE_KINDS)]
            for b in isl["bones"]:
                q = rng.normal(size=4) * 0.15 + (0, 0, 0, 1)
                poses[c, b, 4:8] = steered_quat(rng, kind) if b in isl["steer"] else q / np.linalg.norm(q)
                poses[c, b, 0:3] = rng.uniform(-0.5, 0.5, 3) if b in iks else rng.uniform(-0.2, 0.2, 3)
                if kind == "nan" and b in isl["steer"]:
                    poses[c, b, 0:3] = np.nan                     # a NaN parent ROTATION only makes the SLerp return identity
    return poses


# ---- the steered crowd ---------------------------------------------------------------------------------------------------------------
class Case:
    pass


_cases = {}


def solve_traced(oracle, rig, poses):
    """(palette, append trace [N, 9], IK trace [M, 8]) of one instance."""
    out = {}

    def run():
        out["ik"] = oracle.trace_ik(lambda: out.setdefault("pal", oracle.bone_solve_full(rig[0], rig[1], poses, *rig[2:])))
    out["ap"] = oracle.trace_append(run)
    return out["pal"], out["ap"], out["ik"]


def choose(branches, kinds, nan):
    """The candidate of each of the NI rows of ONE island: branches[c] = SLerp branch of the island's first mixing bone in candidate c
    (None: no mixing bone), kinds[c] its pose kind, nan[c] whether its palettes hold a NaN.  Greedy, deterministic."""
    used_kind, used, rows = {}, np.zeros(len(kinds), int), []
    for i in range(NI):
        want_nan = i in ix.NAN_ROWS
        g16 = {branches[c] for c in rows[i - i % 16:]}
        best, best_key = None, None
        for c in range(len(kinds)):
            if bool(nan[c]) != want_nan:
                continue
            key = (branches[c] in g16, used_kind.get(kinds[c], 0), used[c], c)
            if best_key is None or key < best_key:
                best, best_key = c, key
        rows.append(best)
        used[best] += 1
        used_kind[kinds[best]] = used_kind.get(kinds[best], 0) + 1
    return rows


def case(name, oracle=None):
    """The steered crowd of RIGS[name], computed once and never written: .rig, .islands, .poses [NI, NB, 8], .want [NI, NB, 16]
    (the oracle's palettes, computed with both traces on), .trace (per instance u32 [N, 9]), .ik_trace (per instance u32 [M, 8]),
    .records (all instances' append records with the instance as a first column, u32 [R, 10]), .island_of [NB], .seq [NB],
    .nan_rows (bool [NI]: some palette value of the instance is NaN), .picks [island][NI], .labels [NI][island]."""
    if name in _cases:
        return _cases[name]
    oracle = oracle or Oracle()
    rig, islands = build_rig(name)
    nb = rig[0].shape[0]
    pool = pool_poses(rig, islands, 4000 + ALL_RIGS.index(name))
    island_of = np.zeros(nb, int)
    for k, isl in enumerate(islands):
        island_of[isl["bones"]] = k
    solved = [solve_traced(oracle, rig, pool[c]) for c in range(POOL)]
    cs = Case()
    cs.name, cs.rig, cs.islands, cs.island_of, cs.seq = name, rig, islands, island_of, sequence(rig)
    cs.picks = []
    for k, isl in enumerate(islands):
        nan = [bool(np.isnan(pal[isl["bones"]]).any()) for pal, _, _ in solved]
        kinds = [POSE_KINDS[(c + k) % len(POSE_KINDS)] for c in range(POOL)]
        branches = [None] * POOL
        if isl["mixing"]:
            m = isl["mixing"][0]
            for c, (_, ap, _) in enumerate(solved):
                rec = ap[(ap[:, F["bone"]] == m) & (ap[:, F["context"]] == SEQ)]
                assert rec.shape[0] == 1, (name, isl["name"], "a mixing bone is evaluated once, in the sequence")
                branches[c] = int(rec[0, F["slerp"]])
        cs.picks.append(choose(branches, kinds, nan))
    poses = np.zeros((NI, nb, 8), np.float32)
    for k, isl in enumerate(islands):
        poses[:, isl["bones"]] = pool[cs.picks[k]][:, isl["bones"]]
    res = [solve_traced(oracle, rig, poses[i]) for i in range(NI)]
    cs.poses, cs.want = poses, np.stack([r[0] for r in res])
    cs.trace, cs.ik_trace = [r[1] for r in res], [r[2] for r in res]
    cs.records = np.concatenate([np.concatenate([np.full((t.shape[0], 1), i, np.uint32), t], axis=1) for i, t in enumerate(cs.trace)])
    cs.nan_rows = np.isnan(cs.want).any(axis=(1, 2))
    # per instance and island, the pose kind its steered bones hold (what test_ik_exits.assert_oracle prints with a mismatch)
    cs.labels = [[f"{isl['name']}:{POSE_KINDS[(cs.picks[k][i] + k) % len(POSE_KINDS)]}" for k, isl in enumerate(islands)] for i in range(NI)]
    # the islands are independent: an island's evaluations in the assembled crowd are those of the pool row it came from
    for k in range(len(islands)):
        for i in range(NI):
            mine, theirs = cs.trace[i], solved[cs.picks[k][i]][1]
            assert np.array_equal(mine[island_of[mine[:, 0]] == k], theirs[island_of[theirs[:, 0]] == k]), (name, islands[k]["name"], i)
    for a in (cs.poses, cs.want, cs.records):
        a.setflags(write=False)
    _cases[name] = cs
    return cs


# ---- classes -------------------------------------------------------------------------------------------------------------------------
def class_counts(cs):
    """{class: evaluations of the case that are it}, read off the append trace and the rig's tables (never off the island names).
    Classes that are about a bone WITHOUT records (T5) count instances."""
    rest, parent, level, flags, ap, ar, ik = cs.rig
    nb = flags.size
    rec = cs.records[:, 1:]
    b, p = rec[:, F["bone"]].astype(int), rec[:, F["parent"]].astype(int)
    kind, ctx, depth = rec[:, F["kind"]], rec[:, F["context"]], rec[:, F["depth"]]
    state, slerp = rec[:, F["parent_state"]], rec[:, F["slerp"]]
    post = (flags >> 12 & 1).astype(bool)
    appends = ((flags & (F_ROT | F_TR)) != 0) & (ap >= 0) & (ap < nb)
    seq = cs.seq
    out = {}

    def put(key, mask):
        out[key] = int(np.count_nonzero(mask))
    in_seq = ctx == SEQ
    same_list = post[b] == post[p]
    other = p != b
    t1_ = in_seq & other & same_list & (state == WRITTEN) & (seq[p] < seq[b])
    t2_ = in_seq & other & same_list & (state == UNWRITTEN) & (seq[p] > seq[b])
    chained = other & appends[p]                                  # T6: the append parent is an append bone itself
    for k, kn in ((ROT, "rot"), (TR, "tr"), (ROTTR, "rot+tr")):
        put(f"T1 parent earlier, {kn}", t1_ & (kind == k))
        put(f"T2 parent later, {kn}", t2_ & (kind == k))
        put(f"T4 names itself, {kn}", (state == SELF) & (p == b) & (kind == k))
        put(f"T6 chained, {kn}", chained & (kind == k))
    put("T2 later by index", t2_ & (level[p] == level[b]) & (p > b))
    put("T2 later by level", t2_ & (level[p] > level[b]) & (p < b))
    put("T3 pre reads post (reset state)", in_seq & ~post[b] & post[p] & (state == UNWRITTEN))
    put("T3 post reads pre", in_seq & post[b] & ~post[p] & (state == WRITTEN))
    flagged_out = [x for x in range(nb) if flags[x] & (F_ROT | F_TR) and not appends[x]]
    for key, want in (("T5 parent -1, flag set, no record", -1), ("T5 parent nb + 5, flag set, no record", nb + 5)):
        bones = [x for x in flagged_out if ap[x] == want]
        out[key] = NI * len(bones) if bones and not np.isin(b, bones).any() else 0
    pp = np.where(appends[p], ap[p], -1)                          # the parent's append parent
    ppp = np.where((pp >= 0) & appends[pp], ap[pp], -1)
    cyc = chained & (pp == b)
    put("T6 depth 3 in evaluation order", chained & ~cyc & (state == WRITTEN) & (ppp >= 0) & (seq[pp] < seq[p]) & (seq[ppp] < seq[pp])
        & (seq[p] < seq[b]))
    put("T6 depth 2 against evaluation order", chained & ~cyc & (state == UNWRITTEN) & (pp >= 0) & (seq[pp] > seq[p]) & (seq[p] > seq[b]))
    put("T6 two-cycle, first (reads the reset state)", cyc & (state == UNWRITTEN))
    put("T6 two-cycle, second (reads the written one)", cyc & (state == WRITTEN))
    put("T6 tr through a rot-only append bone", chained & ((kind & TR) != 0) & ((flags[p] >> 8 & 3) == ROT))
    put("T7 append parent is the bone's parent", other & (parent[b] == p))
    put("T7 append parent is the bone's child", other & (parent[p] == b))
    for r in RATIOS:
        put(f"ratio {r:g} on rot+tr", (kind == ROTTR) & (rec[:, F["ratio_bits"]] == np.float32(r).view(np.uint32)))
    # IK interplay
    if ik is not None:
        ikb = [x for x in range(nb) if flags[x] & F_IK]
        link_of, link_pos, target_of = {}, {}, {}
        for x in ikb:
            links = [int(y) for y in ik["link_bone"][ik["link_off"][x]:ik["link_off"][x + 1]]]
            for j, y in enumerate(links):
                link_of[y], link_pos[y] = x, j
            target_of[int(ik["target"][x])] = x
        nested_inner = {x for x in ikb if x in link_of or x in target_of}            # an IK bone that is a link / target of another
        win = {x for x in ikb if not nested_inner and window_chain(cs.rig, x)}
        own = np.array([link_of.get(x, -1) for x in range(nb)])
        pos = np.array([link_pos.get(x, -1) for x in range(nb)])
        tof = np.array([target_of.get(x, -1) for x in range(nb)])
        is_ik = np.isin(np.arange(nb), ikb)
        in_win_link = np.array([link_of.get(x, -1) in win for x in range(nb)])
        first = ctx == FIRST
        same_chain = (own[b] >= 0) & (own[b] == own[p]) & other
        put("I1 append link, parent a link of its chain, root-ward", first & same_chain & (pos[p] > pos[b]))
        put("I1 append link, parent a link of its chain, tip-ward", first & same_chain & (pos[p] < pos[b]))
        put("I1 append link, parent outside the chain", first & (own[b] >= 0) & (own[p] != own[b]) & (tof[p] != own[b]))
        loop_t = (ctx == LOOP) & (tof[b] >= 0)
        put("I2 append target in the loop, rot from a link of its chain", loop_t & ((kind & ROT) != 0) & (own[p] == tof[b]))
        put("I2 append target in the loop, tr from outside", loop_t & ((kind & TR) != 0) & (own[p] != tof[b]) & (cs.island_of[p] == cs.island_of[b]))
        put("I3 the IK bone appends, tr", in_seq & is_ik[b] & ((kind & TR) != 0))
        put("I3 the IK bone appends, rot", in_seq & is_ik[b] & ((kind & ROT) != 0))
        i4_ = in_seq & in_win_link[p] & (own[b] < 0)
        put("I4 parent a window chain's link, read before the IK bone", i4_ & (seq[b] < seq[np.maximum(own[p], 0)]))
        put("I4 parent a window chain's link, read after the IK bone", i4_ & (seq[b] > seq[np.maximum(own[p], 0)]))
        put("I5 parent is a target", in_seq & (tof[p] >= 0) & other & (tof[b] < 0) & (own[b] < 0))
        put("I5 parent is an IK bone", in_seq & is_ik[p] & other)
        roots = {int(parent[int(ik["link_bone"][ik["link_off"][x + 1] - 1])]) for x in win}
        put("I6 an append bone is the parent of a window chain's root-most link", in_seq & np.isin(b, list(roots)))
        put("I7 append link in a nested (inner) chain", first & (depth == 2) & np.isin(own[b], list(nested_inner)))
        put("a window chain's IK bone appends", in_seq & np.isin(b, list(win)))
    # SLerp input: the branch taken, and the pose of the parent it came from where that pose is what the parent holds
    # (a plain bone, written in the sequence: total rotation = pose rotation)
    plain = ~appends & ~is_link_mask(cs.rig)
    direct = (state == WRITTEN) & plain[p] & ((kind & ROT) != 0)
    pk = np.array([POSE_KINDS.index(pose_kind(cs.poses[i, x, 4:8])) for i, x in zip(cs.records[:, 0], p)])
    put("S regular", slerp == S_REGULAR)
    put("S flipped (w < 0)", (slerp == S_FLIP) & direct & (pk == POSE_KINDS.index("flipped")))
    put("S identity pose on a written parent (omega <= 1e-7)", (slerp == S_SMALL) & direct & (pk == POSE_KINDS.index("identity")))
    put("S w = the largest float below 1", (slerp == S_REGULAR) & direct & (pk == POSE_KINDS.index("w_below_1")))
    put("S w = 0", (slerp == S_REGULAR) & direct & (pk == POSE_KINDS.index("w_zero")))
    put("S un-normalised, w > 1 (NaN omega -> identity)", (slerp == S_NAN) & direct & (pk == POSE_KINDS.index("w_above_1")) & (rec[:, F["nan"]] == 0))
    put("S un-normalised, norm 0.5", direct & (pk == POSE_KINDS.index("norm_0.5")) & np.isin(slerp, (S_REGULAR, S_FLIP)))
    put("S un-normalised, norm 1.5", direct & (pk == POSE_KINDS.index("norm_1.5")) & np.isin(slerp, (S_REGULAR, S_FLIP)))
    put("S NaN pose (NaN rows only)", (slerp == S_NAN) & direct & (pk == POSE_KINDS.index("nan")))
    put("NaN total after the append", rec[:, F["nan"]] == 1)
    put("S unwritten parent (omega <= 1e-7)", (slerp == S_SMALL) & (state == UNWRITTEN))
    return out


def is_link_mask(rig):
    ik = rig[6]
    out = np.zeros(rig[3].size, bool)
    if ik is not None:
        out[ik["link_bone"]] = True
    return out


TOPOLOGY = [f"{t}, {k}" for t in ("T1 parent earlier", "T2 parent later", "T4 names itself", "T6 chained") for k in ("rot", "tr", "rot+tr")] + [
    "T2 later by index", "T2 later by level", "T3 pre reads post (reset state)", "T3 post reads pre", "T5 parent -1, flag set, no record",
    "T5 parent nb + 5, flag set, no record", "T6 depth 3 in evaluation order", "T6 depth 2 against evaluation order",
    "T6 two-cycle, first (reads the reset state)", "T6 two-cycle, second (reads the written one)", "T6 tr through a rot-only append bone",
    "T7 append parent is the bone's parent", "T7 append parent is the bone's child"] + [f"ratio {r:g} on rot+tr" for r in RATIOS]
SLERP = ["S regular", "S flipped (w < 0)", "S identity pose on a written parent (omega <= 1e-7)", "S w = the largest float below 1", "S w = 0",
         "S un-normalised, w > 1 (NaN omega -> identity)", "S un-normalised, norm 0.5", "S un-normalised, norm 1.5", "S NaN pose (NaN rows only)",
         "S unwritten parent (omega <= 1e-7)", "NaN total after the append"]
I123 = ["I1 append link, parent a link of its chain, root-ward", "I1 append link, parent a link of its chain, tip-ward",
        "I2 append target in the loop, rot from a link of its chain", "I2 append target in the loop, tr from outside"]
# rig -> the classes it must realise (every class of the issue is in at least one list)
REQUIRED = {
    "topo": TOPOLOGY + SLERP,
    "ik": I123 + ["I3 the IK bone appends, tr", "I3 the IK bone appends, rot"] + SLERP,
    "window": ["I3 the IK bone appends, tr", "I3 the IK bone appends, rot", "a window chain's IK bone appends",
               "I4 parent a window chain's link, read before the IK bone", "I4 parent a window chain's link, read after the IK bone",
               "I5 parent is a target", "I5 parent is an IK bone", "I6 an append bone is the parent of a window chain's root-most link"]
    + [f"ratio {r:g} on rot+tr" for r in RATIOS] + SLERP,
    "nested": ["I7 append link in a nested (inner) chain", "T7 append parent is the bone's parent", "T7 append parent is the bone's child"] + I123 + SLERP,
}


def label(r):
    """One trace record -> the histogram's key."""
    r = [int(x) for x in r]
    return "/".join([Oracle.APPEND_KINDS[r[F["kind"]]], Oracle.APPEND_CONTEXTS[r[F["context"]]], "depth%d" % r[F["depth"]],
                     Oracle.APPEND_PARENT_STATES[r[F["parent_state"]]], Oracle.APPEND_SLERPS[r[F["slerp"]]]] + (["nan"] if r[F["nan"]] else []))


def histogram(cs):
    """{island name: {label: evaluations}} of a case."""
    out = {isl["name"]: {} for isl in cs.islands}
    for r in cs.records:
        h = out[cs.islands[cs.island_of[int(r[1])]]["name"]]
        h[label(r[1:])] = h.get(label(r[1:]), 0) + 1
    return {k: dict(sorted(h.items())) for k, h in out.items()}


def neighbour_report(cs, order=None):
    """Per mixing bone: the smallest number of different SLerp branches in an aligned group of 16 instances taken in `order`."""
    order = list(range(NI)) if order is None else [int(i) for i in order]
    out = {}
    for isl in cs.islands:
        for m in isl["mixing"]:
            br = []
            for i in order:
                t = cs.trace[i]
                rec = t[(t[:, F["bone"]] == m) & (t[:, F["context"]] == SEQ)]
                br.append(int(rec[0, F["slerp"]]))
            out[(isl["name"], m)] = min(len(set(br[g:g + 16])) for g in range(0, len(order), 16))
    return out


def load_golden():
    with open(GOLDEN) as f:
        return json.load(f)

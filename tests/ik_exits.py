"""Steered CCD-IK cases: crowds whose every solve is known, from the oracle's exit trace, by the way it leaves the loop.

The device's CCD loop (ccd() in csrc/rig_kernels.hip, its sixteen-lane copy csrc/ik_coop_body.inl) carries a shortcut the reference
does not have: on a window chain, a sweep that reproduces every link's IK rotation bit for bit skips the rest of its half of the
iterations.  Oracle.trace_ik records, per solve, the exit (reached before the loop / reached after a sweep / ran out / loop count 0),
the sweeps run, the first reproducing sweep of each half and whether a NaN is present; this module uses it to CHOOSE the instances of
its crowds, so that every exit, every position of a repeat relative to ikt = loop / 2, and every link kind is present, and so that
neighbouring instances leave the loop at different sweeps (the lanes of a wave diverge).

Rigs.  A rig is a row of independent line chains, one per CONFIGS row (loop count, angle limit, link kinds are the chain's, not the
instance's): root, n links at 0.5 apart along +y, the target as child of link 0, the IK bone as child of the root resting on the
target.  Window rigs: 1, 3 and 6 links (6 = kMaxFastLinks).  Non-window rigs, one per reason a chain leaves the LDS window: 7 links;
an append bone among the links; a target that hangs off a bone between link 0 and itself.  "nested": the 3-link window rig plus one
unrelated nested IK pair, which puts the whole rig on the NESTED kernel variant.

Instances.  A seeded pool of POOL candidate poses per chain (IK-bone translations random in +-1, +-0.05 and +-4 over slightly bent
links; axis-aligned ones over straight links: 0, +-0.3 y, +5 y = collinear, below the root-most link = opposed, 0.2 x, 1e-4 x; on
the sphere link 0 swings the target over, which a one-link chain reaches after angle / angle-limit sweeps; the IK bone pulled onto a
link's own position = 0/0 = NaN) is solved and traced on the whole rig; the chains are independent, so each chain
then picks its own NI = 96 candidates, greedily: in every aligned group of 4 instances as many different exit sweeps as it can get,
in every aligned group of 16 as many classes, rare classes first.  NaN candidates go to the rows NAN_ROWS only and nothing else does:
at most one eighth of every prefix the tests use (1, 5, 16, 17, 96) is a NaN instance.  select_ids() permutes the instances in a way
that maps aligned groups of 4 onto aligned groups of 4 and aligned groups of 16 onto aligned groups of 16, so both neighbour conditions
hold in list order as well, and appends an id that is no row (cell 96: a workgroup of its own whose only listed cell is dead).

What can and cannot hold per chain.  The neighbour conditions (>= 3 distinct exit sweeps in every aligned 4, >= 6 classes in every
aligned 16) are asserted for the chains marked `mixing` in CONFIGS: six per rig, free and limited links, loops 8 to 256.  Of the others,
some cannot meet them by arithmetic -- loop 0, 1, 2 and 3 have at most 1, 2, 3 and 4 possible sweep counts of which a pose reaches
few, all-fixed links and angle limit 0 repeat at sweep 0 whatever the pose -- and the rest (fixed-axis links, which never reach their
target in a one-link chain) do not meet them in every rig.  They share waves with the mixing chains in the ordered kernel (slot k of a
workgroup runs event k of the round), and ik_coop_kernel gives them blocks of their own.  The far_target rig is exempt as a whole:
libmmd does not re-place the bone between link 0 and the target inside the loop, the target never moves and no solve reaches it.

Classes 8 and 9 of the issue (a first-half repeat with no second-half repeat before the loop ends; a first-half repeat followed by
"reached" in the second half): the search was widened once (WIDENED below).  It found class 8 -- the narrowx* chains carry it into every
window rig -- and never class 9.

tests/golden/ik_exit_classes.json pins the class histogram of the chosen cases."""
import json
import os

import numpy as np

from oracle.pyoracle import Oracle

SEG = 0.5
NI = 96
POOL = 384
NAN_ROWS = (9, 14, 25, 38, 51, 60, 77, 90)       # 0 of the first 5, 2 of the first 16 and 17, 8 of 96: at most one eighth of each
NIS = (1, 5, 16, 17, NI)
NONE = Oracle.IK_NONE
PI = float(np.pi)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ik_exit_classes.json")

# link kind -> (lo, hi) of a limited link, None = not limited; LINK_CLASS = what the Poser ctor makes of it: (Euler order, fixed axis)
KINDS = {
    "free": None,
    "knee": ((-PI, 0, 0), (-0.0087, 0, 0)),                     # the usual MMD knee
    "box": ((-1, -0.5, -0.3), (1, 0.5, 0.3)),
    "xyz": ((-2, -1, -0.3), (2, 1, 0.3)),                       # x reaches past +-pi/2: the first Euler-order fallback
    "yzx": ((-2, -2, -0.3), (2, 2, 0.3)),                       # x and y do: the second
    "yonly": ((0, -1, 0), (0, 1, 0)),
    "zonly": ((0, 0, -1), (0, 0, 1)),
    "fixed": ((0, 0, 0), (0, 0, 0)),
    "narrowx": ((-0.2, 0, 0), (0.2, 0, 0)),                     # the first half's reflection rule settles where the clamp does not
}
LINK_CLASS = {"knee": ("XYZ", "X"), "box": ("ZXY", None), "xyz": ("XYZ", None), "yzx": ("YZX", None), "yonly": ("ZXY", "Y"),
              "zonly": ("ZXY", "Z"), "fixed": ("ZXY", "ALL"), "narrowx": ("ZXY", "X")}


def link_class(lo, hi):
    """(Euler order, fixed axis) as poser_impl.inl:63-90 derives them (the float `abs`, the double pi * 0.5f)."""
    lo, hi = np.minimum(np.float32(lo), np.float32(hi)), np.maximum(np.float32(lo), np.float32(hi))
    half_pi = 3.141592653589793 * 0.5
    order = "ZXY" if lo[0] > -half_pi and hi[0] < half_pi else "XYZ" if lo[1] > -half_pi and hi[1] < half_pi else "YZX"
    z = [bool(abs(lo[k]) < np.float32(1e-7) and abs(hi[k]) < np.float32(1e-7)) for k in range(3)]
    fix = "ALL" if all(z) else "X" if z[1] and z[2] else "Y" if z[0] and z[2] else "Z" if z[0] and z[1] else None
    return order, fix


# name, link kinds (a kind = that kind on the even links, free on the odd ones, "kind*" = on every link; "fixed" = every link;
# "sandwich" = free, fixed, free ...),
# loop, angle limit, mixing (the neighbour conditions are asserted for this chain)
CONFIGS = [
    ("free40", "free", 40, 0.5, True),
    ("free15", "free", 15, 2.0, True),
    ("knee15", "knee", 15, 4.0, False),
    ("knee8", "knee", 8, 0.5, False),
    ("box40", "box", 40, 0.5, True),
    ("xyz8", "xyz", 8, 2.0, True),
    ("yzx8", "yzx", 8, 2.0, True),
    ("yonly15", "yonly", 15, 2.0, False),
    ("zonly15", "zonly", 15, 2.0, False),
    ("fixed40", "fixed", 40, 0.5, False),
    ("sandwich15", "sandwich", 15, 2.0, False),
    ("angle0", "free", 40, 0.0, False),
    ("loop0", "knee", 0, 0.5, False),
    ("loop1", "box*", 1, 0.5, False),
    ("loop2", "knee", 2, 0.5, False),
    ("loop3", "knee", 3, 0.5, False),
    ("loop5", "knee", 5, 2.0, False),
    ("loop255", "knee", 255, 0.03, False),
    ("loop256", "free", 256, 0.03, False),
    ("loop257", "knee", 257, 0.03, False),
    ("loopneg", "box", -1, 0.03, True),
    ("narrowx4", "narrowx*", 4, 4.0, False),                   # the widened search's finds (WIDENED below)
    ("narrowx5", "narrowx*", 5, 2.0, False),
    ("narrowx9", "narrowx*", 9, 4.0, False),
    ("narrowx15", "narrowx*", 15, 2.0, False),
    ("narrowx40", "narrowx*", 40, 2.0, False),
    ("narrowx40b", "narrowx*", 40, 4.0, False),
]
FEW = [c for c in CONFIGS if c[0] in ("free40", "knee15", "box40", "sandwich15", "loop1", "loop3")]   # the non-window rigs' chains
RIGS = {                                        # name -> (links per chain, variant, configs, runs on the LDS window)
    "line1": (1, "plain", [c for c in CONFIGS if c[1] != "sandwich"], True),
    "line3": (3, "plain", CONFIGS, True),
    "line6": (6, "plain", CONFIGS, True),
    "links7": (7, "plain", FEW, False),
    "append": (3, "append", FEW, False),
    "far_target": (3, "far_target", FEW, False),
    "nested": (3, "nested", CONFIGS, True),
}
WINDOW_RIGS = ("line1", "line3", "line6")
# The search, widened once for the issue's classes 8 and 9, on the CPU oracle: link kinds free, knee, box, yonly, zonly, xyz, yzx, a
# narrow x-only range (+-0.2), a narrow box (+-0.1) and a one-sided box, once on the even links with free links between and once on
# every link; loops 1, 3, 4, 5, 7, 8, 9, 15, 40; angle limits 0.03, 0.5, 2, 4; the 384 candidate poses above; chains of 1, 3 and 6
# links: 645 120 traced solves.
WIDENED = {
    "solves": 645120,
    "8 first-half repeat, no second-half repeat": "found (318 solves), with limited links only and nearly always the narrow x-only range on "
    "every link, where the first half's reflection settles and the second half's clamp keeps moving: the narrowx* chains of CONFIGS",
    "9 first-half repeat, then reached in the second half": "not found in any of the 645 120 solves",
}


def kinds_of(kind, n):
    if kind == "fixed":
        return ["fixed"] * n
    if kind == "sandwich":
        return ["fixed" if j % 2 else "free" for j in range(n)]
    if kind.endswith("*"):
        return [kind[:-1]] * n
    return [kind if j % 2 == 0 else "free" for j in range(n)]


def build_rig(n_links, variant, configs):
    """(rig = (rest, parent, level, flags, append_parent, append_ratio, ik), chains): chain c = dict(name, cfg, root, links (link 0
    first), target, ik, kinds)."""
    rest, parent, flags, chains = [], [], [], []
    ap, ar = [], []
    ikd = dict(target=[], loop=[], angle=[], link_off=[0], link_bone=[], link_limited=[], link_lo=[], link_hi=[])

    def bone(pos, par, flag=0, ik=None):
        rest.append(pos); parent.append(par); flags.append(flag); ap.append(-1); ar.append(0.0)
        ikd["target"].append(-1 if ik is None else ik["target"])
        ikd["loop"].append(0 if ik is None else ik["loop"])
        ikd["angle"].append(0.0 if ik is None else ik["angle"])
        if ik is not None:
            for lb, kd in zip(ik["links"], ik["kinds"]):
                lim = KINDS[kd]
                ikd["link_bone"].append(lb); ikd["link_limited"].append(0 if lim is None else 1)
                ikd["link_lo"].append((0, 0, 0) if lim is None else lim[0]); ikd["link_hi"].append((0, 0, 0) if lim is None else lim[1])
        ikd["link_off"].append(len(ikd["link_bone"]))
        return len(rest) - 1

    for c, cfg in enumerate(configs):
        name, kind, loop, angle, _ = cfg
        x = 2.0 * c
        root = bone((x, 0, 0), -1)
        line = [root]
        for k in range(1, n_links + 1):
            line.append(bone((x, SEG * k, 0), line[-1]))
        links = line[:0:-1]                                       # link 0 = the bone next to the target
        y = SEG * (n_links + 1)
        hang = links[0]
        if variant == "far_target":                               # a bone that is no link between link 0 and the target
            hang = bone((x, y, 0), links[0])
            y += SEG
        target = bone((x, y, 0), hang)
        kinds = kinds_of(kind, n_links)
        ikb = bone((x, y, 0), root, 0x20, dict(target=target, loop=loop, angle=angle, links=links, kinds=kinds))
        if variant == "append":                                   # the middle link takes half of the root's rotation
            flags[links[1]] |= 0x0100
            ap[links[1]], ar[links[1]] = root, 0.5
        chains.append(dict(name=name, cfg=cfg, root=root, links=links, target=target, ik=ikb, kinds=kinds, y_ik=y))
    if variant == "nested":
        # one unrelated nested pair (synth.make_nested_ik_rig's first kind): IK bone B, with a two-link chain of its own, is the
        # only link of IK bone A, so B's solve runs inside A's whenever A places its link.  Small loops: the cost multiplies.
        x = 2.0 * len(configs)
        q0 = bone((x, 0, 0), -1)
        q1 = bone((x, 0.4, 0), q0)
        q2 = bone((x, 0.8, 0), q1)
        tb = bone((x, 1.2, 0), q2)
        b_ = bone((x + 0.1, 1.2, 0), q0, 0x20, dict(target=tb, loop=3, angle=1.0, links=[q2, q1], kinds=["free", "free"]))
        ta = bone((x + 0.1, 1.6, 0), b_)
        a_ = bone((x + 0.3, 1.5, 0), q0, 0x20, dict(target=ta, loop=2, angle=1.0, links=[b_], kinds=["free"]))
        nested = [q0, q1, q2, tb, b_, ta, a_]
    else:
        nested = []
    ik = dict(target=np.asarray(ikd["target"], np.int32), loop=np.asarray(ikd["loop"], np.int32), angle=np.asarray(ikd["angle"], np.float32),
              link_off=np.asarray(ikd["link_off"], np.uint32), link_bone=np.asarray(ikd["link_bone"], np.int32),
              link_limited=np.asarray(ikd["link_limited"], np.uint8), link_lo=np.asarray(ikd["link_lo"], np.float32).reshape(-1, 3),
              link_hi=np.asarray(ikd["link_hi"], np.float32).reshape(-1, 3))
    has_ap = variant == "append"
    rig = (np.asarray(rest, np.float32), np.asarray(parent, np.int32), None, np.asarray(flags, np.uint16),
           np.asarray(ap, np.int32) if has_ap else None, np.asarray(ar, np.float32) if has_ap else None, ik)
    return rig, chains, nested


# ---- candidate poses ---------------------------------------------------------------------------------------------------------------
AXIS_MOVES = ("zero", "up", "down", "collinear", "opposed", "side", "tiny")


def candidate(rng, k, n_links, reach=SEG):
    """Candidate k of a chain: (IK-bone translation, link rotations [n, 4] link 0 first, tag); reach = from link 0 to the target."""
    slot = k % 8
    rot = np.zeros((n_links, 4), np.float32)
    rot[:, 3] = 1
    tag = "random"
    if slot in (0, 1, 2, 3):                                      # random translation over bent links
        scale = (1.0, 1.0, 0.05, 4.0)[slot]
        t = rng.uniform(-scale, scale, 3)
        for j in range(n_links):
            axis = rng.normal(size=3)
            axis /= np.linalg.norm(axis)
            a = rng.uniform(-0.3, 0.3)
            rot[j] = np.concatenate([np.sin(a / 2) * axis, [np.cos(a / 2)]])
    elif slot == 4:                                               # axis-aligned over straight links
        tag = AXIS_MOVES[(k // 8) % len(AXIS_MOVES)]
        t = dict(zero=(0, 0, 0), up=(0, 0.3, 0), down=(0, -0.3, 0), collinear=(0, 5, 0), opposed=(0, -(SEG * n_links + 0.25), 0),
                 side=(0.2, 0, 0), tiny=(1e-4, 0, 0))[tag]
    elif slot == 6:                                               # within link 0's reach of the target: straight links, the IK bone
        tag = "on_sphere"                                         # on the sphere the target moves on when only link 0 turns
        th, ph = rng.uniform(0.05, 3.0), rng.uniform(0, 2 * np.pi)
        t = (reach * np.sin(th) * np.cos(ph), reach * np.cos(th) - reach, reach * np.sin(th) * np.sin(ph))
    elif slot == 5:                                               # random translation over straight links
        t = rng.uniform(-1, 1, 3)
        tag = "straight"
    else:                                                         # onto a link's own position: its direction to the IK bone is 0/0
        tag = "onto_link"
        t = (0, -SEG * (1 + (k // 8) % n_links), 0)
    return np.asarray(t, np.float32), rot, tag


def pool_poses(rig, chains, nested, variant, seed):
    """POOL candidate poses of the whole rig (every chain its own candidate k in row k) and the candidates' tags [POOL][chain]."""
    nb = rig[0].shape[0]
    rng = np.random.RandomState(seed)
    poses = np.zeros((POOL, nb, 8), np.float32)
    poses[..., 7] = 1
    tags = [[None] * len(chains) for _ in range(POOL)]
    for k in range(POOL):
        for c, ch in enumerate(chains):
            t, rot, tags[k][c] = candidate(rng, k, len(ch["links"]), SEG * (2 if variant == "far_target" else 1))
            if variant == "far_target" and tags[k][c] == "onto_link":
                t = t - np.float32([0, SEG, 0])                    # the IK bone rests one segment further out
            poses[k, ch["ik"], 0:3] = t
            poses[k, ch["links"], 4:8] = rot
            if variant == "append" and tags[k][c] in ("random", "straight"):   # the append parent turns, so the append bone does
                a = rng.uniform(-0.5, 0.5)
                poses[k, ch["root"], 4:8] = (0, 0, np.sin(a / 2), np.cos(a / 2))
        for b in nested:
            q = rng.normal(size=4) * 0.15 + (0, 0, 0, 1)
            poses[k, b, 4:8] = q / np.linalg.norm(q)
            poses[k, b, 0:3] = rng.uniform(-0.2, 0.2, 3)
    return poses, tags


# ---- classes -----------------------------------------------------------------------------------------------------------------------
def classify(rec):
    """One trace record -> the class name (the histogram's key)."""
    _, loop, kind, sweeps, r1, r2, nan, _ = (int(x) for x in rec)
    ikt = loop // 2
    first = None if r1 == NONE else "at_ikt-1" if r1 == ikt - 1 else "early"
    second = None if r2 == NONE else "at_ikt" if r2 == ikt else "at_last" if r2 == loop - 1 else "between"
    if kind == 0:
        name = "before_loop"
    elif kind == 3:
        name = "loop_zero"
    elif kind == 1:
        name = "reached_first_half" if sweeps <= ikt else "reached_second_half"
        if first:
            name += "+first_repeat_" + first
        if second:
            name += "+second_repeat_" + second
    elif first is None and second is None:
        name = "ran_out_no_repeat"
    elif first is None:
        name = "second_repeat_" + second
    elif second is None:
        name = "first_repeat_" + first + "_only"
    else:
        name = "both_repeat_" + first + "+" + second
    return ("nan:" if nan else "") + name


def as_fields(rec):
    return dict(zip(Oracle.IK_TRACE_FIELDS, (int(x) for x in rec)))


# required class -> predicate of a trace record (classes 1-7 of the issue with their sub-positions; 8 and 9 are wanted, not required)
def _ran(r): return r["exit"] == 2 and not r["nan"]
REQUIRED = {
    "1 reached before the loop": lambda r: r["exit"] == 0,
    "2 reached in the first half": lambda r: r["exit"] == 1 and r["sweeps"] <= r["loop"] // 2 and not r["nan"],
    "3 reached in the second half": lambda r: r["exit"] == 1 and r["sweeps"] > r["loop"] // 2 and not r["nan"],
    "4 ran out, no repeat": lambda r: _ran(r) and r["repeat_first_half"] == NONE and r["repeat_second_half"] == NONE,
    "5 second half only, at ikt": lambda r: _ran(r) and r["repeat_first_half"] == NONE and r["repeat_second_half"] == r["loop"] // 2,
    "5 second half only, between": lambda r: _ran(r) and r["repeat_first_half"] == NONE and r["repeat_second_half"] != NONE
    and r["loop"] // 2 < r["repeat_second_half"] < r["loop"] - 1,
    "5 second half only, at loop-1": lambda r: _ran(r) and r["repeat_first_half"] == NONE and r["repeat_second_half"] == r["loop"] - 1,
    "5 loop 1: the repeat is sweep 0": lambda r: _ran(r) and r["loop"] == 1 and r["repeat_second_half"] == 0,
    "6 both, first at ikt-1": lambda r: _ran(r) and r["repeat_second_half"] != NONE and r["repeat_first_half"] == r["loop"] // 2 - 1,
    "6 both, first earlier": lambda r: _ran(r) and r["repeat_second_half"] != NONE and r["repeat_first_half"] != NONE
    and r["repeat_first_half"] + 1 < r["loop"] // 2,
    "6 both, second at ikt": lambda r: _ran(r) and r["repeat_first_half"] != NONE and r["repeat_second_half"] == r["loop"] // 2,
    "6 both, second later": lambda r: _ran(r) and r["repeat_first_half"] != NONE and r["repeat_second_half"] != NONE
    and r["repeat_second_half"] > r["loop"] // 2,
    "7 NaN": lambda r: bool(r["nan"]),
}
WANTED = {
    "8 first-half repeat, no second-half repeat": lambda r: _ran(r) and r["repeat_first_half"] != NONE and r["repeat_second_half"] == NONE,
    "9 first-half repeat, then reached in the second half": lambda r: r["exit"] == 1 and not r["nan"] and r["repeat_first_half"] != NONE
    and r["sweeps"] > r["loop"] // 2,
}
# required chain-level class -> the chains of CONFIGS that are it; a solve counts when it enters the loop (or is loop 0 and not reached)
CHAIN_CLASSES = {
    "loop 0": ["loop0"], "loop 1": ["loop1"], "loop 2": ["loop2"], "loop 3": ["loop3"], "loop 255": ["loop255"], "loop 256": ["loop256"],
    "loop 257 (clamps to 256)": ["loop257"], "loop -1 (clamps to 256)": ["loopneg"], "angle limit 0": ["angle0"],
    "all links fixed": ["fixed40"], "a fixed link between two free ones": ["sandwich15"], "fix X, limited": ["knee15"],
    "fix Y, limited": ["yonly15"], "fix Z, limited": ["zonly15"], "Euler order XYZ (first fallback)": ["xyz8"],
    "Euler order YZX (second fallback)": ["yzx8"],
}
POSE_CLASSES = {"collinear (dot clamps to 1)": "collinear", "opposed (dot clamps to -1)": "opposed"}
MIN_PER_CLASS = 4


# ---- choosing and ordering ---------------------------------------------------------------------------------------------------------
def choose(trace, tags):
    """trace [POOL, 8] of ONE chain -> the candidate of each of the NI rows.  Greedy, deterministic: NaN candidates on NAN_ROWS only;
    every row takes the candidate that adds an exit sweep count to its aligned group of 4, then a class to its aligned group of 16,
    then the class (and pose tag) used least so far, then the candidate used least, then the lowest index."""
    labels = [classify(r) for r in trace]
    nan = trace[:, 6] != 0
    sweeps = trace[:, 3]
    used_label, used_tag, used = {}, {}, np.zeros(len(labels), int)
    rows = []
    for i in range(NI):
        want_nan = i in NAN_ROWS and nan.any()
        g4 = {int(sweeps[k]) for k in rows[i - i % 4:]}
        g16 = {labels[k] for k in rows[i - i % 16:]}
        best, best_key = None, None
        for k in range(len(labels)):
            if bool(nan[k]) != want_nan:
                continue
            key = (int(sweeps[k]) in g4, labels[k] in g16, used_label.get(labels[k], 0), used_tag.get(tags[k], 0), used[k], k)
            if best_key is None or key < best_key:
                best, best_key = k, key
        rows.append(best)
        used[best] += 1
        used_label[labels[best]] = used_label.get(labels[best], 0) + 1
        used_tag[tags[best]] = used_tag.get(tags[best], 0) + 1
    return rows


def select_ids(seed=5):
    """A list that presents the NI instances permuted -- the aligned blocks of 16 in another order, inside each the aligned groups of
    4 in another order, inside each the four instances in another order, so a group of 4 (16) cells holds a group of 4 (16)
    instances -- followed by an id that is no row."""
    rng = np.random.RandomState(seed)
    ids = []
    for b16 in rng.permutation(NI // 16):
        for g4 in rng.permutation(4):
            ids += [16 * b16 + 4 * g4 + int(e) for e in rng.permutation(4)]
    return np.asarray(ids + [NI + 7], np.uint32)


class Case:
    pass


_cases = {}


def case(name, oracle=None):
    """The steered crowd of RIGS[name], computed once and never written: .rig, .chains, .poses [NI, NB, 8], .want [NI, NB, 16] (the
    oracle's palettes), .trace [NI, chains, 8] (the record of chain c's solve in instance i), .labels, .tags, .nan_rows (bool [NI]:
    the trace marks a NaN in some solve of the instance), .window, .n_records (trace records per instance, nested solves included)."""
    if name in _cases:
        return _cases[name]
    oracle = oracle or Oracle()
    n_links, variant, configs, window = RIGS[name]
    rig, chains, nested = build_rig(n_links, variant, configs)
    seed = 1000 + sorted(RIGS).index(name)
    pool, tags = pool_poses(rig, chains, nested, variant, seed)
    col = {ch["ik"]: c for c, ch in enumerate(chains)}

    def traced(poses):
        out = {}
        rec = oracle.trace_ik(lambda: out.setdefault("pal", oracle.bone_solve_full(rig[0], rig[1], poses, *rig[2:])))
        per = np.zeros((len(chains), 8), np.uint32)
        seen = np.zeros(len(chains), int)
        for r in rec:
            if int(r[0]) in col:
                per[col[int(r[0])]] = r
                seen[col[int(r[0])]] += 1
        assert (seen == 1).all(), "every plain chain is solved exactly once per frame"
        return out["pal"], per, len(rec)

    pool_trace = np.stack([traced(pool[k])[1] for k in range(POOL)])            # [POOL, chains, 8]
    cs = Case()
    cs.name, cs.rig, cs.chains, cs.window, cs.nested_bones, cs.variant = name, rig, chains, window, nested, variant
    cs.picks = [choose(pool_trace[:, c], [t[c] for t in tags]) for c in range(len(chains))]
    poses = np.zeros((NI,) + pool.shape[1:], np.float32)
    for i in range(NI):
        poses[i] = pool[i]                                                      # bones outside the chains (the nested pair): row i's
        for c, ch in enumerate(chains):
            own = [ch["root"], ch["ik"], ch["target"]] + ch["links"]
            poses[i, own] = pool[cs.picks[c][i], own]
    res = [traced(poses[i]) for i in range(NI)]
    cs.poses, cs.want = poses, np.stack([r[0] for r in res])
    cs.trace = np.stack([r[1] for r in res])
    cs.n_records = [r[2] for r in res]
    cs.labels = [[classify(cs.trace[i, c]) for c in range(len(chains))] for i in range(NI)]
    cs.tags = [[tags[cs.picks[c][i]][c] for c in range(len(chains))] for i in range(NI)]
    cs.nan_rows = (cs.trace[:, :, 6] != 0).any(axis=1)
    # the chains are independent: a chain's solve in the assembled crowd is its solve in the pool row it came from
    for c in range(len(chains)):
        assert np.array_equal(cs.trace[:, c], pool_trace[cs.picks[c], c]), (name, chains[c]["name"])
    for a in (cs.poses, cs.want, cs.trace):
        a.setflags(write=False)
    _cases[name] = cs
    return cs


def histogram(cs):
    """{chain name: {class: instances}} of a case."""
    out = {}
    for c, ch in enumerate(cs.chains):
        h = {}
        for i in range(NI):
            h[cs.labels[i][c]] = h.get(cs.labels[i][c], 0) + 1
        out[ch["name"]] = dict(sorted(h.items()))
    return out


def class_counts(cs):
    """{required / wanted class: DIFFERENT solves of the case that are it} (a candidate that two rows of a chain share counts once)."""
    recs = {(c, cs.picks[c][i]): (as_fields(cs.trace[i, c]), cs.chains[c]["name"], cs.tags[i][c]) for i in range(NI) for c in range(len(cs.chains))}
    recs = list(recs.values())
    out = {k: sum(1 for r, _, _ in recs if p(r)) for k, p in list(REQUIRED.items()) + list(WANTED.items())}
    for k, names in CHAIN_CLASSES.items():
        out[k] = sum(1 for r, n, _ in recs if n in names and r["exit"] != 0)
    for k, tag in POSE_CLASSES.items():
        out[k] = sum(1 for r, _, t in recs if t == tag and r["exit"] != 0 and r["exit"] != 3)
    return out


def neighbour_report(cs, order=None):
    """Per mixing chain: (the smallest number of distinct exit sweeps in an aligned group of 4, the smallest number of classes in an
    aligned group of 16), the instances taken in `order` (default: as stored)."""
    order = list(range(NI)) if order is None else [int(i) for i in order]
    out = {}
    for c, ch in enumerate(cs.chains):
        if not ch["cfg"][4]:
            continue
        sw = [int(cs.trace[i, c, 3]) for i in order]
        lb = [cs.labels[i][c] for i in order]
        out[ch["name"]] = (min(len(set(sw[g:g + 4])) for g in range(0, len(order), 4)),
                           min(len(set(lb[g:g + 16])) for g in range(0, len(order), 16)))
    return out


def load_golden():
    with open(GOLDEN) as f:
        return json.load(f)

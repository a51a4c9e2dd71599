"""Append (inherit) bones at every topology: the steered crowds of tests/append_cases.py on every form of the device solve.

transform_at reads the append parent's totals as they stand at that moment; the round schedule, the LDS-window eligibility test, the
store order for a bone that names itself and the physics seam's Fix all depend on that read happening in the reference's order.
append_cases.py builds rigs of independent islands, one per topology, and picks, from the oracle's append trace, crowds in which
every class occurs and neighbouring instances take different SLerp branches; its docstring says which island realises what.  Here:

CPU -- the steering itself: the rigs are what they claim (vmd.Skeleton(...).info); every required class is there in at least
ik_exits.MIN_PER_CLASS evaluations; the neighbour condition in stored and in select-list order; an append target is re-evaluated once
per link step; NaN instances are exactly ik_exits.NAN_ROWS, at most one eighth of every case set, everything else finite; T5's
out-of-range parents give the palettes of the rig with the flag cleared and no record; the trace changes no bit; the oracle is
libmmd's on every steered instance, the seam case with overrides included; the pinned histogram.

GPU -- palettes against the oracle with golden_util.assert_bits_equal_or_both_nan on EVERY instance plus equal NaN positions: the
default, then (MMDX_IK_COOP, MMDX_SOLVE_DENSE) in all four settings at 1, 5, 16, 17 and 96 instances, agreeing with each other; the
schedule against MMDX_SOLVE_SEQUENTIAL=1; the select call on a permuted list with an id that is no row and on its 37-row prefix;
the physics seam without overrides and with a strict override ON an append-translate bone and on an append parent; bone morphs on
an append parent and on an append bone."""
import numpy as np
import pytest

from oracle.pyoracle import Oracle, Reference, reference_available
from simple_mmd_renderer_amd import vmd
from tests import append_cases as ac
from tests import golden_util as gu
from tests import ik_exits as ix
from tests import test_solve_select as sel
from tests.test_ik_exits import COOP, DENSE, FORMS, assert_oracle, assert_same
from tests.test_physics_seam import random_transforms

F = ac.F


@pytest.fixture(autouse=True)
def _lib(hip_lib):
    return hip_lib


def is_nested(name):
    return name == "nested"


# ---- CPU: the steering ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ac.ALL_RIGS)
def test_rigs_are_what_they_claim(name):
    """Host side (creating a skeleton needs no device): at most about 150 bones, IK loops of at most 15, every append bone has a
    child, the append count, rounds that really are shared, sixteen-lane rounds exactly on the rig whose chains are all window chains."""
    rig, islands = ac.build_rig(name)
    rest, parent, level, flags, ap, ar, ik = rig
    nb = rest.shape[0]
    assert nb <= 150 and sorted(b for isl in islands for b in isl["bones"]) == list(range(nb))
    valid = ((flags & (ac.F_ROT | ac.F_TR)) != 0) & (ap >= 0) & (ap < nb)
    flagged = (flags & (ac.F_ROT | ac.F_TR)) != 0
    assert all((parent == b).any() for b in np.flatnonzero(flagged)), "every append bone has a child"
    sk = vmd.Skeleton(*rig)
    assert sk.info["n_append_bones"] == int(valid.sum()) > 0
    assert sk.info["n_solve_rounds"] < nb, "rounds are shared: fewer rounds than events"
    ikb = np.flatnonzero(flags & ac.F_IK)
    assert sk.info["n_ik_bones"] == ikb.size
    if ik is not None:
        assert int(ik["loop"].max()) <= 15
    if name == "topo":
        assert ikb.size == 0 and (flags & ac.F_POST).any() and int(flagged.sum()) - int(valid.sum()) == 2 and level.max() == 2
    if name == "window":
        assert all(ac.window_chain(rig, int(b)) for b in ikb) and sk.info["n_ik_rounds_16_lanes"] > 0
    if name == "ik":
        assert sum(ac.window_chain(rig, int(b)) for b in ikb) == 2 and ikb.size == 6          # the I3 chains only
    if name == "nested":
        assert sk.info["n_ik_rounds_16_lanes"] == 0               # (a rig with nested IK anywhere never takes ik_coop_kernel)
        assert any(int(ik["target"][b]) in ikb or set(ik["link_bone"][ik["link_off"][b]:ik["link_off"][b + 1]]) & set(ikb) for b in ikb)
    sk.close()


@pytest.mark.parametrize("name", ac.ALL_RIGS)
def test_every_required_class_is_realised(oracle, name):
    cs = ac.case(name, oracle)
    counts = ac.class_counts(cs)
    short = {k: counts[k] for k in ac.REQUIRED[name] if counts[k] < ix.MIN_PER_CLASS}
    assert not short, (name, short)


def test_every_class_of_the_issue_is_required_somewhere():
    everything = set().union(*[set(v) for v in ac.REQUIRED.values()])
    for k in ac.TOPOLOGY + ac.SLERP + ac.I123 + [
            "I3 the IK bone appends, tr", "I3 the IK bone appends, rot", "I4 parent a window chain's link, read before the IK bone",
            "I4 parent a window chain's link, read after the IK bone", "I5 parent is a target", "I5 parent is an IK bone",
            "I6 an append bone is the parent of a window chain's root-most link", "I7 append link in a nested (inner) chain"]:
        assert k in everything, k
    assert len(ac.TOPOLOGY) == 12 + 13 + len(ac.RATIOS)


@pytest.mark.parametrize("name", ac.ALL_RIGS)
def test_neighbours_take_different_slerp_branches(oracle, name):
    """Every aligned group of 16 instances holds all four SLerp branches, per mixing bone, as stored and as the select list
    presents them: the `omega > 1e-7` branch diverges across the instances of a slot."""
    cs = ac.case(name, oracle)
    ids = ix.select_ids()
    for order in (None, ids[:-1]):
        rep = ac.neighbour_report(cs, order)
        assert len(rep) >= 2
        assert all(n >= 4 for n in rep.values()), (name, rep)


@pytest.mark.parametrize("name", ["ik", "nested"])
def test_an_append_target_is_re_evaluated_once_per_link_step(oracle, name):
    """The in-loop records of an append target: one per link step of its solve (every link is free, so a sweep has one step per
    link and the IK trace's sweep count gives the steps), after one first-placement record."""
    cs = ac.case(name, oracle)
    chains = [ch for isl in cs.islands if isl["name"] in ("i2_rot", "i2_tr") for ch in isl["chains"]]
    assert len(chains) == 2
    steps = 0
    for i in range(ac.NI):
        t, k = cs.trace[i], cs.ik_trace[i]
        for ch in chains:
            solve = k[k[:, 0] == ch["ik"]]
            assert solve.shape[0] == 1
            mine = t[t[:, F["bone"]] == ch["target"]]
            assert (mine[:, F["context"]] == ac.FIRST).sum() == 1 and (mine[:, F["context"]] == ac.SEQ).sum() == 1
            assert (mine[:, F["context"]] == ac.LOOP).sum() == int(solve[0, 3]) * len(ch["links"]), (name, i)
            steps += int(solve[0, 3])
    assert steps > 2 * ac.NI                                      # the loops are entered


@pytest.mark.parametrize("name", ac.ALL_RIGS)
def test_nan_instances_are_the_marked_ones_and_few(oracle, name):
    cs = ac.case(name, oracle)
    assert np.flatnonzero(cs.nan_rows).tolist() == list(ix.NAN_ROWS)
    assert np.isfinite(cs.want[~cs.nan_rows]).all() and np.isfinite(cs.poses[~cs.nan_rows]).all()
    for ni in ix.NIS:
        assert 8 * int(cs.nan_rows[:ni].sum()) <= ni, (name, ni)
    assert 8 * int(cs.nan_rows[ix.select_ids()[:37]].sum()) <= 37


def test_out_of_range_parents_leave_no_record_and_change_nothing(oracle):
    """T5: the flag set with parent -1 / nb + 5 is the rig with the flag cleared, bit for bit, and the branch is never entered."""
    cs = ac.case("topo", oracle)
    cleared = ac.flag_cleared(cs.rig)
    bones = np.flatnonzero(cleared[3] != cs.rig[3])
    assert sorted(int(cs.rig[4][b]) for b in bones) == [-1, cs.rig[0].shape[0] + 5]
    assert not np.isin(cs.records[:, 1], bones).any()
    for i in range(ac.NI):
        gu.assert_bits_equal(oracle.bone_solve_full(cleared[0], cleared[1], cs.poses[i], *cleared[2:]), cs.want[i], f"instance {i}")


@pytest.mark.parametrize("name", ac.ALL_RIGS)
def test_traced_equals_untraced(oracle, name):
    """append_cases.case() computed .want with both traces on; the same solves with them off give the same bits, NaN payloads
    included.  And the trace's shape: nothing recorded without a solve, nine named columns."""
    cs = ac.case(name, oracle)
    for i in range(ac.NI):
        gu.assert_bits_equal(oracle.bone_solve_full(cs.rig[0], cs.rig[1], cs.poses[i], *cs.rig[2:]), cs.want[i], f"{name}, instance {i}")
    assert oracle.trace_append(lambda: None).shape == (0, 9) and len(Oracle.APPEND_TRACE_FIELDS) == 9
    depth = cs.records[:, 1 + F["depth"]]
    assert int(depth.max()) == dict(topo=0, window=0, ik=1, nested=2)[name]       # (the window rig has no append bone INSIDE a solve)
    assert ((cs.records[:, 1 + F["context"]] == ac.SEQ) == (depth == 0)).all()


def test_trace_records_say_what_the_evaluation_did(oracle):
    """The trace on a frame whose course is known without it: the rest pose.  Every written parent holds the identity (omega <=
    1e-7), translation-only bones report no SLerp, the ratio's bits are the rig's, no NaN."""
    cs = ac.case("topo", oracle)
    rest, parent, level, flags, ap, ar, ik = cs.rig
    poses = np.zeros((rest.shape[0], 8), np.float32)
    poses[:, 7] = 1
    rec = oracle.trace_append(lambda: oracle.bone_solve_full(rest, parent, poses, level, flags, ap, ar, ik))
    valid = np.flatnonzero(((flags & 0x0300) != 0) & (ap >= 0) & (ap < rest.shape[0]))
    assert sorted(rec[:, F["bone"]].tolist()) == valid.tolist()                  # FK only: one evaluation per append bone
    b = rec[:, F["bone"]]
    assert np.array_equal(rec[:, F["parent"]], ap[b]) and np.array_equal(rec[:, F["kind"]], flags[b] >> 8 & 3)
    assert np.array_equal(rec[:, F["ratio_bits"]], ar[b].view(np.uint32))
    assert (rec[:, F["slerp"]] == np.where(rec[:, F["kind"]] == ac.TR, ac.S_NONE, ac.S_SMALL)).all()
    assert not rec[:, F["nan"]].any() and not rec[:, F["context"]].any() and not rec[:, F["depth"]].any()
    assert np.array_equal(rec[:, F["parent_state"]] == ac.SELF, rec[:, F["parent"]] == b)
    seq = cs.seq
    other = rec[:, F["parent"]] != b
    assert np.array_equal(rec[other, F["parent_state"]] == ac.WRITTEN, seq[rec[other, F["parent"]]] < seq[b[other]])


def seam_overrides(cs):
    """The override list of the seam case: strict on an append-TRANSLATE bone (Fix re-derives its local matrix from the augmented
    translation) and on an append parent, Synchronize-only on another append parent and on a rot+tr bone with ratio 2."""
    by = {isl["name"]: isl for isl in cs.islands}
    flags, ap = cs.rig[3], cs.rig[4]
    tr_bone = by["t1_tr"]["bones"][2]
    strict_parent = by["t3_post_pre"]["steer"][0]
    loose_parent = by["t1_rot"]["steer"][0]
    ratio2 = [b for b in by["ratios"]["mixing"] if cs.rig[5][b] == 2.0][0]
    over = np.asarray([tr_bone, strict_parent, loose_parent, ratio2], np.int64)
    strict = np.asarray([1, 1, 0, 1], np.uint8)
    assert flags[tr_bone] >> 8 & 3 == ac.TR and (ap == strict_parent).any() and (ap == loose_parent).any() and flags[ratio2] >> 8 & 3 == ac.ROTTR
    assert not (flags[over] & ac.F_POST).any() and (flags[ap == strict_parent] & ac.F_POST).all()      # read across the seam
    xf = random_transforms(np.random.RandomState(77), ac.NI, over.size)
    return over, strict, xf


_seam = {}


def seam_want(oracle):
    """(over, strict, xf, the oracle's palettes [NI, NB, 16]) of the seam case with overrides: computed once."""
    if not _seam:
        cs = ac.case("topo", oracle)
        over, strict, xf = seam_overrides(cs)
        want = np.stack([oracle.bone_solve_physics(cs.rig[0], cs.rig[1], cs.poses[i], over, strict, xf[i], *cs.rig[2:])[0] for i in range(ac.NI)])
        want.setflags(write=False)
        _seam["v"] = (over, strict, xf, want)
    return _seam["v"]


def test_seam_overrides_change_the_append_bones(oracle):
    """The override case is not vacuous: the strict append-translate bone's palette differs from the plain solve's and from its
    override (Fix moved it), and the post-physics bone that reads the overridden parent across the seam is still the plain one
    (Synchronize and Fix write matrices, never the totals an append reads)."""
    cs = ac.case("topo", oracle)
    over, strict, xf, want = seam_want(oracle)
    ok = ~cs.nan_rows
    tr_bone = int(over[0])
    assert (gu.bits(want[ok, tr_bone]) != gu.bits(cs.want[ok, tr_bone])).any(axis=1).all()
    assert (gu.bits(want[ok, tr_bone]) != gu.bits(xf[ok, 0])).any(axis=1).all()
    reader = int(np.flatnonzero(cs.rig[4] == over[1])[0])
    gu.assert_bits_equal(want[ok, reader], cs.want[ok, reader], "the post-physics reader of an overridden parent")


@pytest.mark.skipif(not reference_available(), reason="oracle/_ref/libmmd_ref.so not built")
@pytest.mark.parametrize("name", ac.ALL_RIGS)
def test_oracle_equals_libmmd_on_every_steered_instance(oracle, name):
    cs = ac.case(name, oracle)
    ref = Reference.skeleton(*cs.rig)
    for i in range(ac.NI):
        gu.assert_bits_equal_or_both_nan(cs.want[i], ref.solve(cs.poses[i]), f"{name}, instance {i}")
    if name == "topo":
        over, strict, xf, want = seam_want(oracle)
        for i in range(ac.NI):
            gu.assert_bits_equal_or_both_nan(want[i], ref.solve_physics(cs.poses[i], over, strict, xf[i])[0], f"seam with overrides, instance {i}")
        morphs, rates = morph_case(cs)
        mref = Reference.skeleton(*cs.rig, morphs=morphs)
        for i in range(ac.NI):
            want_i = oracle.bone_solve_full(cs.rig[0], cs.rig[1], cs.poses[i], *cs.rig[2:], morphs, rates[i])
            gu.assert_bits_equal_or_both_nan(want_i, mref.solve(cs.poses[i], rates[i]), f"bone morphs, instance {i}")
        mref.close()
    ref.close()


def test_class_histogram_is_the_pinned_one(oracle):
    """A change to the oracle, the trace or the steering shows as a diff of classes (regenerate with append_cases.histogram)."""
    pinned = ac.load_golden()
    assert sorted(pinned) == ac.ALL_RIGS
    for name in ac.ALL_RIGS:
        assert ac.histogram(ac.case(name, oracle)) == pinned[name], name


# ---- GPU -------------------------------------------------------------------------------------------------------------------------------
def check_shape(sk, name, shape, coop, dense, cells, what, select=0):
    nested = int(is_nested(name))
    want = dict(solver="ordered", nested=nested, dense=int(dense == "1" and not nested), select=select, workgroups=(cells + 15) // 16)
    assert {k: shape[k] for k in want} == want, (what, shape)
    if coop == "1" and sk.info["n_ik_rounds_16_lanes"]:
        assert shape["coop_launches"] == sk.info["n_ik_rounds_16_lanes"] and shape["segments"] > 1, (what, shape, sk.info)
    else:
        assert shape["coop_launches"] == 0 and shape["segments"] == 1, (what, shape)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ac.ALL_RIGS)
def test_gpu_every_form_equals_the_oracle_and_the_others(monkeypatch, oracle, name):
    """The default with no environment first, then ik_coop_kernel / one lane per solve, each on the plain and the forced dense
    ordered kernel; the nested rig reports nested = 1 and is never dense; only the window rig launches ik_coop_kernel."""
    cs = ac.case(name, oracle)
    for v in (COOP, DENSE, "MMDX_SOLVE_SEQUENTIAL"):
        monkeypatch.delenv(v, raising=False)
    sk = vmd.Skeleton(*cs.rig)
    assert (sk.info["n_ik_rounds_16_lanes"] > 0) == (name == "window")
    default = sk.solve(cs.poses)
    assert_oracle(default, cs, range(ac.NI), f"{name}, default")
    check_shape(sk, name, sk.last_solve_shape(), "1", "0", ac.NI, f"{name}, default")
    for ni in ix.NIS:
        results = []
        for coop, dense in FORMS:
            what = f"{name}, {COOP}={coop}, {DENSE}={dense}, {ni} instances"
            monkeypatch.setenv(COOP, coop)
            monkeypatch.setenv(DENSE, dense)
            got = sk.solve(cs.poses[:ni])
            check_shape(sk, name, sk.last_solve_shape(), coop, dense, ni, what)
            assert_oracle(got, cs, range(ni), what)
            results.append(got)
        for got, form in zip(results[1:], FORMS[1:]):
            assert_same(got, results[0], f"{name}, {ni} instances: {form} vs {FORMS[0]}")
        assert_same(results[0], default[:ni], f"{name}, {ni} instances: the first rows of the full crowd")
    sk.close()
    if name == "topo":                                            # T5 on the device: the rig with the flags cleared, bit for bit
        monkeypatch.delenv(COOP)
        monkeypatch.delenv(DENSE)
        cleared = vmd.Skeleton(*ac.flag_cleared(cs.rig))
        assert cleared.info["n_append_bones"] == sk.info["n_append_bones"]
        assert_same(cleared.solve(cs.poses), default, "topo with T5's flags cleared")
        cleared.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ac.ALL_RIGS)
def test_gpu_round_schedule_equals_sequential(monkeypatch, oracle, name):
    """A skeleton created under MMDX_SOLVE_SEQUENTIAL=1 (one event per round, in sequence order) gives the scheduled one's bits:
    every dependency edge the schedule needs for an append read is there."""
    cs = ac.case(name, oracle)
    nb = cs.rig[0].shape[0]
    monkeypatch.delenv("MMDX_SOLVE_SEQUENTIAL", raising=False)
    sched = vmd.Skeleton(*cs.rig)
    monkeypatch.setenv("MMDX_SOLVE_SEQUENTIAL", "1")
    seq = vmd.Skeleton(*cs.rig)
    assert seq.info["n_solve_rounds"] == nb and sched.info["n_solve_rounds"] < nb
    a, b = sched.solve(cs.poses), seq.solve(cs.poses)
    assert_oracle(b, cs, range(ac.NI), f"{name}, sequential")
    assert_same(a, b, f"{name}: scheduled vs sequential")
    sched.close()
    seq.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ac.ALL_RIGS)
def test_gpu_select_permuted_list_with_an_id_that_is_no_row(monkeypatch, oracle, name):
    """mmdx_skeleton_solve_select: the whole permuted list (97 cells: the last workgroup's only listed cell is no row), then its
    first 37 (a partly empty workgroup; the other rows keep their pattern and their poses hold NaN)."""
    cs = ac.case(name, oracle)
    for v in (COOP, DENSE, "MMDX_SOLVE_SEQUENTIAL"):
        monkeypatch.delenv(v, raising=False)
    sk = vmd.Skeleton(*cs.rig)
    ids = ix.select_ids()
    for count in (ids.size, 37):
        what = f"{name}, select {count}"
        rows = sel.listed_rows(ids, count, ac.NI)
        assert rows.sum() == min(count, ac.NI)
        got = sel.run(sk, sel.nan_unlisted(cs.poses, rows), ids, count)
        check_shape(sk, name, sk.last_solve_shape(), "1", "0", ids.size, what, select=1)
        assert_oracle(got[rows], cs, np.flatnonzero(rows), what)
        assert (got[~rows].view(np.uint8) == sel.PATTERN).all(), what + ": a row that is not listed was written"
    sk.close()


@pytest.mark.gpu
def test_gpu_physics_seam_without_and_with_overrides(monkeypatch, oracle):
    """The rig that holds T3 through mmdx_skeleton_solve_pre / _post: an empty override list gives the plain solve's palettes (a
    pre-physics bone reads a post-physics one in its reset state, a post-physics one reads a pre-physics one across the seam);
    with overrides, physics_override_kernel's Fix reads the append-augmented translation of a strict append-translate bone."""
    cs = ac.case("topo", oracle)
    for v in (COOP, DENSE, "MMDX_SOLVE_SEQUENTIAL"):
        monkeypatch.delenv(v, raising=False)
    sk = vmd.Skeleton(*cs.rig, physics_seam=True)
    for ni in ix.NIS:
        sk.solve_pre(cs.poses[:ni])
        got = sk.solve_post(np.zeros(0, np.int32), np.zeros(0, np.uint8), np.zeros((ni, 0, 16), np.float32))
        assert_oracle(got, cs, range(ni), f"pre + post without overrides, {ni} instances")
    over, strict, xf, want = seam_want(oracle)
    for ni in (17, ac.NI):
        sk.solve_pre(cs.poses[:ni])
        got = sk.solve_post(over, strict, xf[:ni])
        for i in range(ni):
            assert_same(got[i], want[i], f"pre + overrides + post, {ni} instances: instance {i}")
    sk.close()


def morph_case(cs):
    """Bone morphs (translation and rotation) on an append parent, on an append bone and on a bone that names itself, and a
    group morph over the first two; rates per instance, 0, tiny, fractional, 1 and above."""
    by = {isl["name"]: isl for isl in cs.islands}
    bones = [by["t1_rottr"]["steer"][0], by["ratios"]["mixing"][4], by["t4_rottr"]["steer"][0], by["t6_depth3"]["steer"][1]]
    rng = np.random.RandomState(31)
    rot = rng.normal(size=(len(bones), 4)) * 0.4 + (0, 0, 0, 1)
    rot /= np.linalg.norm(rot, axis=1, keepdims=True)
    n = len(bones)
    morphs = dict(type=np.asarray([2] * n + [0], np.int32), offset=np.asarray(list(range(n + 1)) + [n + 2], np.uint32),
                  index=np.asarray(bones + [0, 1], np.uint32),
                  value=np.concatenate([rng.uniform(-0.5, 0.5, (n, 3)), [[0.5, 0, 0], [0.25, 0, 0]]]).astype(np.float32),
                  rotation=np.concatenate([rot, [[0, 0, 0, 1]] * 2]).astype(np.float32))
    rates = rng.choice([0, 5e-8, 0.3, 1.0, 1.7], (ac.NI, n + 1)).astype(np.float32)
    flags, ap = cs.rig[3], cs.rig[4]
    assert (ap == bones[0]).any() and flags[bones[1]] & 0x0300 and ap[bones[2]] == bones[2] and flags[bones[3]] & 0x0300
    return morphs, rates


@pytest.mark.gpu
def test_gpu_bone_morphs_on_append_parents_and_append_bones(monkeypatch, oracle):
    """mmdx_skeleton_solve_morphed: the morph's rotation and translation enter the totals BEFORE the append branch, on the parent
    (whose totals the append bone reads) and on the append bone itself."""
    cs = ac.case("topo", oracle)
    for v in (COOP, DENSE, "MMDX_SOLVE_SEQUENTIAL"):
        monkeypatch.delenv(v, raising=False)
    morphs, rates = morph_case(cs)
    sk = vmd.Skeleton(*cs.rig, morphs=morphs)
    got = sk.solve(cs.poses, morph_weights=rates)
    changed = 0
    for i in range(ac.NI):
        want = oracle.bone_solve_full(cs.rig[0], cs.rig[1], cs.poses[i], *cs.rig[2:], morphs, rates[i])
        assert_same(got[i], want, f"morphed, instance {i}")
        changed += int((gu.bits(want) != gu.bits(cs.want[i])).any())
    assert changed > ac.NI // 2
    sk.close()

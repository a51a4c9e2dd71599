"""CCD-IK at every way out of its loop: the steered crowds of tests/ik_exits.py on every form of the device solve.

The device's loop has a shortcut the reference lacks (a sweep that reproduces every link's IK rotation bit for bit skips the rest of
its half of the iterations; window chains only; written out twice: ccd() and ik_coop_body.inl).  ik_exits.py picks, from the oracle's
exit trace, crowds in which every exit and every position of a repeat relative to ikt = loop / 2 occurs, with neighbours that leave at
different sweeps; its docstring says how.  Here:

CPU -- the steering itself: every required class is there, in every window rig, at least MIN_PER_CLASS different solves; the neighbour
conditions in stored and in select-list order; NaN instances are exactly the rows the trace marks, at most one eighth of every case
set, everything else finite; the trace changes no bit; the oracle is libmmd's on every steered instance; the pinned histogram.

GPU -- palettes against the oracle with golden_util.assert_bits_equal_or_both_nan on EVERY instance (so NaN exactly where the oracle
has NaN), at 1, 5, 16, 17 and 96 instances: ik_coop_kernel and one lane per solve, each on the plain and the forced dense ordered
kernel, all four agreeing with each other; the NESTED variant; the select call on a permuted list with an id that is no row; the
physics-seam pair of calls without overrides; the motion -> palette call; the three rigs that stay off the LDS window."""
import numpy as np
import pytest

from oracle.pyoracle import Reference, reference_available
from simple_mmd_renderer_amd import vmd
from tests import golden_util as gu
from tests import ik_exits as ix
from tests import test_solve_select as sel

DENSE, COOP = "MMDX_SOLVE_DENSE", "MMDX_IK_COOP"
ALL_RIGS = sorted(ix.RIGS)
NEIGHBOUR_RIGS = [r for r in ALL_RIGS if r != "far_target"]     # (its chains never move their target: see test_neighbours_differ)


@pytest.fixture(autouse=True)
def _lib(hip_lib):
    return hip_lib


# ---- CPU: the steering ---------------------------------------------------------------------------------------------------------------
def test_link_kinds_are_what_they_claim():
    for kind, want in ix.LINK_CLASS.items():
        assert ix.link_class(*ix.KINDS[kind]) == want, kind
    orders = {ix.LINK_CLASS[k][0] for k in ix.LINK_CLASS}
    fixes = {ix.LINK_CLASS[k][1] for k in ix.LINK_CLASS}
    assert orders == {"ZXY", "XYZ", "YZX"} and fixes == {None, "X", "Y", "Z", "ALL"}
    assert ix.kinds_of("sandwich", 3) == ["free", "fixed", "free"] and set(ix.kinds_of("fixed", 6)) == {"fixed"}
    loops = {c[2] for c in ix.CONFIGS}
    assert {0, 1, 2, 3, 255, 256, 257, -1} <= loops and any(c[3] == 0.0 for c in ix.CONFIGS)


@pytest.mark.parametrize("name", ALL_RIGS)
def test_rigs_are_the_kind_they_claim(name):
    """Window rigs: every IK round runs sixteen lanes per solve, which the plan grants to rounds of window chains only; the other
    rigs have no such round.  (Host side: creating a skeleton needs no device.)"""
    n_links, variant, configs, window = ix.RIGS[name]
    rig, chains, nested = ix.build_rig(n_links, variant, configs)
    sk = vmd.Skeleton(*rig)
    assert sk.info["n_ik_bones"] == len(chains) + (2 if nested else 0)
    assert sk.info["n_ik_links"] == n_links * len(chains) + (3 if nested else 0)
    if window and not nested:
        assert sk.info["n_ik_rounds_16_lanes"] > 0
    else:                                                         # (a rig with nested IK anywhere never takes ik_coop_kernel)
        assert sk.info["n_ik_rounds_16_lanes"] == 0
    assert (n_links <= 6) == (name != "links7") and (rig[4] is not None) == (name == "append")
    if name == "far_target":
        assert all(rig[1][ch["target"]] != ch["links"][0] for ch in chains)
    sk.close()


@pytest.mark.parametrize("name", ix.WINDOW_RIGS + ("nested",))
def test_every_required_class_is_realised(oracle, name):
    cs = ix.case(name, oracle)
    counts = ix.class_counts(cs)
    required = list(ix.REQUIRED) + list(ix.CHAIN_CLASSES) + list(ix.POSE_CLASSES)
    if name == "line1":
        required.remove("a fixed link between two free ones")    # needs three links
    short = {k: counts[k] for k in required if counts[k] < ix.MIN_PER_CLASS}
    assert not short, (name, short)
    assert counts["8 first-half repeat, no second-half repeat"] >= ix.MIN_PER_CLASS        # found by the widened search: kept
    assert counts["9 first-half repeat, then reached in the second half"] == 0              # never found: ik_exits.WIDENED says so


@pytest.mark.parametrize("name", NEIGHBOUR_RIGS)
def test_neighbours_differ(oracle, name):
    """Every aligned group of 4 instances holds >= 3 distinct exit sweeps, every aligned group of 16 >= 6 classes, per mixing chain,
    as stored and as the select list presents them.  Not far_target: libmmd does not re-place the bone between link 0 and the target
    inside the loop, so the target never moves, no solve there ever reaches it and a chain has two or three sweep counts in all."""
    cs = ix.case(name, oracle)
    ids = ix.select_ids()
    assert sorted(ids[:-1].tolist()) == list(range(ix.NI)) and ids[-1] >= ix.NI and not np.array_equal(ids[:-1], np.arange(ix.NI))
    for order in (None, ids[:-1]):
        rep = ix.neighbour_report(cs, order)
        assert len(rep) >= 2
        assert all(s >= 3 and c >= 6 for s, c in rep.values()), (name, rep)


@pytest.mark.parametrize("name", ALL_RIGS)
def test_nan_instances_are_the_marked_ones_and_few(oracle, name):
    cs = ix.case(name, oracle)
    assert np.flatnonzero(cs.nan_rows).tolist() == list(ix.NAN_ROWS)
    has_nan = np.isnan(cs.want).any(axis=(1, 2))
    assert np.array_equal(has_nan, cs.nan_rows)                   # NaN palettes exactly where the trace marks a NaN solve ...
    assert np.isfinite(cs.want[~cs.nan_rows]).all()               # ... and everything else is finite
    for ni in ix.NIS:
        assert 8 * int(cs.nan_rows[:ni].sum()) <= ni, (name, ni)
    assert 8 * int(cs.nan_rows[ix.select_ids()[:37]].sum()) <= 37


@pytest.mark.parametrize("name", ALL_RIGS)
def test_traced_equals_untraced(oracle, name):
    """ik_exits.case() computed .want with the trace on; the same solves with it off give the same bits, NaN payloads included."""
    cs = ix.case(name, oracle)
    for i in range(ix.NI):
        gu.assert_bits_equal(oracle.bone_solve_full(cs.rig[0], cs.rig[1], cs.poses[i], *cs.rig[2:]), cs.want[i], f"{name}, instance {i}")
    assert min(cs.n_records) >= len(cs.chains)
    assert (min(cs.n_records) > len(cs.chains)) == (name == "nested")      # the nested pair's solves are recorded as well


@pytest.mark.skipif(not reference_available(), reason="oracle/_ref/libmmd_ref.so not built")
@pytest.mark.parametrize("name", ALL_RIGS)
def test_oracle_equals_libmmd_on_every_steered_instance(oracle, name):
    cs = ix.case(name, oracle)
    ref = Reference.skeleton(*cs.rig)
    for i in range(ix.NI):
        gu.assert_bits_equal_or_both_nan(cs.want[i], ref.solve(cs.poses[i]), f"{name}, instance {i}")
    ref.close()


def test_collinear_and_opposed_poses_clamp_the_dot_product(oracle):
    """The libm trace of a collinear (opposed) instance holds acos calls whose argument is exactly 1 (-1)."""
    cs = ix.case("line3", oracle)
    for tag, arg in (("collinear", 1.0), ("opposed", -1.0)):
        rows = [i for i in range(ix.NI) if not cs.nan_rows[i] and sum(t == tag for t in cs.tags[i]) >= 3]
        assert rows, tag
        for i in rows[:4]:
            rec = oracle.trace_libm(lambda: oracle.bone_solve_full(cs.rig[0], cs.rig[1], cs.poses[i], *cs.rig[2:]))
            acos = rec[rec[:, 0] == 4]
            assert (acos[:, 1] == np.float32(arg).view(np.uint32)).sum() >= 3, (tag, i)


def test_class_histogram_is_the_pinned_one(oracle):
    """A change to the oracle, the trace or the search shows as a diff of classes (regenerate with ik_exits.histogram)."""
    pinned = ix.load_golden()
    assert sorted(pinned) == ALL_RIGS
    for name in ALL_RIGS:
        assert ix.histogram(ix.case(name, oracle)) == pinned[name], name


def test_trace_records_say_what_the_solve_did(oracle):
    """The trace on three solves whose course is known without it: rest pose (reached before the loop), loop 0, all links fixed
    (every sweep reproduces: sweep 0 in the first half, sweep ikt in the second)."""
    cs = ix.case("line3", oracle)
    col = {ch["name"]: c for c, ch in enumerate(cs.chains)}
    poses = np.zeros((cs.rig[0].shape[0], 8), np.float32)
    poses[:, 7] = 1
    rec = oracle.trace_ik(lambda: oracle.bone_solve_full(cs.rig[0], cs.rig[1], poses, *cs.rig[2:]))
    assert rec.shape == (len(cs.chains), 8) and (rec[:, 2] == 0).all() and (rec[:, 3] == 0).all() and (rec[:, 6] == 0).all()
    assert sorted(rec[:, 0].tolist()) == sorted(ch["ik"] for ch in cs.chains) and (rec[:, 7] == 3).all()
    assert rec[col["loop257"], 1] == 256 and rec[col["loopneg"], 1] == 256 and rec[col["loop0"], 1] == 0
    for ch in cs.chains:
        poses[ch["ik"], 0:3] = (0.3, -0.2, 0.1)
    rec = oracle.trace_ik(lambda: oracle.bone_solve_full(cs.rig[0], cs.rig[1], poses, *cs.rig[2:]))
    by = {int(r[0]): ix.as_fields(r) for r in rec}
    z = by[cs.chains[col["loop0"]]["ik"]]
    assert ix.Oracle.IK_EXITS[z["exit"]] == "loop_zero" and z["sweeps"] == 0
    f = by[cs.chains[col["fixed40"]]["ik"]]
    assert ix.Oracle.IK_EXITS[f["exit"]] == "ran_out" and f["sweeps"] == 40 and f["repeat_first_half"] == 0 and f["repeat_second_half"] == 20
    assert oracle.trace_ik(lambda: None).shape == (0, 8)


# ---- GPU -------------------------------------------------------------------------------------------------------------------------------
def assert_oracle(got, cs, rows, what):
    """Every row of got against the oracle's palette of instance rows[k]: bits, NaN exactly where the oracle has NaN."""
    for k, i in enumerate(rows):
        gu.assert_bits_equal_or_both_nan(got[k], cs.want[i], f"{what}: instance {i} ({', '.join(sorted(set(cs.labels[i])))})")
        assert np.array_equal(np.isnan(got[k]), np.isnan(cs.want[i])), f"{what}: instance {i}: NaN where the oracle has none, or the reverse"


def assert_same(a, b, what):
    gu.assert_bits_equal_or_both_nan(a, b, what)
    assert np.array_equal(np.isnan(a), np.isnan(b)), what + ": NaN positions differ"


def check_shape(sk, cs, shape, coop, dense, cells, what, select=0):
    nested = int(cs.name == "nested")
    want = dict(solver="ordered", nested=nested, dense=int(dense == "1" and not nested), select=select, workgroups=(cells + 15) // 16)
    assert {k: shape[k] for k in want} == want, (what, shape)
    if coop == "1" and cs.window and not nested:
        assert shape["coop_launches"] == sk.info["n_ik_rounds_16_lanes"] > 0 and shape["segments"] > 1, (what, shape, sk.info)
    else:
        assert shape["coop_launches"] == 0 and shape["segments"] == 1, (what, shape)


FORMS = [("1", "0"), ("0", "0"), ("1", "1"), ("0", "1")]          # (MMDX_IK_COOP, MMDX_SOLVE_DENSE); the first is the default


@pytest.mark.gpu
@pytest.mark.parametrize("name", ALL_RIGS)
def test_gpu_every_form_equals_the_oracle_and_the_others(monkeypatch, oracle, name):
    """ik_coop_kernel (the default), one lane per solve on the LDS window, and both under the forced dense ordered kernel -- for the
    rigs off the window the same four settings all run ccd() on the HBM state; the nested rig reports nested = 1 and is never dense."""
    cs = ix.case(name, oracle)
    sk = vmd.Skeleton(*cs.rig)
    default = sk.solve(cs.poses)                                  # no environment at all
    assert_oracle(default, cs, range(ix.NI), f"{name}, default")
    check_shape(sk, cs, sk.last_solve_shape(), "1", "0", ix.NI, f"{name}, default")
    for ni in ix.NIS:
        results = []
        for coop, dense in FORMS:
            what = f"{name}, {COOP}={coop}, {DENSE}={dense}, {ni} instances"
            monkeypatch.setenv(COOP, coop)
            monkeypatch.setenv(DENSE, dense)
            got = sk.solve(cs.poses[:ni])
            check_shape(sk, cs, sk.last_solve_shape(), coop, dense, ni, what)
            assert_oracle(got, cs, range(ni), what)
            results.append(got)
        for got, form in zip(results[1:], FORMS[1:]):
            assert_same(got, results[0], f"{name}, {ni} instances: {form} vs {FORMS[0]}")
        assert_same(results[0], default[:ni], f"{name}, {ni} instances: the first rows of the full crowd")
    sk.close()


@pytest.mark.gpu
@pytest.mark.parametrize("coop,dense", FORMS)
@pytest.mark.parametrize("name", ["line1", "line3", "line6", "links7", "nested"])
def test_gpu_select_permuted_list_with_an_id_that_is_no_row(monkeypatch, oracle, name, coop, dense):
    """mmdx_skeleton_solve_select on the plain and the dense ordered kernel, with ik_coop_select_kernel and without: the whole list
    (97 cells: the last workgroup's only listed cell is no row), then its first 37 (a partly empty workgroup; the other rows keep
    their pattern and their poses hold NaN), then the whole list with one more id that is no row in the middle of a wave."""
    cs = ix.case(name, oracle)
    sk = vmd.Skeleton(*cs.rig)
    monkeypatch.setenv(COOP, coop)
    monkeypatch.setenv(DENSE, dense)
    whole = ix.select_ids()
    middle = whole.copy()
    middle[24] = ix.NI + 5                                        # cell 24: the second workgroup, the third group of four of its wave
    for ids, count in ((whole, whole.size), (whole, 37), (middle, middle.size)):
        what = f"{name}, select {count}{' with a dead cell in the middle' if ids is middle else ''}, {COOP}={coop}, {DENSE}={dense}"
        rows = sel.listed_rows(ids, count, ix.NI)
        assert rows.sum() == min(count, ix.NI) - (ids is middle)
        got = sel.run(sk, sel.nan_unlisted(cs.poses, rows), ids, count)
        check_shape(sk, cs, sk.last_solve_shape(), coop, dense, ids.size, what, select=1)
        assert_oracle(got[rows], cs, np.flatnonzero(rows), what)
        assert (got[~rows].view(np.uint8) == sel.PATTERN).all(), what + ": a row that is not listed was written"
    sk.close()


@pytest.mark.gpu
@pytest.mark.parametrize("coop", ["1", "0"])
@pytest.mark.parametrize("name", ["line3", "line6", "append"])
def test_gpu_physics_seam_without_overrides(monkeypatch, oracle, name, coop):
    """mmdx_skeleton_solve_pre then mmdx_skeleton_solve_post with an empty override list: the plain solve's palettes."""
    cs = ix.case(name, oracle)
    sk = vmd.Skeleton(*cs.rig, physics_seam=True)
    monkeypatch.setenv(COOP, coop)
    for ni in ix.NIS:
        sk.solve_pre(cs.poses[:ni])
        check_shape(sk, cs, sk.last_solve_shape(), coop, "0", ni, f"{name}, pre, {ni}")
        got = sk.solve_post(np.zeros(0, np.int32), np.zeros(0, np.uint8), np.zeros((ni, 0, 16), np.float32))
        assert_oracle(got, cs, range(ni), f"{name}, pre + post, {COOP}={coop}, {ni} instances")
    sk.close()


@pytest.mark.gpu
def test_gpu_motion_to_palette_in_one_call(oracle):
    """mmdx_skeleton_solve_motion on line3: a motion with one key per posed bone and instance, at frame = instance, so that the
    evaluated poses ARE the steered poses (a key hit returns the key verbatim) -- asserted -- and the palettes the oracle's."""
    cs = ix.case("line3", oracle)
    nb = cs.rig[0].shape[0]
    names = [f"b{b}" for b in range(nb)]
    rest_pose = np.float32([0, 0, 0, 0, 0, 0, 0, 1])
    posed = [b for b in range(nb) if (gu.bits(cs.poses[:, b]) != gu.bits(rest_pose)).any()]
    keys = [(names[b], i, tuple(cs.poses[i, b, 0:3].tolist()), tuple(cs.poses[i, b, 4:8].tolist()), None) for b in posed for i in range(ix.NI)]
    bm = vmd.Vmd(vmd.write_vmd(keys, [])).bind_bones(names)
    sk = vmd.Skeleton(*cs.rig)
    for ni in ix.NIS:
        frames = np.arange(ni, dtype=np.uint32)
        gu.assert_bits_equal(bm.eval(frames), cs.poses[:ni], f"the evaluated poses, {ni} instances")
        assert_oracle(sk.solve_motion(bm, frames), cs, range(ni), f"solve_motion, {ni} instances")
    back = np.arange(ix.NI, dtype=np.uint32)[::-1].copy()
    assert_oracle(sk.solve_motion(bm, back), cs, back, "solve_motion, the frames in reverse")
    sk.close()

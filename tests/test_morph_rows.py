"""Every walk over the morph gather table at row lengths around its own pipeline depth.

Seven software-pipelined loops in csrc/kernels.hip walk the sliced-ELL table, each with its depth and its tail arithmetic:
W1 for_row<F16,16> (morph_apply_kernel), W2 row_prefetch / row_consume<F16, 8 | 16> in deform_kernel with shared rates gathered
in the kernel, W3 the same pair in frame_kernel, W4 walk_head + walk_from_head (per-instance rates, 512 threads, file order: the
head is requested again between the packs), W5 the rolling window without a head (256 threads), W6 for_row<F16,4> (tile order) and
W7 pack_kernel's inline walk.  A refill loop runs only when a slice is longer than the depth, a second refill needs twice the
depth, and the tails have one case per residue of the length -- while the models of the other small-shape tests have slices of
0 to 7 entries (9 in one).  tests/morph_rows.py builds models whose slice lengths are chosen: 0..9, 15, 16, 17, 31, 32, 33 and 67.

CPU: the realised slice lengths (restated from mmdx_model_get_vertex_order) contain every required length, every slice is ragged,
the plan's entry counts agree; the oracle equals libmmd on these long rows (where oracle/_ref is built); the planner
(tests/launch_shape_driver.cpp) gives every GPU case the kernel, threads and group it claims, per-instance cases two packs and
more per workgroup.
GPU: every walk on the f32 and on the f16 table, bit for bit against the oracle with the launch shape read back after the call;
select + bounds, 32-byte vertices, non-finite offsets (the predicated walk over long rows, several packs), 640 slots (the next
pack's weights through the strided restaging loop) and fast math within the header's tolerance."""
import collections

import numpy as np
import pytest

from oracle.pyoracle import Reference, reference_available
from simple_mmd_renderer_amd import _capi as api
from simple_mmd_renderer_amd import synth
from simple_mmd_renderer_amd.engine import DeformModel, device_count
from tests import golden_util as gu
from tests import morph_rows as mr
from tests.test_crowd_groups import (FUSED1, FUSED4, NONE, SHARED, Expect, Row, crowd_env, planner, poisoned, positions,  # noqa: F401
                                     run, verify, within_fast_math_tolerance)

SOA, V32, POS16 = api.OUT_SOA, api.OUT_VERTEX32, api.OUT_SOA_POS16
OVERRIDES = ("MMDX_GROUP", "MMDX_THREADS", "MMDX_SHARED_FUSED", "MMDX_INTERLEAVE", "MMDX_SELECT_INTERLEAVE", "MMDX_STORE_WT",
             "MMDX_LDS_TARGET", "MMDX_FUSED_PACK", "MMDX_FRAME_KERNEL", "MMDX_FRAME_THREADS", "MMDX_MORPH_AUTOSKIP", "MMDX_STAGGER")
FAST_A = 0.007            # offset scale of the fast-math ladder: test_fast_math_walks_within_the_header_tolerance
FAST_XMAX = 34.0

# ---- the case table -----------------------------------------------------------------------------------------------------------------
# model: "ladder" | "nonfinite" | "many" | "fast"; env: the MMDX_* overrides of the call (all others unset); kernel / threads /
# group / morph: what the call must launch (validated against the planner on the CPU, read back from the library on the GPU).
Case = collections.namedtuple("Case", "name walk model f16 layout ni shared env kernel threads group morph tile sel_bounds")


def _case(name, walk, model, f16, layout, ni, shared, env, kernel, threads, group, morph, tile=False, sel_bounds=False):
    return Case(name, walk, model, f16, layout, ni, shared, {"MMDX_" + k: v for k, v in env.items()}, kernel, threads, group, morph,
                tile, sel_bounds)


W4_ENV, W5_ENV, W7_ENV = dict(GROUP=16), dict(GROUP=8, THREADS=256), dict(GROUP=8, FUSED_PACK=1)


def _per_instance(model, tag, f16, layout, walks="4567"):
    """W4: 19 instances in workgroups of 16 and 3 = two full packs of 8, then a partial one.  W5 / W7: 11 instances in workgroups
    of 8 and 3 = two packs of 4, then a partial one.  W6: both shapes on a tile-order model.  (pack_kernel deals quads
    interleaved: its first workgroup serves instances 0-3 and 8-10, the second 4-7.)"""
    out = []
    if "4" in walks:
        out.append(_case(f"W4-{tag}", "W4", model, f16, layout, 19, False, W4_ENV, "deform", 512, 16, FUSED4))
    if "5" in walks:
        out.append(_case(f"W5-{tag}", "W5", model, f16, layout, 11, False, W5_ENV, "deform", 256, 8, FUSED4))
    if "6" in walks:
        out.append(_case(f"W6-512-{tag}", "W6", model, f16, layout, 19, False, W4_ENV, "deform", 512, 16, FUSED4, tile=True))
        out.append(_case(f"W6-256-{tag}", "W6", model, f16, layout, 11, False, W5_ENV, "deform", 256, 8, FUSED4, tile=True))
    if "7" in walks:
        out.append(_case(f"W7-{tag}", "W7", model, f16, layout, 11, False, W7_ENV, "pack", 512, 8, FUSED4))
    return out


def _cases():
    cases = []
    for tag, f16, layout in (("f32", False, SOA), ("f16", True, POS16)):
        c = lambda name, walk, ni, env, kernel, threads, morph: _case(f"{name}-{tag}", walk, "ladder", f16, layout, ni, True, env,  # noqa: E731
                                                                     kernel, threads, 1, morph)
        cases += [
            c("W1-pass-9", "W1", 9, {}, "deform", 256, SHARED),
            c("W1-pass-3", "W1", 3, dict(SHARED_FUSED=0), "deform", 256, SHARED),
            c("W2-3-256", "W2", 3, dict(THREADS=256), "deform", 256, FUSED1),
            c("W2-3-512", "W2", 3, dict(THREADS=512), "deform", 512, FUSED1),
            c("W2-9-256", "W2", 9, dict(SHARED_FUSED=2, THREADS=256), "deform", 256, FUSED1),
            c("W2-9-512", "W2", 9, dict(SHARED_FUSED=2, THREADS=512), "deform", 512, FUSED1),
            c("W3-frame-128", "W3", 1, dict(FRAME_KERNEL=2, FRAME_THREADS=128), "frame", 128, FUSED1),
            c("W3-frame-256", "W3", 1, dict(FRAME_KERNEL=2, FRAME_THREADS=256), "frame", 256, FUSED1),
            c("W2-one-frame-512", "W2", 1, dict(FRAME_KERNEL=0), "deform", 512, FUSED1),
            c("W2-one-frame-256", "W2", 1, dict(FRAME_KERNEL=0, THREADS=256), "deform", 256, FUSED1)]
        cases += _per_instance("ladder", tag, f16, layout)
        cases += _per_instance("nonfinite", "nonfinite-" + tag, f16, layout)
        cases += _per_instance("many", "many-slots-" + tag, f16, layout, walks="457")
    # 32-byte vertices.  The pack kernel has the two-array layouts only: with MMDX_FUSED_PACK=1 a 32-byte-vertex call takes
    # deform_kernel<512> at the forced group -- the second row pins that.
    cases.append(_case("W4-vertex32", "W4", "ladder", False, V32, 19, False, W4_ENV, "deform", 512, 16, FUSED4))
    cases.append(_case("W7-vertex32-takes-W4", "W4", "ladder", False, V32, 11, False, W7_ENV, "deform", 512, 8, FUSED4))
    # select + bounds, one per walk that has the flavours (blocked, so that list position = workgroup * group + g)
    blocked = dict(INTERLEAVE=0, SELECT_INTERLEAVE=0)
    cases.append(_case("W2-select-bounds", "W2", "ladder", False, SOA, 9, True, dict(blocked, SHARED_FUSED=2, THREADS=256, GROUP=4),
                       "deform", 256, 4, FUSED1, sel_bounds=True))
    for cs in _per_instance("ladder", "select-bounds", False, SOA, walks="456"):
        if cs.name != "W6-512-select-bounds":
            cases.append(cs._replace(sel_bounds=True))
    # fast math: SoA, rows of up to 33 entries
    cases += [_case("W1-fast", "W1", "fast", False, SOA, 9, True, {}, "deform", 256, 1, SHARED),
              _case("W2-fast", "W2", "fast", False, SOA, 3, True, dict(THREADS=256), "deform", 256, 1, FUSED1)]
    cases += [cs for cs in _per_instance("fast", "fast", False, SOA, walks="456") if cs.name != "W6-256-fast"]
    return cases


CASES = _cases()
EXACT = [c for c in CASES if c.model != "fast"]
FAST = [c for c in CASES if c.model == "fast"]
BAD_POS = 5             # list position of the id >= ni of a select case: inside the first workgroup's (W2: the second's) instances


def pack_of(case):
    return 8 if (case.kernel, case.threads) == ("deform", 512) else 4


def flat_model(kind, f16):
    if kind == "ladder":
        return mr.ladder()
    if kind == "nonfinite":
        return mr.with_nonfinite_offsets(mr.ladder(), f16)
    if kind == "many":
        return mr.many_slots()
    return mr.ladder(mr.LADDER33, offset_scale=FAST_A)


def case_inputs(case, m, frame):
    """(palettes [ni, NB, 16], rates [ni | 1, NM]) of a case; `frame` varies the shared rates between the cases of one model."""
    pals = synth.make_palettes(m, np.arange(case.ni) * 3 + 1)
    skipped = mr.BAD_MORPHS if case.model == "nonfinite" else ()
    floor = 0.5 if case.model == "fast" else 0.05
    if case.shared:
        return pals, mr.shared_rates(m.nm, frame, floor, skipped)[None, :]
    return pals, mr.instance_rates(m.nm, case.ni, pack_of(case), floor, skipped)


def select_ids(case):
    """The device list of a select case: all instances but three in a seeded random order, one id >= ni at BAD_POS; behind the
    count the three unlisted ids.  Returns (ids, count, listed)."""
    perm = np.random.default_rng(900 + case.ni).permutation(case.ni)
    live = [int(i) for i in perm[:case.ni - 3]]
    live.insert(BAD_POS, case.ni + 5)
    return np.array(live + [int(i) for i in perm[case.ni - 3:]], np.uint32), len(live), sorted(live[:BAD_POS] + live[BAD_POS + 1:])


# ---- CPU: coverage -------------------------------------------------------------------------------------------------------------------
VARIANTS = [("ladder", False), ("ladder", True), ("nonfinite", False), ("nonfinite", True), ("fast", False)]


@pytest.mark.parametrize("tile", [False, True], ids=["file-order", "tile-order"])
@pytest.mark.parametrize("kind,f16", VARIANTS, ids=[f"{k}-{'f16' if h else 'f32'}" for k, h in VARIANTS])
def test_ladder_realises_every_required_slice_length(hip_lib, kind, f16, tile):
    """The slice lengths restated from mmdx_model_get_vertex_order and the per-vertex entry counts: every length of
    mr.REQUIRED occurs (and one >= 65, except in the fast-math ladder, whose rows end at 33), every slice of length L >= 2 has
    a lane with exactly L entries and a lane with fewer, 64 x the sum of the lengths is the plan's padded entry count and the
    plan's entry count is the model's."""
    m = flat_model(kind, f16)
    cnt, slots = mr.entry_counts(m)
    assert np.array_equal(cnt, m.meta["counts"]) and slots == mr.NM
    with DeformModel(m, host_only=True, f16_positions=f16, tile_order=tile) as dm:
        rows = mr.slice_rows(dm.vertex_order()[0], cnt)
        lengths = mr.slice_lengths(dm.vertex_order()[0], cnt)
        assert dm.info.n_tiles == 5 and len(lengths) == 40 and dm.nv == mr.NV and dm.nv % mr.TILE == 3
        assert set(mr.REQUIRED) <= set(lengths), sorted(set(mr.REQUIRED) - set(lengths))
        assert (max(lengths) >= mr.LONG) == (kind != "fast") and (kind != "fast" or max(lengths) == 33)
        for length, r in zip(lengths, rows):
            if length >= 2:
                assert (r == length).any() and (r < length).any(), (length, r)
        assert 64 * sum(lengths) == dm.info.n_entries_padded
        assert dm.info.n_entries == cnt.sum() and dm.info.n_slots == slots
        # three one-class tiles in the order they were asked for, then the mixed tile
        want = [x for _, t in (mr.LADDER33 if kind == "fast" else mr.LADDER) for x in t]
        assert lengths[:24] == want
        skin = dm.get_skin()[0]
        assert [len(set(skin[t * mr.TILE:(t + 1) * mr.TILE])) for t in range(4)] == [1, 1, 1, 3]
    assert np.signbit(m.positions[m.positions == 0]).sum() >= 6          # the -0.0 components


def test_many_slots_model(hip_lib):
    m = mr.many_slots()
    cnt, slots = mr.entry_counts(m)
    for f16 in (False, True):
        with DeformModel(m, host_only=True, f16_positions=f16) as dm:
            lengths = mr.slice_lengths(dm.vertex_order()[0], cnt)
            assert dm.info.n_slots == slots >= 600 and dm.info.n_entries == cnt.sum()
            assert 64 * sum(lengths) == dm.info.n_entries_padded and 0 < max(lengths) <= 16
    # restaged through the strided loop: more float4 weights per pack than threads, in all three kernels
    assert slots + 1 > 512


def test_inputs_of_the_cases():
    """Per-instance rates: every instance its own, consecutive packs differ in every slot, the first pack wholly below the skip
    with all three kinds, later packs apply (nearly) everything; the non-finite morphs are skipped in every instance."""
    for case in CASES:
        if case.shared:
            continue
        pack = pack_of(case)
        assert case.name == "W7-vertex32-takes-W4" or (case.group >= 2 * pack and case.ni > case.group and (case.ni - case.group) % pack not in (0, 4))
        m = flat_model(case.model, case.f16)
        _, r = case_inputs(case, m, 0)
        assert r.shape == (case.ni, m.nm) and len({x.tobytes() for x in r}) == case.ni
        assert (r[:pack] < 1e-7).all() and {(r[:pack] < 0).any(), (r[:pack] == 0).any(), (r[:pack] == np.float32(5e-8)).any()} == {True}
        for i in range(case.ni - pack):
            assert (r[i] != r[i + pack]).all()
        assert ((r[pack:] >= 1e-7).mean(axis=1) > 0.9).all()
        if case.model == "nonfinite":
            assert (r[:, list(mr.BAD_MORPHS)] < 1e-7).all()
            assert (~np.isfinite(m.morph_value)).sum() == 2 and ((m.morph_value == 70000.0).sum() == 1) == case.f16
        if case.model == "fast":
            assert ((r < 1e-7) | (r >= 0.5)).all()


# ---- CPU: the oracle on long rows ----------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not reference_available(), reason="oracle/_ref/libmmd_ref.so not built")
@pytest.mark.parametrize("kind", ["ladder", "nonfinite", "many"])
def test_oracle_equals_libmmd_on_long_rows(oracle, kind):
    """oracle.morph + oracle.skin against the real libmmd on rows of up to 67 entries (the other fixtures pin the oracle on rows
    as short as the kernels' own): rates of a shared case, of three instances of a per-instance case and rates around the 1e-7
    skip (the two binary32 neighbours of 1e-7, 5e-8, 0, negative)."""
    m = flat_model(kind, False)
    skipped = mr.BAD_MORPHS if kind == "nonfinite" else ()
    edge = mr.shared_rates(m.nm, 5, 0.05, skipped)
    e = np.float32(1e-7)
    edge[np.arange(7) * 9 % m.nm + 1] = (e, np.nextafter(e, np.float32(0)), np.nextafter(e, np.float32(1)), 5e-8, 0.0, -1e-7, 1.0)
    edge[list(skipped)] = 0.0
    per = mr.instance_rates(m.nm, 19, 8, 0.05, skipped)
    ref = Reference(m)
    skin = oracle.normalize(m)
    try:
        for k, rates in enumerate((mr.shared_rates(m.nm, 0, 0.05, skipped), edge, per[0], per[9], per[18])):
            pal = synth.make_palettes(m, [3 * k + 1])[0]
            rp, rn, _ = ref.run(rates, pal)
            op, on = oracle.skin(m, pal, oracle.morph(m, rates), skin)
            assert np.isfinite(op).all() and np.isfinite(on).all()
            gu.assert_bits_equal(op, rp, f"{kind} rates {k}: pos")
            gu.assert_bits_equal(on, rn, f"{kind} rates {k}: nrm")
    finally:
        ref.close()


# ---- CPU: the planner ----------------------------------------------------------------------------------------------------------------
def morph_mode(ns, shared, ni, shared_fused):
    """plan_morph_pass (csrc/launch_shape.cpp) for a call that promises nothing about its rates; ns <= 8192."""
    if not ns:
        return NONE
    if not (shared or ni == 1):
        return FUSED4
    return FUSED1 if ni == 1 or shared_fused == 2 or (shared_fused == 1 and ni <= 8) else SHARED


def test_planner_gives_every_case_its_shape(hip_lib, planner):
    """Every GPU case through tests/launch_shape_driver.cpp: the claimed kernel, threads (the frame kernel's come from
    MMDX_FRAME_THREADS, past the planner) and group; the morph mode from plan_morph_pass restated; per-instance cases at least
    two packs per workgroup."""
    scalars = {}
    calls = []
    for case in CASES:
        key = (case.model, case.f16, case.tile)
        if key not in scalars:
            with DeformModel(flat_model(case.model, case.f16), host_only=True, f16_positions=case.f16, tile_order=case.tile) as dm:
                scalars[key] = dict(f16=case.f16, tile_order=case.tile, ntiles=dm.info.n_tiles, max_tile_bones=dm.info.max_tile_bones,
                                    ns=dm.info.n_slots)
        env = case.env
        assert case.morph == morph_mode(scalars[key]["ns"], case.shared, case.ni, env.get("MMDX_SHARED_FUSED", 1)), case.name
        nwork = len(select_ids(case)[0]) if case.sel_bounds else case.ni
        calls.append(dict(scalars[key], layout=case.layout, ni=case.ni, nwork=nwork, morph=case.morph, bounds=case.sel_bounds,
                          select=case.sel_bounds, threads=env.get("MMDX_THREADS", 0), group=env.get("MMDX_GROUP", 0),
                          fused_pack=env.get("MMDX_FUSED_PACK", 0), frame_kernel=env.get("MMDX_FRAME_KERNEL", 1)))
    for case, s in zip(CASES, planner(calls)):
        assert "error" not in s, (case.name, s)
        assert api.DEBUG_KERNELS[s["kernel"]] == case.kernel, (case.name, s)
        if case.kernel != "frame":
            assert (s["threads"] if case.kernel == "deform" else 512, s["group"]) == (case.threads, case.group), (case.name, s)
        if case.morph == FUSED4 and case.name != "W7-vertex32-takes-W4":
            assert s["group"] >= 2 * pack_of(case), (case.name, s)
    # every walk on both tables; the non-finite and the many-slots variants on both tables too
    for f16 in (False, True):
        assert {c.walk for c in CASES if c.model == "ladder" and c.f16 == f16 and not c.sel_bounds} == {f"W{k}" for k in range(1, 8)}
        assert {c.walk for c in CASES if c.model == "nonfinite" and c.f16 == f16} == {"W4", "W5", "W6", "W7"}
        assert {c.walk for c in CASES if c.model == "many" and c.f16 == f16} == {"W4", "W5", "W7"}
    assert {c.walk for c in CASES if c.sel_bounds} == {"W2", "W4", "W5", "W6"}
    assert {c.walk for c in FAST} == {"W1", "W2", "W4", "W5", "W6"}


# ---- GPU -----------------------------------------------------------------------------------------------------------------------------
class Bench:
    """Handles and oracle expectations, made once per module."""

    def __init__(self, oracle):
        self.oracle, self.flat, self.dm, self.exp, self.calls = oracle, {}, {}, {}, 0

    def get(self, case):
        fkey = (case.model, case.f16 and case.model == "nonfinite")
        if fkey not in self.flat:
            self.flat[fkey] = flat_model(*fkey)
        key = fkey + (case.f16, case.tile)
        if key not in self.dm:
            self.dm[key] = DeformModel(self.flat[fkey], f16_positions=case.f16, tile_order=case.tile, fast_math=case.model == "fast")
            with np.errstate(over="ignore"):             # (70000.0 -> binary16 inf in the quantised copy, on purpose)
                self.exp[key] = Expect(self.oracle, self.flat[fkey], self.dm[key].vertex_order()[0] if case.tile else None)
        return self.dm[key], self.exp[key]

    def close(self):
        for dm in self.dm.values():
            dm.close()


@pytest.fixture(scope="module")
def bench(hip_lib, oracle):
    assert device_count() >= 1, "no HIP device visible: the GPU tests must run on the MI355X box"
    b = Bench(oracle)
    yield b
    b.close()


def launch(bench, crowd_env, case):
    """One call of the case with device-resident operands into sentinel-filled arrays; the launch shape read back and compared;
    returns what verify() / within_fast_math_tolerance() take."""
    dm, exp = bench.get(case)
    bench.calls += 1
    pals, rates = case_inputs(case, exp.m, 10 + bench.calls)
    crowd_env(**dict(dict.fromkeys(OVERRIDES), **case.env))
    row = Row(case.name, dm.nv, case.ni, case.group, case.threads, case.morph, case.tile, False, 0, 0)
    scale = 0.1 if case.layout == V32 else 1.0
    ids = listed = None
    gp, gr = pals, rates
    if case.sel_bounds:
        ids, count, listed = select_ids(case)
        row = row._replace(n_ids=len(ids), count=count)
        gp, gr = poisoned(pals, rates, case.shared, listed)
    walked = dm.morph_pass_stats()[0]
    out = run(dm, row, case.layout, gp, gr, case.shared, 0, scale, case.sel_bounds, ids=ids)
    s = dm.last_launch_shape()
    tiles = case.kernel != "frame"
    want = dict(kernel=case.kernel, threads=case.threads, group=case.group, morph=case.morph, layout=case.layout, f16=int(case.f16),
                tile_order=int(case.tile), bounds=int(case.sel_bounds), select=int(case.sel_bounds), write_through=0,
                ngroups=((len(ids) if case.sel_bounds else case.ni) + case.group - 1) // case.group if tiles else 0)
    assert {k: s[k] for k in want} == want, (case.name, s)
    # the shared pass really walked the table (it skips the walk when it finds the rates of its last run)
    assert dm.morph_pass_stats()[0] - walked == (1 if case.morph == SHARED else 0), case.name
    return dm, exp, row, out, pals, rates, scale, listed


@pytest.mark.gpu
@pytest.mark.parametrize("case", EXACT, ids=[c.name for c in EXACT])
def test_walk_bit_exact_against_the_oracle(bench, crowd_env, case):
    """One case of the table: every instance, both arrays, byte for byte the oracle's (the f16 layout: the oracle on inputs that
    went through binary16 once, its positions rounded to binary16; tile order: remapped through vertex_order()); select cases:
    bounds equal to min / max of the oracle's positions, unlisted instances and their bounds rows keep the fill pattern; the
    sentinel bytes behind the outputs are intact; the oracle's results are finite (the non-finite offsets are never applied)."""
    dm, exp, row, out, pals, rates, scale, listed = launch(bench, crowd_env, case)
    verify(exp, out, row, case.layout, dm.nv, 0, pals, rates, case.shared, scale, listed, case.name)
    for i in (range(case.ni) if listed is None else listed):
        a, b = exp.rows(case.layout, rates[0] if case.shared else rates[i], pals[i], scale)
        assert np.isfinite(positions(a, case.layout, dm.nv)).all() and (b is None or np.isfinite(b.view(np.float32)).all())


@pytest.mark.gpu
@pytest.mark.parametrize("case", FAST, ids=[c.name for c in FAST])
def test_fast_math_walks_within_the_header_tolerance(bench, crowd_env, case):
    """The contracted code object (kernels_fast.hip) on a ladder with rows of up to n = 33 entries, against include/mmdx.h's
    MMDX_CREATE_FAST_MATH tolerance (tests/test_fast_math.py: 1e-5 (1 + |x_ref|) per position component, 2e-6 per normal
    component).  The inputs are chosen so that the check can neither fail by rounding alone nor hide a dropped or doubled entry:
    offsets of magnitude a/2 .. a per component, a = FAST_A = 0.007, rates skipped or >= 0.5.
      upper bound on a: a contracted and an uncontracted row sum differ by at most n^2 a 2^-23 = 1089 a 2^-23, to stay under
        a tenth of the smallest position tolerance (1e-6): a <= 7.70e-3.  The rest of the tolerance is the skinning's.
      lower bound on a: one dropped or doubled entry moves a component by at least a/4 = 1.75e-3, to stay at or above five
        times the largest tolerance 1e-5 (1 + |x|) over the coordinate range: |x| <= 34 (asserted on the oracle's positions;
        they reach about 24), i.e. a >= 7.0e-3 at the edge of that range, 5.0e-3 at |x| = 24."""
    assert 33 ** 2 * FAST_A * 2.0 ** -23 <= 0.1 * 1e-5 and FAST_A / 4 >= 5 * 1e-5 * (1 + FAST_XMAX)
    dm, exp, row, out, pals, rates, scale, _ = launch(bench, crowd_env, case)
    off = np.abs(exp.m.morph_value)
    assert off.min() >= np.float32(FAST_A / 2) and off.max() <= np.float32(FAST_A)
    for i in range(case.ni):
        a, _ = exp.rows(case.layout, rates[0] if case.shared else rates[i], pals[i], scale)
        assert np.abs(positions(a, case.layout, dm.nv)).max() <= FAST_XMAX
    assert (out[0][-64:] == 0xFF).all() and (out[1][-64:] == 0xFF).all()
    if case.tile:
        # within_fast_math_tolerance reads instance i at i * nv rows: the arrays are dense
        assert out[0].size == case.ni * dm.nv * 12 + 64
    within_fast_math_tolerance(out, exp, row, case.layout, dm.nv, pals, rates, case.shared, scale)

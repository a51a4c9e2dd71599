"""The ordered bone solver's two-workgroups-per-CU compilation (DENSE: __launch_bounds__(256, 2), 256 VGPRs, spills) at small crowds.

On its own the launcher takes that compilation only above 16 instances per CU -- thousands of instances -- so every form of the
solve except one 44-bone rig used to run on the plain compilation alone.  MMDX_SOLVE_DENSE (read per call) forces it, and
mmdx_debug_last_solve_shape (Skeleton.last_solve_shape) proves after every call which compilation ran, with how many workgroups,
in how many ordered-segment launches and with how many ik_coop launches.

Every GPU case solves once under MMDX_SOLVE_DENSE=1 and once under =0 and asserts: the shape says dense = 1, then dense = 0, with
ceil(cells / 16) workgroups; the two results are bit-identical; the forced-dense result is the oracle's, bit for bit except where
both are NaN (a degenerate chain divides 0 by 0 upstream too).  So that "both NaN" cannot hide a failure, fewer than a quarter of
a case's instances may hold a NaN anywhere in the oracle's palette (the condition of test_gpu_full_size_crowd_rig) -- asserted in
every case; the seeds below were chosen on the CPU with the oracle alone.  Instance counts 1, 17 and 40: sixteen instances per
workgroup, so one partly empty workgroup, two, and three with the last one half empty.  The oracle's palettes are computed once
per rig for 40 instances and shared, never written; the smaller counts take the first rows of the same poses.

CPU: the decision itself (csrc/solve_shape.hpp plan_solve_dense), swept by tests/solve_shape_driver.cpp under ASan + UBSan."""
import os

import numpy as np
import pytest

from simple_mmd_renderer_amd import _capi as api
from simple_mmd_renderer_amd import synth, vmd
from simple_mmd_renderer_amd.engine import DeviceBuffer
from tests import golden_util as gu
from tests import host_program as hp
from tests import test_solve_select as sel
from tests.host_program import ROOT
from tests.test_physics_seam import physics_case, random_transforms
from tests.test_rig import NESTED_CASES, long_chain_rig, many_long_chains_rig, random_poses

DENSE, COOP = "MMDX_SOLVE_DENSE", "MMDX_IK_COOP"
NIS = (1, 17, 40)
NI_MAX = max(NIS)
LDS_BOUND = 80 * 1024 - 1024          # solve_shape.hpp: 2 * (lds + 1024) <= 160 KB


@pytest.fixture(autouse=True)
def _lib(hip_lib):
    return hip_lib


# ---- CPU: the decision ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def driver():
    return hp.build("solve_shape_driver", [os.path.join(hp.TESTS, "solve_shape_driver.cpp")], opt="-O1", sanitize=True)


def test_decision_sweep_under_sanitizers(driver):
    r = hp.run(driver, ["sweep"])
    assert r.returncode == 0, r.stdout + r.stderr
    counts = dict(kv.split("=") for kv in r.stdout.split())
    assert int(counts["failures"]) == 0 and "ERROR" not in r.stderr
    assert int(counts["rows"]) == 2 * 11 * 4 * 8 * 5


def test_decision_nested_lds_bound_crowd_size_and_env(driver):
    """The cases of the decision by name, against this file's own statement of the rule: nested rigs are never dense under any env
    value; the LDS bound on both sides; wgs == cus and wgs == cus + 1; env -1, 0 and 1."""
    cus = 256
    cases, want = [], []
    for env in (-1, 0, 1):
        for lds in (0, LDS_BOUND, LDS_BOUND + 1):
            for wgs in (1, cus, cus + 1, 100000):
                cases.append((1, lds, wgs, cus, env)); want.append(0)                       # nested
                fits = 2 * (lds + 1024) <= 160 * 1024
                cases.append((0, lds, wgs, cus, env))
                want.append(int(fits and (env == 1 or (env == -1 and wgs > cus))))
    r = hp.run(driver, ["eval"], stdin="".join("%d %d %d %d %d\n" % c for c in cases))
    assert r.returncode == 0, r.stdout + r.stderr
    got = [int(x) for x in r.stdout.split()]
    assert len(got) == len(cases)
    assert got == want, [c for c, g, w in zip(cases, got, want) if g != w]
    # and spelled out: what each env value does to a small crowd, the crowd-size rule at its boundary, the bound at its boundary
    table = dict(zip(cases, got))
    assert table[(0, 0, 1, cus, 1)] == 1 and table[(0, 0, 1, cus, 0)] == 0 and table[(0, 0, 1, cus, -1)] == 0
    assert table[(0, 0, cus, cus, -1)] == 0 and table[(0, 0, cus + 1, cus, -1)] == 1 and table[(0, 0, cus + 1, cus, 0)] == 0
    assert table[(0, LDS_BOUND, 1, cus, 1)] == 1 and table[(0, LDS_BOUND + 1, 1, cus, 1)] == 0
    assert table[(1, 0, cus + 1, cus, 1)] == 0 and table[(1, 0, cus + 1, cus, -1)] == 0


def test_binding_declares_the_solve_shape():
    assert hasattr(api.lib(), "mmdx_debug_last_solve_shape") and "mmdx_debug_last_solve_shape" in api.SIGNATURES
    import ctypes as C
    assert C.sizeof(api.DebugSolveShape) == 10 * 4
    text = open(os.path.join(ROOT, "include", "mmdx_bench.h")).read()
    body = text[text.index("typedef struct mmdx_debug_solve_shape {"):text.index("} mmdx_debug_solve_shape;")]
    assert body.count("uint32_t") == 10 and body.index("struct_size") < body.index("solver")
    assert "mmdx_debug_last_solve_shape" not in open(os.path.join(ROOT, "include", "mmdx.h")).read()
    # host state only: a skeleton that never solved says so, without a device
    rest, parent, level, flags = synth.make_skeleton(3, 1)
    sk = vmd.Skeleton(rest, parent, level, flags)
    shape = sk.last_solve_shape()
    assert shape["solver"] == "none" and not any(v for k, v in shape.items() if k != "solver")
    bad = api.DebugSolveShape()
    bad.struct_size = 36
    assert api.lib().mmdx_debug_last_solve_shape(sk.h, C.byref(bad)) == 1
    sk.close()


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------------
def wgs_of(cells):
    return (cells + 15) // 16


def dense_then_plain(monkeypatch, sk, solve, cells, nested=0, select=0, what=""):
    """solve() under MMDX_SOLVE_DENSE=1, then under =0: the shape after each (dense = 1 then 0 -- a nested rig 0 both times --, the
    workgroup count, the form), identical bits.  Returns the forced-dense result and its shape."""
    out = []
    for env in ("1", "0"):
        monkeypatch.setenv(DENSE, env)
        res = solve()
        shape = sk.last_solve_shape()
        want = dict(solver="ordered", nested=nested, dense=int(env == "1" and not nested), select=select, workgroups=wgs_of(cells))
        assert {k: shape[k] for k in want} == want, (what, env, shape)
        assert shape["lds"] <= LDS_BOUND or nested, (what, shape)          # (else =1 could not have been dense)
        out.append((res, shape))
    monkeypatch.delenv(DENSE)
    assert {k: v for k, v in out[0][1].items() if k != "dense"} == {k: v for k, v in out[1][1].items() if k != "dense"}, what
    gu.assert_bits_equal(out[0][0], out[1][0], what + ": forced dense vs plain")
    return out[0]


def assert_oracle(got, want, what):
    """got == the oracle's rows, NaN only where both are; fewer than a quarter of the instances have a NaN in the oracle's palette."""
    ni = got.shape[0]
    n_nan = int(np.isnan(want[:ni]).any(axis=(1, 2)).sum())
    assert 4 * n_nan < ni, f"{what}: {n_nan} of {ni} oracle palettes hold a NaN: 'both NaN' would hide too much, pick another seed"
    for i in range(ni):
        gu.assert_bits_equal_or_both_nan(got[i], want[i], f"{what}: palette of instance {i}")


def chain_poses(nb, ik_bones, seed):
    """Rest pose everywhere, the IK bones displaced (test_gpu_long_ik_chains)."""
    rng = np.random.RandomState(seed)
    poses = np.zeros((NI_MAX, nb, 8), np.float32)
    poses[..., 7] = 1
    poses[:, ik_bones, 0:3] = rng.uniform(-1, 1, (NI_MAX, len(ik_bones), 3))
    return poses


def _levels(seed, n_ik, n_app):
    return lambda: (synth.make_ik_rig(300, seed, n_ik=n_ik, n_append=n_app, post_physics=0.3, levels=3), random_poses(NI_MAX, 300, 700 + seed))


def _chain(n_links):
    def make():
        rest, parent, flags, ik = long_chain_rig(n_links)
        return (rest, parent, None, flags, None, None, ik), chain_poses(200, [199], n_links)
    return make


def _many_chains():
    rest, parent, flags, ik = many_long_chains_rig()
    return (rest, parent, None, flags, None, None, ik), chain_poses(rest.shape[0], np.flatnonzero(flags == 0x20), 5)


# name -> (rig and poses [40], the rig has IK chains that run on an LDS window, environment the SKELETON is created under)
RIGS = {
    "levels11": (_levels(11, 16, 20), True, {}),               # test_gpu_dense_rigs_with_levels_and_post_physics
    "levels12": (_levels(12, 4, 40), True, {}),
    "levels13": (_levels(13, 24, 0), True, {}),
    "chain6": (_chain(6), True, {}),                            # test_gpu_long_ik_chains: the longest chain of the LDS window ...
    "chain7": (_chain(7), False, {}),                           # ... and the shortest on the HBM state
    "chain12": (_chain(12), False, {}),
    "many_chains": (_many_chains, True, {}),                    # test_gpu_many_long_chains_share_a_round
    "ik300": (lambda: (synth.make_ik_rig(300, 7, n_ik=8, n_append=12), random_poses(NI_MAX, 300, 207)), True, {}),
    "sequential": (lambda: (synth.make_ik_rig(150, 3, n_ik=6, n_append=10), random_poses(NI_MAX, 150, 203)), True,
                   {"MMDX_SOLVE_SEQUENTIAL": "1"}),            # one event per round
}
_cache = {}


def rig_case(oracle, name):
    """(rig, poses [40], the oracle's palettes [40]) of a RIGS row: computed once, shared, never written."""
    if name not in _cache:
        rig, poses = RIGS[name][0]()
        want = np.stack([oracle.bone_solve_full(rig[0], rig[1], poses[i], *rig[2:]) for i in range(NI_MAX)])
        for a in (poses, want):
            a.setflags(write=False)
        _cache[name] = (rig, poses, want)
    return _cache[name]


@pytest.mark.parametrize("name", sorted(RIGS))
def test_oracle_palettes_of_the_cases_are_mostly_finite(oracle, name):
    """The seed choice, checked where it was made: on the CPU, with the oracle alone, for every instance count the GPU cases use."""
    _, _, want = rig_case(oracle, name)
    for ni in NIS:
        assert 4 * int(np.isnan(want[:ni]).any(axis=(1, 2)).sum()) < ni, (name, ni)


@pytest.mark.gpu
@pytest.mark.parametrize("coop", ["0", "1"])
@pytest.mark.parametrize("name", sorted(RIGS))
def test_gpu_forced_dense_equals_plain_and_oracle(monkeypatch, oracle, name, coop):
    """Levels and post-physics bones, chains on both sides of the LDS-window / HBM-state boundary, many chains in one round, the
    300-bone rig, one event per round -- each with one lane per solve inside the ordered kernel (MMDX_IK_COOP=0: no ik_coop launch,
    one ordered segment: the dense compilation's own ccd() runs) and with ik_coop_kernel (=1: on a rig with window chains some
    ik_coop launches, and the dense compilation runs the segments around them)."""
    _, windows, create_env = RIGS[name]
    rig, poses, want = rig_case(oracle, name)
    for k, v in create_env.items():
        monkeypatch.setenv(k, v)
    sk = vmd.Skeleton(*rig)
    for k in create_env:
        monkeypatch.delenv(k)
    if create_env:
        assert sk.info["n_solve_rounds"] == sk.nb
    monkeypatch.setenv(COOP, coop)
    for ni in NIS:
        what = f"{name}, MMDX_IK_COOP={coop}, {ni} instances"
        got, shape = dense_then_plain(monkeypatch, sk, lambda: sk.solve(poses[:ni]), ni, what=what)
        if coop == "0":
            assert shape["coop_launches"] == 0 and shape["segments"] == 1, (what, shape)
        else:
            assert shape["coop_launches"] == sk.info["n_ik_rounds_16_lanes"], (what, shape, sk.info)
            if windows:
                assert shape["coop_launches"] > 0 and shape["segments"] > 1, (what, shape)
            else:
                assert shape["coop_launches"] == 0 and shape["segments"] == 1, (what, shape)
        assert_oracle(got, want, what)
    sk.close()


MORPH_CASES = [(44, 1, 3, 4), (150, 2, 6, 8)]                     # of test_gpu_bone_morphs_vs_oracle


def morph_case(oracle, nb, seed, n_ik, n_app):
    key = ("morph", nb, seed)
    if key not in _cache:
        rig = synth.make_ik_rig(nb, seed, n_ik=n_ik, n_append=n_app)
        morphs = synth.make_bone_morphs(nb, 90 + seed)
        poses = random_poses(NI_MAX, nb, 500 + seed)
        rates = np.random.RandomState(seed).choice([0, 5e-8, 0.3, 1.0, 1.7, -0.5], (NI_MAX, morphs["type"].size)).astype(np.float32)
        per = np.stack([oracle.bone_solve_full(rig[0], rig[1], poses[i], *rig[2:], morphs, rates[i]) for i in range(NI_MAX)])
        shared = np.stack([oracle.bone_solve_full(rig[0], rig[1], poses[i], *rig[2:], morphs, rates[3]) for i in range(NI_MAX)])
        plain = np.stack([oracle.bone_solve_full(rig[0], rig[1], poses[i], *rig[2:]) for i in range(NI_MAX)])
        for a in (poses, rates, per, shared, plain):
            a.setflags(write=False)
        _cache[key] = (rig, morphs, poses, rates, per, shared, plain)
    return _cache[key]


@pytest.mark.parametrize("nb,seed,n_ik,n_app", MORPH_CASES)
def test_oracle_morphed_palettes_are_mostly_finite_and_moved(oracle, nb, seed, n_ik, n_app):
    _, _, _, _, per, shared, plain = morph_case(oracle, nb, seed, n_ik, n_app)
    for ni in NIS:
        for want in (per, shared):
            assert 4 * int(np.isnan(want[:ni]).any(axis=(1, 2)).sum()) < ni, (nb, ni)
    assert not np.array_equal(gu.bits(per[0]), gu.bits(plain[0])) and not np.array_equal(gu.bits(shared[0]), gu.bits(plain[0]))


@pytest.mark.gpu
@pytest.mark.parametrize("nb,seed,n_ik,n_app", MORPH_CASES)
def test_gpu_forced_dense_bone_morphs(monkeypatch, oracle, nb, seed, n_ik, n_app):
    """mmdx_skeleton_solve_morphed with per-instance rates and with shared rates (the 5e-8 skip among them)."""
    rig, morphs, poses, rates, per, shared, _ = morph_case(oracle, nb, seed, n_ik, n_app)
    sk = vmd.Skeleton(*rig, morphs)
    assert sk.info["n_bone_morph_entries"] > 0
    for ni in NIS:
        what = f"{nb} bones, {ni} instances"
        got, _ = dense_then_plain(monkeypatch, sk, lambda: sk.solve(poses[:ni], morph_weights=rates[:ni]), ni, what=what + ", own rates")
        assert_oracle(got, per, what + ", own rates")
        got, _ = dense_then_plain(monkeypatch, sk, lambda: sk.solve(poses[:ni], morph_weights=rates[3]), ni, what=what + ", shared rates")
        assert_oracle(got, shared, what + ", shared rates")
    sk.close()


SEAM = (150, 3, 6, 8)                                            # of test_gpu_physics_seam_vs_oracle: IK, append and post-physics bones


def seam_case(oracle):
    if "seam" not in _cache:
        nb, seed, n_ik, n_app = SEAM
        rig, over, strict, rng = physics_case(nb, seed, n_ik, n_app)
        poses = random_poses(NI_MAX, nb, 500 + seed)
        xf = random_transforms(rng, NI_MAX, over.size)
        want = np.stack([oracle.bone_solve_physics(rig[0], rig[1], poses[i], over, strict, xf[i], *rig[2:])[0] for i in range(NI_MAX)])
        for a in (poses, xf, want):
            a.setflags(write=False)
        _cache["seam"] = (rig, over, strict, poses, xf, want)
    return _cache["seam"]


def test_oracle_seam_palettes_are_finite_and_the_overrides_are_of_both_kinds(oracle):
    rig, over, strict, _, _, want = seam_case(oracle)
    assert 0 < strict.sum() < strict.size                          # strict (Fix) and non-strict (Synchronize only) overrides
    assert (rig[3] & 0x1000).any()                                 # post-physics bones
    for ni in NIS:
        assert 4 * int(np.isnan(want[:ni]).any(axis=(1, 2)).sum()) < ni, ni


@pytest.mark.gpu
@pytest.mark.parametrize("coop", ["0", "1"])
def test_gpu_forced_dense_physics_seam(monkeypatch, oracle, coop):
    """mmdx_skeleton_solve_pre, the reactor's writes (strict and non-strict), mmdx_skeleton_solve_post -- the sequence of
    test_physics_seam.py: both steps report dense, the palettes are those of the same sequence on the oracle."""
    rig, over, strict, poses, xf, want = seam_case(oracle)
    sk = vmd.Skeleton(*rig, physics_seam=True)
    assert sk.info["n_post_physics"] > 0
    monkeypatch.setenv(COOP, coop)
    for ni in NIS:
        what = f"seam, MMDX_IK_COOP={coop}, {ni} instances"
        steps = []

        def both_steps():
            sk.solve_pre(poses[:ni])
            steps.append(sk.last_solve_shape())
            return sk.solve_post(over, strict, xf[:ni])
        got, post = dense_then_plain(monkeypatch, sk, both_steps, ni, what=what)
        pre_dense, pre_plain = steps
        assert pre_dense["solver"] == "ordered" and pre_dense["dense"] == 1 and pre_dense["workgroups"] == wgs_of(ni), (what, pre_dense)
        assert pre_plain["dense"] == 0 and pre_plain["workgroups"] == wgs_of(ni), (what, pre_plain)
        if coop == "0":
            assert pre_dense["coop_launches"] == post["coop_launches"] == 0 and pre_dense["segments"] == post["segments"] == 1
        else:
            assert pre_dense["coop_launches"] + post["coop_launches"] == sk.info["n_ik_rounds_16_lanes"] > 0, (what, pre_dense, post)
        assert_oracle(got, want, what)
    sk.close()


@pytest.mark.gpu
@pytest.mark.parametrize("coop", ["0", "1"])
def test_gpu_forced_dense_select(monkeypatch, oracle, coop):
    """mmdx_skeleton_solve_select on 70 rows: a device list of capacity 48 (three workgroups of state cells), a device-side count of
    37 (the third workgroup: five live cells), an id that is no row in the middle of the second workgroup.  The listed rows equal
    the plain forced-dense call and the oracle, every other palette row keeps its 0xA5 pattern, the shape says select = 1,
    dense = 1; the poses of rows that are not listed hold NaN."""
    monkeypatch.setenv(COOP, coop)
    ni, cap, count = sel.NI, 48, 37
    rig = sel.RIGS["ik44"]()
    sk = vmd.Skeleton(*rig)
    poses = random_poses(ni, sk.nb, 1300 + sk.nb)
    ids = np.random.RandomState(48).permutation(ni)[:cap].astype(np.uint32)
    ids[24] = ni + 5                                              # cell 24: workgroup 1, lane group 8 of 16
    rows = sel.listed_rows(ids, count, ni)
    assert rows.sum() == count - 1 and not rows[ids[count:]].any()
    plain, _ = dense_then_plain(monkeypatch, sk, lambda: sk.solve(poses), ni, what="plain call on 70")
    got, shape = dense_then_plain(monkeypatch, sk, lambda: sel.run(sk, sel.nan_unlisted(poses, rows), ids, count), cap, select=1,
                                  what=f"select, MMDX_IK_COOP={coop}")
    assert (shape["coop_launches"] > 0 and shape["segments"] > 1) if coop == "1" else (shape["coop_launches"] == 0 and shape["segments"] == 1)
    sel.check(got, plain, rows, "37 of a capacity of 48")
    want = np.stack([oracle.bone_solve_full(rig[0], rig[1], poses[i], *rig[2:]) for i in np.flatnonzero(rows)])
    assert_oracle(got[rows], want, "listed rows")
    sk.close()


@pytest.mark.gpu
def test_gpu_forced_dense_solve_motion_on_an_ik_rig(monkeypatch, oracle):
    """mmdx_skeleton_solve_motion on the rig of test_gpu_solve_motion_on_an_ik_rig_takes_the_ordered_solver: forced dense it equals
    eval then solve, host and device operands, and the oracle on the evaluated poses."""
    nb = 48
    rig = synth.make_ik_rig(nb, 77, n_ik=3, n_append=4)
    names = [f"b{i}" for i in range(nb)]
    v = vmd.Vmd(vmd.write_vmd(synth.make_bone_keys(names, 9, keys_per=4, span=100), []))
    bm, sk = v.bind_bones(names), vmd.Skeleton(*rig)
    all_frames = ((np.arange(NI_MAX) * 7) % 110).astype(np.uint32)
    poses = bm.eval(all_frames)
    want = np.stack([oracle.bone_solve_full(rig[0], rig[1], poses[i], *rig[2:]) for i in range(NI_MAX)])
    for ni in NIS:
        frames = all_frames[:ni]
        one, _ = dense_then_plain(monkeypatch, sk, lambda: sk.solve_motion(bm, frames), ni, what=f"solve_motion, {ni}")
        two, _ = dense_then_plain(monkeypatch, sk, lambda: sk.solve(bm.eval(frames)), ni, what=f"eval then solve, {ni}")
        gu.assert_bits_equal(one, two, f"solve_motion vs eval then solve, {ni} instances")
        assert_oracle(one, want, f"solve_motion, {ni} instances")
        d_fr, d_pal = DeviceBuffer.from_numpy(frames), DeviceBuffer(ni * nb * 64)

        def on_device():
            d_pal.memset(0xFF)
            sk.solve_motion_device(bm, ni, d_fr.ptr, d_pal.ptr)
            api.check(api.lib().mmdx_device_synchronize())
            return d_pal.download((ni, nb, 16), np.float32)
        dev, _ = dense_then_plain(monkeypatch, sk, on_device, ni, what=f"solve_motion, device operands, {ni}")
        gu.assert_bits_equal(dev, one, f"device operands, {ni} instances")
        d_fr.free(); d_pal.free()
    sk.close()


@pytest.mark.gpu
@pytest.mark.parametrize("coop", ["0", "1"])
def test_gpu_nested_rig_is_never_dense(monkeypatch, oracle, coop):
    """Nested IK has no dense compilation: under MMDX_SOLVE_DENSE=1 the shape says nested = 1, dense = 0 (and no ik_coop launch under
    either MMDX_IK_COOP), and the palettes are the oracle's."""
    nb, seed = NESTED_CASES[1]
    rig = synth.make_nested_ik_rig(nb, seed)
    poses = random_poses(NI_MAX, nb, 950 + seed)
    want = np.stack([oracle.bone_solve_full(rig[0], rig[1], poses[i], *rig[2:]) for i in range(NI_MAX)])
    sk = vmd.Skeleton(*rig)
    monkeypatch.setenv(COOP, coop)
    for ni in NIS:
        got, shape = dense_then_plain(monkeypatch, sk, lambda: sk.solve(poses[:ni]), ni, nested=1, what=f"nested, {ni} instances")
        assert shape["nested"] == 1 and shape["dense"] == 0 and shape["coop_launches"] == 0 and shape["segments"] == 1, shape
        assert_oracle(got, want, f"nested, {ni} instances")
    sk.close()


@pytest.mark.gpu
def test_gpu_parallel_fk_solve_says_so(monkeypatch):
    """A rig without append bones and IK: the record says that the ordered solver did not run, whatever MMDX_SOLVE_DENSE holds."""
    rest, parent, level, flags = synth.make_skeleton(40, 2, 5, 0.25, 3)
    sk = vmd.Skeleton(rest, parent, level, flags)
    monkeypatch.setenv(DENSE, "1")
    sk.solve(random_poses(17, 40, 3))
    shape = sk.last_solve_shape()
    assert shape["solver"] == "parallel_fk" and not any(v for k, v in shape.items() if k != "solver"), shape
    sk.close()

"""Root motion on the GPU: mmdx_animator_root_motion and mmdx_bone_motion_in_place (include/mmdx.h).

The kernel is held, bit for bit and with no tolerance anywhere, by the golden rows of the real libmmd
(tests/golden/root_motion_expect.npz) and by the numpy restatement tests/root_motion_ref.py fed R values from the existing, pinned
MotionSet.eval_bones_time; tests/test_root_motion_cpu.py holds the restatement and the host build of csrc/root_math.hpp to the same
rows without a GPU.
"""
import numpy as np
import pytest

from simple_mmd_renderer_amd import _capi as api
from simple_mmd_renderer_amd import synth, vmd
from simple_mmd_renderer_amd.engine import DeformModel, DeviceBuffer
from tests import animator_ref as ar
from tests import golden_util as gu
from tests import root_motion_ref as rm
from tests import test_animator as ta
from tests import test_root_motion_cpu as cpu

F = np.float32
NONE = rm.NONE
ALL_AXES = api.ROOT_X | api.ROOT_Y | api.ROOT_Z
STATE = ("clips_a", "clips_b", "times_a", "times_b", "weights", "speed", "fade_rate")


@pytest.fixture(autouse=True)
def _lib(hip_lib):
    return hip_lib


_close = ta.close_all


def poke(an, **arrays):
    """Write animator arrays through their device addresses: what an adopter's own kernel may leave there -- clip ids outside the
    bank, NaN clocks -- and mmdx_animator_set_state would refuse."""
    addr = an.device_arrays()
    types = dict(ar.ARRAYS)
    for k, v in arrays.items():
        a = np.ascontiguousarray(v, types[k])
        raw = DeviceBuffer.adopt(addr[k], a.nbytes)
        raw.upload(a)
        raw.ptr = None


def headings(n, seed):
    """Placements f32 [n, 8]: identity, unit and unnormalised headings by turns, a fourth float that is not 0."""
    rng = np.random.RandomState(seed)
    q = rng.normal(size=(n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    q[0::3] = (0, 0, 0, 1)
    q[2::3] *= rng.uniform(0.4, 1.7, (q[2::3].shape[0], 1))
    return np.concatenate([rng.uniform(-20, 20, (n, 3)), rng.uniform(-1, 1, (n, 1)), q], 1).astype(F)


def r_from_set(ms, root_bone, pl):
    """R at the instants of a plan, from the pinned evaluator: the translation of `root_bone` in the rows of eval_bones_time."""
    n = pl["clips"].shape[0]
    clips = np.where(pl["sampled"], pl["clips"][:, :, None], NONE).astype(np.uint32)
    rows = ms.eval_bones_time(clips.reshape(-1), pl["times"].reshape(-1))
    return rows[:, root_bone, :3].reshape(n, 2, 4, 3)


# ---------------------------------------------------------------------------------------- golden rows ----
@pytest.mark.gpu
@pytest.mark.parametrize("device_dt", [False, True], ids=["host_dt", "device_dt"])
def test_gpu_golden_rows_through_the_kernel(device_dt):
    """Every row of the fixture is an instance; one call per (dt, axes) pair of the fixture, each on a fresh copy of the
    placements: the rows of that pair equal libmmd's, all others are whatever their own pair gives and are not looked at."""
    z = rm.fixture()
    n = z["dt"].size
    ms = rm.root_bank()
    an = vmd.Animator(ms, n, [tuple(r) for r in rm.CLIP_ROWS])
    assert [r[0] for r in an.clip_table()] == rm.table()["length"].tolist()
    an.set_state(**{k: z[k] for k in STATE if not k.startswith("clips")})
    poke(an, clips_a=z["clips_a"], clips_b=z["clips_b"])                     # ids out of range among them
    before = an.get_state()
    d_place, d_dt = DeviceBuffer(n * 32), DeviceBuffer(8)
    seen = 0
    nan_rows = np.isnan(z["dt"])
    for dt in np.unique(z["dt"][~nan_rows]).tolist() + [float("nan")]:
        with_dt = nan_rows if dt != dt else z["dt"] == dt
        for axes in np.unique(z["axes"][with_dt]).tolist():
            rows = with_dt & (z["axes"] == axes)
            d_place.upload(z["placements"])
            if device_dt:
                d_dt.upload(np.array([dt], np.float64))
                an.root_motion(ms, 0, axes, d_place.ptr, dt_ptr=d_dt.ptr)
            elif dt != dt:
                with pytest.raises(api.MmdxError, match="dt is NaN"):
                    an.root_motion(ms, 0, axes, d_place.ptr, dt=dt)
            else:
                an.root_motion(ms, 0, axes, d_place.ptr, dt=dt)
            got = d_place.download((n, 8), F)
            gu.assert_bits_equal_or_both_nan(got[rows, :3], z["expect"][rows], f"dt {dt}, axes {axes}")
            gu.assert_bits_equal(got[:, 3:], z["placements"][:, 3:], f"dt {dt}, axes {axes}: the fourth float and the heading")
            seen += int(rows.sum())
    assert seen == n
    ar.assert_states_equal(an.get_state(), before, "the animator's arrays after every call")
    _close(an, ms, d_place, d_dt)


# ---------------------------------------------------------------------------------------- the sweep ----
def sweep_with_a_walker(ni):
    """animator_ref.sweep(ni, 60).  From 8 instances on the scenario sets its corners by hand, and instance 2 of them plays the
    looping clip 0, whose root has keys: it moves and, in the step of 7 s, crosses the seam.  Below 8 there are no corners and
    what plays is the seed's; there instance 0 is made that walker, so that the small sizes move and fold too."""
    table, state, dts, requests = ar.sweep(ni, 60)
    if ni < 8:
        state["clips_a"][0], state["times_a"][0], state["speed"][0] = 0, 1.9, 1.0
        state["clips_b"][0], state["times_b"][0], state["weights"][0], state["fade_rate"][0] = NONE, 0.0, 0.0, 0.0
    return table, state, dts, requests


def test_sweep_folds_at_every_size():
    """Without a GPU: the scenario of every size crosses a loop seam with a side that is read (the fold needs no R)."""
    for ni in (1, 7, 8, 9, 63, 64, 65, 257):
        table, state, dts, requests = sweep_with_a_walker(ni)
        states, _ = ar.run_reference(table, state, dts, requests)
        folds = sum(int(rm.plan(cur, table, dt)["folded"].any(1).sum()) for cur, dt in zip([state] + states[:-1], dts))
        assert folds >= 1, ni
@pytest.mark.gpu
@pytest.mark.parametrize("ni", [1, 7, 8, 9, 63, 64, 65, 257])
def test_gpu_sweep_equals_the_restatement(ni):
    """60 steps of `root motion -> request -> advance` on the scenario of the animator's tests: the placements after every step
    against the restatement (R from eval_bones_time), the eleven arrays against animator_ref."""
    table, state, dts, requests = sweep_with_a_walker(ni)
    want_states, events = ar.run_reference(table, state, dts, requests)
    ms = ta.scenario_set(["b0", "b1", "b2"])
    root_bone = 1 if ni == 65 else 0
    an = vmd.Animator(ms, ni, ta.rows_for_create())
    an.set_state(**state)
    place = headings(ni, 40 + ni)
    d_place = DeviceBuffer.from_numpy(place)
    cur = state
    seen = {}
    for k, (dt, req) in enumerate(zip(dts, requests)):
        axes = (ALL_AXES, api.ROOT_X | api.ROOT_Z, ALL_AXES, api.ROOT_Y)[k % 4]
        pl = rm.plan(cur, table, dt)
        place, ev = rm.apply(cur, table, dt, r_from_set(ms, root_bone, pl), axes, place)
        for name, hit in ev.items():
            seen[name] = seen.get(name, 0) + int(hit.sum())
        an.root_motion(ms, root_bone, axes, d_place.ptr, dt=dt)
        if req[0].size:
            an.request(*req)
        an.advance(dt)
        gu.assert_bits_equal(d_place.download((ni, 8), F), place, f"NI {ni}, step {k} (dt {dt}): placements")
        ar.assert_states_equal(an.get_state(), want_states[k], f"NI {ni}, step {k} (dt {dt})")
        cur = want_states[k]
    assert not np.isnan(place).any()
    # every size, the ones around the 8-lane group included: somebody moved, and somebody crossed a loop seam
    assert seen["moved"] >= 3 and seen["fold_forwards"] + seen["fold_backwards"] >= 1, (ni, seen)
    if ni >= 63:
        for name in ("fold_forwards", "fold_backwards", "fold_while_fading", "mix", "row_a", "moved"):
            assert seen[name] >= 3, (name, seen)
        n = {name: ta.count_events(events, name) for name in ("promote", "at_once", "request_waits", "then_none")}
        assert min(n.values()) >= 3, n                                       # a promotion, a switch at once, a request in a fade, THEN -> rest
    _close(an, ms, d_place)


# ---------------------------------------------------------------------------------------- what is not read, what is not written ----
def poison_case():
    """16 instances mid-fade, all clocks close to a seam so that folds occur; the weights put rows on A, on B and in between."""
    n = 16
    s = ar.initial_state(n)
    s["clips_a"][:] = np.arange(n) % 2
    s["clips_b"][:] = (np.arange(n) + 1) % 2
    s["times_a"][:] = np.where(s["clips_a"] == 0, 1.49, 0.99)
    s["times_b"][:] = np.where(s["clips_b"] == 0, 1.2, 0.98)
    s["fade_rate"][:] = 3.0
    s["weights"][:] = np.array([0.0, 5e-8, -1.0, 0.0, 1.0, 2.0, 1 - 5e-8, 1.0, 0.25, 0.5, 0.75, 1e-7, 0.0, 1.0, 0.5, 0.3], F)
    return s


@pytest.mark.gpu
def test_gpu_a_side_the_weight_does_not_read_may_hold_anything():
    s = poison_case()
    n = s["loops"].size
    side = rm.mb.side_of(s["weights"])
    assert (side == 0).sum() >= 4 and (side == 1).sum() >= 4 and (side == 2).sum() >= 4
    ms = rm.root_bank()
    an = vmd.Animator(ms, n, [tuple(r) for r in rm.CLIP_ROWS])
    place = headings(n, 3)
    d_place = DeviceBuffer.from_numpy(place)
    an.set_state(**s)
    an.root_motion(ms, 0, ALL_AXES, d_place.ptr, dt=1 / 30)
    clean = d_place.download((n, 8), F)
    assert (clean[:, :3] != place[:, :3]).any(1).all()                       # everybody moved
    pl = rm.plan(s, rm.table(), 1 / 30)
    want, ev = rm.apply(s, rm.table(), 1 / 30, r_from_set(ms, 0, pl), ALL_AXES, place)
    gu.assert_bits_equal(clean, want, "the clean run")
    assert ev["fold_forwards"].sum() >= 8
    # side b of the rows on A, side a of the rows on B: an id far outside the bank and a NaN clock
    bad = dict(clips_a=np.where(side == 1, 0x7FFFFFF0, s["clips_a"]), clips_b=np.where(side == 0, 0x7FFFFFF0, s["clips_b"]),
               times_a=np.where(side == 1, np.nan, s["times_a"]), times_b=np.where(side == 0, np.nan, s["times_b"]))
    poke(an, **bad)
    d_place.upload(place)
    an.root_motion(ms, 0, ALL_AXES, d_place.ptr, dt=1 / 30)
    gu.assert_bits_equal(d_place.download((n, 8), F), clean, "with the unread sides poisoned")
    _close(an, ms, d_place)


@pytest.mark.gpu
def test_gpu_nothing_else_is_written_and_a_nan_device_dt_writes_nothing():
    ni = 65
    table, state, _, _ = ar.sweep(ni, 1)
    ms = ta.scenario_set(["b0", "b1", "b2"])
    an = vmd.Animator(ms, ni, ta.rows_for_create())
    an.set_state(**state)
    place = headings(ni, 9)
    guard = 16
    image = np.full(guard + ni * 8 + guard, -123.25, F)
    image[guard:guard + ni * 8] = place.reshape(-1)
    d = DeviceBuffer.from_numpy(image)
    d_dt = DeviceBuffer.from_numpy(np.array([np.nan], np.float64))
    an.root_motion(ms, 0, ALL_AXES, d.ptr + guard * 4, dt_ptr=d_dt.ptr)
    gu.assert_bits_equal(d.download(image.shape, F), image, "after a NaN step")
    d_dt.upload(np.array([1 / 30], np.float64))
    an.root_motion(ms, 0, ALL_AXES, d.ptr + guard * 4, dt_ptr=d_dt.ptr)
    got = d.download(image.shape, F)
    gu.assert_bits_equal(got[:guard], image[:guard], "the floats ahead of the array")
    gu.assert_bits_equal(got[-guard:], image[-guard:], "the floats behind the array")
    moved = got[guard:-guard].reshape(ni, 8)
    gu.assert_bits_equal(moved[:, 3:], place[:, 3:], "the fourth float and the quaternions")
    assert (moved[:, :3] != place[:, :3]).any(1).sum() >= 8            # (half the clips have no root keys, a quarter of the crowd stands)
    ar.assert_states_equal(an.get_state(), state, "the animator's arrays")
    # axes = 0: nothing moves, but +0 is still added (a -0 coordinate becomes +0, nothing else changes)
    d.upload(image)
    an.root_motion(ms, 0, 0, d.ptr + guard * 4, dt_ptr=d_dt.ptr)
    gu.assert_bits_equal(d.download(image.shape, F), image, "axes = 0")
    _close(an, ms, d, d_dt)


# ---------------------------------------------------------------------------------------- the dyadic walk ----
@pytest.mark.gpu
def test_gpu_dyadic_walk_across_two_seams():
    """Linear keys 0 -> 16 along Z over frames 0..64 in a loop of a stated 2.0 s, dt = 1/32: instance 0 heads a half turn about Y
    (an exact matrix: the closed form N * 0.234375 holds exactly), instance 1 the quarter turn, whose matrix is not exactly
    representable (tests/test_root_motion_cpu.py says why): there the restatement is the yardstick.  Animator.step issues both
    calls."""
    v = vmd.Vmd(vmd.write_vmd([("root", 0, (0.0, 0.0, 0.0), (0.0, 0.0, 0.0, 1.0), None),
                               ("root", 64, (0.0, 0.0, 16.0), (0.0, 0.0, 0.0, 1.0), None)], []))
    bm = v.bind_bones(["root"])
    ms = vmd.MotionSet([bm])
    an = vmd.Animator(ms, 2, [(cpu.DYADIC_LENGTH, vmd.ANIM_LOOP, NONE, 0.0)])
    an.request([0, 1], [0, 0])
    an.advance(0.0)                                                          # both start clip 0 at 0
    want = {h: cpu.dyadic_walk(h)[0] for h in ("half", "quarter")}
    # the restatement's R (tests/test_root_motion_cpu.dyadic_r) is the evaluator's, at every clock of the walk
    t = np.arange(0, 65) / 32.0
    gu.assert_bits_equal(ms.eval_bones_time(np.zeros(t.size, np.uint32), t)[:, 0, :3], cpu.dyadic_r(t), "R of the walk")
    d_place = DeviceBuffer.from_numpy(np.concatenate([cpu.dyadic_placement("half"), cpu.dyadic_placement("quarter")]))
    for k in range(cpu.DYADIC_STEPS):
        an.step(ms, 0, api.ROOT_Z, d_place.ptr, dt=cpu.DYADIC_DT)
        if k % 16 == 15 or k in (63, 64, 127, 128):
            got = d_place.download((2, 8), F)
            gu.assert_bits_equal(got[0, :3], want["half"][k], f"step {k}: the half turn")
            gu.assert_bits_equal(got[1, :3], want["quarter"][k], f"step {k}: the quarter turn")
    assert got[0, :3].tolist() == [0, 0, -cpu.DYADIC_STEPS * 0.234375]
    assert an.get_state(names=("loops",))["loops"].tolist() == [2, 2]
    _close(an, ms, bm, v, d_place)


# ---------------------------------------------------------------------------------------- in place ----
@pytest.mark.gpu
def test_gpu_in_place_rows_equal_the_source_except_the_masked_channels():
    names = rm.rig_small_names() + [rm.ROOT_NAME]
    root = len(names) - 1
    z = rm.fixture()
    times = np.unique(np.concatenate([z["times"].reshape(-1), np.arange(0, 48) / 30.0, [-1.0, 9.0]]))
    frames = np.arange(0, 50, dtype=np.uint32)
    for name in ("curved", "still", "no_root"):
        v = vmd.Vmd(rm.VMDS[name])
        bm = v.bind_bones(names)
        src_t, src_f = bm.eval_time(times), bm.eval(frames)                   # frame hits return the keys unchanged
        if name == "curved":
            assert (src_t[:, root, :3] != 0).any(0).all() and len({r.tobytes() for r in src_t[:, root, :3]}) > 40
        for axes in (ALL_AXES, api.ROOT_X | api.ROOT_Z, api.ROOT_Y, 0):
            ip = bm.in_place(root, axes)
            for what, got, src in (("times", ip.eval_time(times), src_t), ("frames", ip.eval(frames), src_f)):
                want = src.copy()
                for c in range(3):
                    if axes & (1 << c):
                        want[:, root, c] = 0.0
                gu.assert_bits_equal(got, want, f"{name}, axes {axes}, {what}")
            ip.close()
        _close(bm, v)


# ---------------------------------------------------------------------------------------- the C++ mirror ----
@pytest.mark.gpu
def test_cpp_root_motion_matches_python_path(tmp_path):
    """host/motion_example.cpp --crowd ends with a walking crowd: mmdx::MotionSet built in place, mmdx::Animator::Step with the
    moving set, the blend solve and PlacePalettes for 60 steps.  The same sequence from Python gives the same placements and placed
    palettes."""
    import subprocess
    from simple_mmd_renderer_amd import build, pmx
    nb = 40
    rig = synth.make_ik_rig(nb, 11, n_ik=3, n_append=4)
    m = synth.make_model(600, nb, 5, 60, seed=12)
    m.bone_pos, m.bone_parent = rig[0].copy(), rig[1].astype(m.bone_parent.dtype)
    bnames, mnames = ["骨%d" % b for b in range(nb)], ["表情%d" % k for k in range(m.nm)]
    (tmp_path / "m.pmx").write_bytes(pmx.write_pmx(m, pmx.PmxWriteOptions(rig=rig, bone_names=bnames, morph_names=mnames)))
    paths = []
    for k in range(3):
        p = tmp_path / ("c%d.vmd" % k)
        p.write_bytes(vmd.write_vmd(synth.make_bone_keys(bnames[:30 - k], 13 + k, keys_per=4, span=24), [(mnames[0], 0, 0.5), (mnames[0], 19, 1.0)]))
        paths.append(str(p))
    ni, hz = 37, 60.0
    exe = build.build_host_example(name="motion_example")
    r = subprocess.run([exe, "--crowd", str(ni), str(hz), str(tmp_path / "m.pmx")] + paths, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "walked checksum=" in r.stderr, r.stdout + r.stderr
    pm = pmx.load_pmx(str(tmp_path / "m.pmx"))
    vs = [vmd.Vmd(p) for p in paths]
    bms, mms = [v.bind_bones(pm.bone_names) for v in vs], [v.bind_morphs(pm.morph_names) for v in vs]
    still = [b.in_place(0, ALL_AXES) for b in bms]
    moving, in_place, sk = vmd.MotionSet(bms, mms), vmd.MotionSet(still, mms), pm.skeleton()
    ids = np.arange(ni, dtype=np.uint32)
    half = F(0.05) * ids.astype(F)
    where = np.zeros((ni, 8), F)
    where[:, 0], where[:, 5], where[:, 7] = F(12) * ids.astype(F), half, F(1) - half * half
    with DeformModel(m) as dm:
        an = vmd.Animator(in_place, ni)
        an.request(ids, ids % 3, model=dm)
        d_where, d_pal = DeviceBuffer.from_numpy(where), DeviceBuffer(ni * nb * 64)
        dev = api.PALETTE_ON_DEVICE | api.PLACE_ON_DEVICE | api.OUT_ON_DEVICE
        for _ in range(60):
            an.step(moving, 0, ALL_AXES, d_where.ptr, dt=1.0 / hz, model=dm)
            sk.solve_motion_set_blend_time_device(in_place, ni, *an.operand_ptrs(), d_pal.ptr, dm)
            dm.place_palettes(ni, d_pal.ptr, d_where.ptr, d_pal.ptr, dev)
        dm.sync()
        pal, walked = d_pal.download((ni, nb, 16), F), d_where.download((ni, 8), F)
        _close(an, d_where, d_pal)
    assert (walked[:, :3] != where[:, :3]).any(1).sum() >= ni // 3 and not np.isnan(pal).any()      # the first clip moves bone 0

    def fnv(a):
        h = 1469598103934665603
        for byte in np.ascontiguousarray(a).view(np.uint8).ravel().tolist():
            h = ((h ^ byte) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
        return h
    want = "walked checksum=%016x where=%016x" % (fnv(pal), fnv(walked))
    assert want in r.stderr, (want, r.stderr)
    _close(moving, in_place, sk, still, bms, mms, vs)


# ---------------------------------------------------------------------------------------- the recorded frame ----
@pytest.mark.gpu
def test_gpu_graph_of_root_motion_advance_solve_place_and_bounds():
    """{root motion, advance (one device dt), blend solve of the in-place set, place with the placements on the device, palette
    bounds} recorded once and replayed eight times with dt rewritten: placements, palettes and boxes equal the unrecorded sequence
    on a second animator.  Destroying the root set or the animator invalidates a graph that holds it."""
    m = synth.make_model(2048, 64, 8, 200, 112)
    names = [f"bone{i}" for i in range(m.nb)]
    ni = 9
    sk = vmd.Skeleton(m.bone_pos, np.asarray(m.bone_parent, np.int32))
    vs = [vmd.Vmd(d) for d in ta.scenario_vmds(names)]
    moving = [v.bind_bones(names) for v in vs]
    still = [b.in_place(0, ALL_AXES) for b in moving]
    roots = [v.bind_bones(names[:1]) for v in vs]
    in_place_set = vmd.MotionSet(still)
    new_root_set = lambda: vmd.MotionSet(roots)                              # noqa: E731
    root_set = new_root_set()
    assert in_place_set.clip_frames().tolist() == list(ar.CLIP_FRAMES)
    start = ar.initial_state(ni)
    start["clips_a"][:] = [0, 3, 5, NONE, 2, 6, 0, 4, 6]
    start["times_a"][:] = [1.9, 0.6, 0.7, 0.0, 1.4, 0.39, 0.1, 0.2, 0.0]
    start["speed"][:] = [1.0, 1.0, 0.5, 1.0, -1.0, 1.0, -1.0, 1.0, 2.0]
    start["clips_b"][:3] = [2, 0, 6]
    start["fade_rate"][:3] = 2.0
    start["weights"][:3] = [0.2, 0.5, 0.8]
    dts = [1 / 60, 1 / 30, 0.25, 1 / 144, 1 / 60, 0.5, -1 / 30, 1 / 60]
    place0 = headings(ni, 77)
    dev = api.PALETTE_ON_DEVICE | api.OUT_ON_DEVICE
    with DeformModel(m) as dm:
        eager, replayed = (vmd.Animator(in_place_set, ni, ta.rows_for_create()) for _ in range(2))
        d_dt = DeviceBuffer.from_numpy(np.array([0.0], np.float64))
        d_place, d_pal, d_box = DeviceBuffer(ni * 32), DeviceBuffer(ni * m.nb * 64), DeviceBuffer(ni * 24)

        def frame(an, rs):
            an.root_motion(rs, 0, ALL_AXES, d_place.ptr, dt_ptr=d_dt.ptr, model=dm)
            an.advance_device_dt(d_dt.ptr, dm)
            sk.solve_motion_set_blend_time_device(in_place_set, ni, *an.operand_ptrs(), d_pal.ptr, dm)
            dm.place_palettes(ni, d_pal.ptr, d_place.ptr, d_pal.ptr, dev | api.PLACE_ON_DEVICE)
            dm.palette_bounds_raw(ni, d_pal.ptr, d_box.ptr, dev)

        def results():
            dm.sync()
            return d_place.download((ni, 8), F), d_pal.download((ni, m.nb, 16), F), d_box.download((ni, 6), F)
        eager.set_state(dm, **start)
        d_place.upload(place0)
        want = []
        for dt in dts:
            d_dt.upload(np.array([dt], np.float64))
            frame(eager, root_set)
            want.append(results())
        assert len({w[0].tobytes() for w in want}) == len(dts) and not any(np.isnan(x).any() for w in want for x in w)
        assert (want[-1][0][:, :3] != place0[:, :3]).any(1).sum() >= ni - 2
        # the run before recording, as the header requires; then back to the start
        frame(replayed, root_set)
        dm.sync()
        replayed.set_state(dm, **start)
        d_place.upload(place0)
        dm.graph_begin()
        frame(replayed, root_set)
        g = dm.graph_end()
        gu.assert_bits_equal(d_place.download((ni, 8), F), place0, "recording does not run anything")
        for k, dt in enumerate(dts):
            d_dt.upload(np.array([dt], np.float64))
            d_pal.memset(0); d_box.memset(0)
            g.launch()
            for what, a, b in zip(("placements", "palettes", "boxes"), results(), want[k]):
                gu.assert_bits_equal(a, b, f"replay {k}: {what}")
        ar.assert_states_equal(replayed.get_state(dm), eager.get_state(dm), "the state after eight replays")
        root_set.close()                                                      # took part in the recording
        with pytest.raises(api.MmdxError, match="destroyed"):
            g.launch()
        g.close()
        # ... and so does the animator: a second recording of the two calls alone, with a fresh root set
        root_set = new_root_set()
        replayed.root_motion(root_set, 0, ALL_AXES, d_place.ptr, dt_ptr=d_dt.ptr, model=dm)
        dm.sync()
        dm.graph_begin()
        replayed.root_motion(root_set, 0, ALL_AXES, d_place.ptr, dt_ptr=d_dt.ptr, model=dm)
        replayed.advance_device_dt(d_dt.ptr, dm)
        g = dm.graph_end()
        g.launch()
        dm.sync()
        replayed.close()
        with pytest.raises(api.MmdxError, match="destroyed"):
            g.launch()
        g.close()
        _close(eager, d_dt, d_place, d_pal, d_box)
    _close(root_set, in_place_set, roots, still, moving, vs, sk)

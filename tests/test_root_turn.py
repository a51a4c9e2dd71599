"""Root motion that turns, on the GPU: mmdx_animator_root_motion_turn and mmdx_bone_motion_in_place_turn (include/mmdx.h).

The kernel is held, bit for bit and with no tolerance anywhere, by the golden rows of the real libmmd
(tests/golden/root_turn_expect.npz) and by the numpy restatement tests/root_turn_ref.py fed (T, Q) from the existing, pinned
MotionSet.eval_bones_time; tests/test_root_turn_cpu.py holds the restatement and the host build of csrc/root_math.hpp to the same
rows without a GPU, and the definition to its closed form.
"""
import numpy as np
import pytest

from simple_mmd_renderer_amd import _capi as api
from simple_mmd_renderer_amd import synth, vmd
from simple_mmd_renderer_amd.engine import DeformModel, DeviceBuffer
from tests import animator_ref as ar
from tests import golden_util as gu
from tests import root_motion_ref as rm
from tests import root_turn_ref as rt
from tests import test_animator as ta
from tests import test_root_motion as plain
from tests import test_root_turn_cpu as cpu

F = np.float32
NONE = rt.NONE
ALL_AXES = api.ROOT_X | api.ROOT_Y | api.ROOT_Z
STATE = plain.STATE
_close = ta.close_all
poke, headings = plain.poke, plain.headings


@pytest.fixture(autouse=True)
def _lib(hip_lib):
    return hip_lib


def tq_from_set(ms, root_bone, pl):
    """(T, Q) at the instants of a plan, from the pinned evaluator: the row of `root_bone` that eval_bones_time writes."""
    n = pl["clips"].shape[0]
    clips = np.where(pl["sampled"], pl["clips"][:, :, None], NONE).astype(np.uint32)
    rows = ms.eval_bones_time(clips.reshape(-1), pl["times"].reshape(-1))[:, root_bone]
    return rows[:, :3].reshape(n, 2, 4, 3), rows[:, 4:].reshape(n, 2, 4, 4)


# ---------------------------------------------------------------------------------------- golden rows ----
@pytest.mark.gpu
@pytest.mark.parametrize("device_dt", [False, True], ids=["host_dt", "device_dt"])
def test_gpu_golden_rows_through_the_kernel(device_dt):
    """Every row of the fixture is an instance; one call per (dt, axes, flags) triple of the fixture, each on a fresh copy of the
    placements: the rows of that triple equal libmmd's, all others are whatever their own triple gives and are not looked at.  The
    NaN-dt rows write nothing."""
    z = rt.fixture()
    n = z["dt"].size
    ms = rt.root_bank()
    an = vmd.Animator(ms, n, [tuple(r) for r in rt.CLIP_ROWS])
    assert [r[0] for r in an.clip_table()] == rt.table()["length"].tolist()
    an.set_state(**{k: z[k] for k in STATE if not k.startswith("clips")})
    poke(an, clips_a=z["clips_a"], clips_b=z["clips_b"])                     # ids out of range among them
    before = an.get_state()
    d_place, d_dt = DeviceBuffer(n * 32), DeviceBuffer(8)
    seen = 0
    nan_rows = np.isnan(z["dt"])
    for dt in np.unique(z["dt"][~nan_rows]).tolist() + [float("nan")]:
        with_dt = nan_rows if dt != dt else z["dt"] == dt
        for axes, flags in sorted({(int(a), int(f)) for a, f in zip(z["axes"][with_dt], z["flags"][with_dt])}):
            rows = with_dt & (z["axes"] == axes) & (z["flags"] == flags)
            normalize = flags == rt.ROOT_NORMALIZE
            d_place.upload(z["placements"])
            if device_dt:
                d_dt.upload(np.array([dt], np.float64))
                an.root_turn(ms, 0, axes, d_place.ptr, dt_ptr=d_dt.ptr, normalize=normalize)
            elif dt != dt:
                with pytest.raises(api.MmdxError, match="dt is NaN"):
                    an.root_turn(ms, 0, axes, d_place.ptr, dt=dt, normalize=normalize)
            else:
                an.root_turn(ms, 0, axes, d_place.ptr, dt=dt, normalize=normalize)
            got = d_place.download((n, 8), F)
            gu.assert_bits_equal_or_both_nan(got[rows][:, :3], z["expect"][rows][:, :3], f"dt {dt}, axes {axes}, flags {flags}: positions")
            gu.assert_bits_equal_or_both_nan(got[rows][:, 4:], z["expect"][rows][:, 4:], f"dt {dt}, axes {axes}, flags {flags}: headings")
            gu.assert_bits_equal(got[:, 3], z["placements"][:, 3], f"dt {dt}, axes {axes}, flags {flags}: the fourth float")
            if dt != dt:
                gu.assert_bits_equal(got, z["placements"], "a NaN dt writes nothing")
            seen += int(rows.sum())
    assert seen == n
    ar.assert_states_equal(an.get_state(), before, "the animator's arrays after every call")
    _close(an, ms, d_place, d_dt)


# ---------------------------------------------------------------------------------------- the sweep ----
@pytest.mark.gpu
@pytest.mark.parametrize("ni", [1, 7, 8, 9, 63, 64, 65, 257])
def test_gpu_sweep_equals_the_restatement(ni):
    """60 steps of `root turn -> request -> advance` on the scenario of the animator's tests, the flags and the axes rotating per
    step: the placements after every step against the restatement ((T, Q) from eval_bones_time), the eleven arrays against
    animator_ref.  There are guard floats around the array, and placements[i][3] keeps its bits."""
    table, state, dts, requests = plain.sweep_with_a_walker(ni)
    want_states, events = ar.run_reference(table, state, dts, requests)
    ms = ta.scenario_set(["b0", "b1", "b2"])
    root_bone = 1 if ni == 65 else 0
    an = vmd.Animator(ms, ni, ta.rows_for_create())
    an.set_state(**state)
    place = headings(ni, 140 + ni)
    fourth = place[:, 3].copy()
    guard = 16
    image = np.full(guard + ni * 8 + guard, -123.25, F)
    image[guard:guard + ni * 8] = place.reshape(-1)
    d = DeviceBuffer.from_numpy(image)
    ptr = d.ptr + guard * 4
    cur = state
    seen = {}
    for k, (dt, req) in enumerate(zip(dts, requests)):
        axes = (ALL_AXES, api.ROOT_X | api.ROOT_Z, ALL_AXES, api.ROOT_Y, 0)[k % 5]
        normalize = k % 3 != 1
        pl = rm.plan(cur, table, dt)
        t, q = tq_from_set(ms, root_bone, pl)
        place, ev = rt.apply(cur, table, dt, t, q, axes, normalize, place)
        for name, hit in ev.items():
            seen[name] = seen.get(name, 0) + int(hit.sum())
        an.root_turn(ms, root_bone, axes, ptr, dt=dt, normalize=normalize)
        if req[0].size:
            an.request(*req)
        an.advance(dt)
        got = d.download(image.shape, F)
        gu.assert_bits_equal(got[guard:-guard].reshape(ni, 8), place, f"NI {ni}, step {k} (dt {dt}): placements")
        gu.assert_bits_equal(got[:guard], image[:guard], f"NI {ni}, step {k}: the floats ahead of the array")
        gu.assert_bits_equal(got[-guard:], image[-guard:], f"NI {ni}, step {k}: the floats behind the array")
        ar.assert_states_equal(an.get_state(), want_states[k], f"NI {ni}, step {k} (dt {dt})")
        cur = want_states[k]
    assert not np.isnan(place).any()
    gu.assert_bits_equal(place[:, 3], fourth, "the fourth float")
    # every size, the ones around the 8-lane group included: somebody moved, turned, and crossed a loop seam
    folds = sum(seen[k] for k in ("fold_forwards_a", "fold_forwards_b", "fold_backwards_a", "fold_backwards_b"))
    assert seen["moved"] >= 3 and seen["turned"] >= 3 and folds >= 1, (ni, seen)
    if ni >= 63:
        for name in ("fold_forwards_a", "fold_backwards_a", "fold_while_fading", "mix", "row_a", "moved", "turned"):
            assert seen[name] >= 3, (name, seen)
    _close(an, ms, d)


# ---------------------------------------------------------------------------------------- what is not read ----
@pytest.mark.gpu
def test_gpu_a_side_the_weight_does_not_read_may_hold_anything():
    """Sides and instants that must not be read are poisoned with NaN clocks and out-of-range ids: nothing changes."""
    s = plain.poison_case()
    s["clips_a"][:] = np.where(np.arange(16) % 2 == 0, 0, rt.Q8)
    s["clips_b"][:] = np.where(np.arange(16) % 2 == 0, rt.Q8, 0)
    s["times_a"][:] = np.where(s["clips_a"] == 0, 1.49, 1.99)
    s["times_b"][:] = np.where(s["clips_b"] == 0, 1.2, 1.98)
    n = s["loops"].size
    side = rm.mb.side_of(s["weights"])
    assert (side == 0).sum() >= 4 and (side == 1).sum() >= 4 and (side == 2).sum() >= 4
    ms = rt.root_bank()
    an = vmd.Animator(ms, n, [tuple(r) for r in rt.CLIP_ROWS])
    place = headings(n, 3)
    d_place = DeviceBuffer.from_numpy(place)
    an.set_state(**s)
    an.root_turn(ms, 0, ALL_AXES, d_place.ptr, dt=1 / 30, normalize=True)
    clean = d_place.download((n, 8), F)
    assert (clean[:, :3] != place[:, :3]).any(1).all() and (clean[:, 4:] != place[:, 4:]).any(1).all()      # everybody moved and turned
    pl = rm.plan(s, rt.table(), 1 / 30)
    t, q = tq_from_set(ms, 0, pl)
    want, ev = rt.apply(s, rt.table(), 1 / 30, t, q, ALL_AXES, True, place)
    gu.assert_bits_equal(clean, want, "the clean run")
    assert ev["fold_forwards_a"].sum() + ev["fold_forwards_b"].sum() >= 8
    # side b of the rows on A, side a of the rows on B: an id far outside the bank and a NaN clock
    bad = dict(clips_a=np.where(side == 1, 0x7FFFFFF0, s["clips_a"]), clips_b=np.where(side == 0, 0x7FFFFFF0, s["clips_b"]),
               times_a=np.where(side == 1, np.nan, s["times_a"]), times_b=np.where(side == 0, np.nan, s["times_b"]))
    poke(an, **bad)
    d_place.upload(place)
    an.root_turn(ms, 0, ALL_AXES, d_place.ptr, dt=1 / 30, normalize=True)
    gu.assert_bits_equal(d_place.download((n, 8), F), clean, "with the unread sides poisoned")
    # a side b that is not fading is not read either, whatever the weight says
    s2 = {k: v.copy() for k, v in s.items()}
    s2["fade_rate"][:] = 0.0
    an.set_state(**s2)
    d_place.upload(place)
    an.root_turn(ms, 0, ALL_AXES, d_place.ptr, dt=1 / 30)
    calm = d_place.download((n, 8), F)
    poke(an, clips_b=np.full(n, 0x7FFFFFF0, np.uint32), times_b=np.full(n, np.nan))
    d_place.upload(place)
    an.root_turn(ms, 0, ALL_AXES, d_place.ptr, dt=1 / 30)
    gu.assert_bits_equal(d_place.download((n, 8), F), calm, "side b without a fade, poisoned")
    pl = rm.plan(s2, rt.table(), 1 / 30)
    t, q = tq_from_set(ms, 0, pl)
    gu.assert_bits_equal(calm, rt.apply(s2, rt.table(), 1 / 30, t, q, ALL_AXES, False, place)[0], "side b without a fade")
    _close(an, ms, d_place)


# ---------------------------------------------------------------------------------------- the Q8 walk ----
@pytest.mark.gpu
def test_gpu_q8_walk_across_the_seams_is_exact():
    """root_q8 from 0 with dt = 0.5, twelve steps (three laps): every sample is a key, every rotation a member of the quaternion
    group, every translation dyadic.  The evaluator returns the keys' own bits, and the placement after every step equals the
    restatement's, whose matrix tests/test_root_turn_cpu.py holds to the float64 closed form with no tolerance.  Animator.step
    with turn=True issues both calls."""
    ms = rt.root_bank()
    an = vmd.Animator(ms, 2, [tuple(r) for r in rt.CLIP_ROWS])
    an.request([0, 1], [rt.Q8, rt.Q8])
    an.advance(0.0)
    times = np.array([0.0, 0.5, 1.0, 1.5, 2.0])
    rows = ms.eval_bones_time(np.full(times.size, rt.Q8, np.uint32), times)[:, 0]
    t, q = rt.q8_at(times)
    gu.assert_bits_equal(rows[:, :3], t, "T of the walk")
    gu.assert_bits_equal(rows[:, 4:], q, "Q of the walk")
    want = {normalize: cpu.q8_walk(normalize) for normalize in (False, True)}
    assert want[False][2] == 3
    d_place = DeviceBuffer.from_numpy(np.stack([cpu.Q8_PLACE, cpu.Q8_PLACE]))
    for k in range(rt.Q8_STEPS):
        # instance 0 and 1 share the call, so the flag is the call's: run the walk twice instead
        an.step(ms, 0, ALL_AXES, d_place.ptr, dt=rt.Q8_DT, turn=True, normalize=False)
        got = d_place.download((2, 8), F)
        gu.assert_bits_equal(got[0], want[False][0][k], f"step {k}")
        gu.assert_bits_equal(got[1], want[False][0][k], f"step {k}, instance 1")
        assert np.array_equal(rt.world(got[0, :3], got[0, 4:]), want[False][1][k]), k          # the float64 chain, exactly
    assert an.get_state(names=("loops",))["loops"].tolist() == [3, 3]
    d_place.upload(np.stack([cpu.Q8_PLACE, cpu.Q8_PLACE]))
    for k in range(rt.Q8_STEPS):
        an.step(ms, 0, ALL_AXES, d_place.ptr, dt=rt.Q8_DT, turn=True, normalize=True)
    gu.assert_bits_equal(d_place.download((2, 8), F)[0], want[True][0][-1], "the normalised walk")
    _close(an, ms, d_place)


# ---------------------------------------------------------------------------------------- in place ----
@pytest.mark.gpu
def test_gpu_in_place_turn_rows_equal_the_source_except_the_root():
    """The rows of an in-place-turn copy through the kernels, at times and at whole frames: the source's, except the root's masked
    channels and a root rotation of exactly {0,0,0,1} in every bit."""
    names = rm.rig_small_names() + [rt.ROOT_NAME]
    root = len(names) - 1
    z = rt.fixture()
    times = np.unique(np.concatenate([z["times"].reshape(-1), np.arange(0, 63) / 30.0, [-1.0, 9.0]]))
    frames = np.arange(0, 62, dtype=np.uint32)
    for name, path in (("curved", rm.VMDS["curved"]), ("q8", rt.Q8_VMD), ("still", rm.VMDS["still"]), ("no_root", rm.VMDS["no_root"])):
        v = vmd.Vmd(path)
        bm = v.bind_bones(names)
        src_t, src_f = bm.eval_time(times), bm.eval(frames)
        if name in ("curved", "q8"):
            assert (src_t[:, root, 4:] != rt.IDENTITY).any(1).sum() > times.size // 2
        for axes in (ALL_AXES, api.ROOT_X | api.ROOT_Z, 0):
            ip = bm.in_place_turn(root, axes)
            for what, got, src in (("times", ip.eval_time(times), src_t), ("frames", ip.eval(frames), src_f)):
                want = src.copy()
                for c in range(3):
                    if axes & (1 << c):
                        want[:, root, c] = 0.0
                want[:, root, 4:] = rt.IDENTITY
                gu.assert_bits_equal(got, want, f"{name}, axes {axes}, {what}")
            ip.close()
        _close(bm, v)


# ---------------------------------------------------------------------------------------- the C++ mirror ----
@pytest.mark.gpu
def test_cpp_root_turn_matches_python_path(tmp_path):
    """host/motion_example.cpp --crowd ends with a crowd that walks and turns: mmdx::MotionSet built with in_place_turn,
    mmdx::Animator::StepTurn with the moving set, the blend solve and PlacePalettes for 60 steps.  The same sequence from Python
    gives the same placements and placed palettes."""
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
    assert r.returncode == 0 and "turned checksum=" in r.stderr, r.stdout + r.stderr
    pm = pmx.load_pmx(str(tmp_path / "m.pmx"))
    vs = [vmd.Vmd(p) for p in paths]
    bms, mms = [v.bind_bones(pm.bone_names) for v in vs], [v.bind_morphs(pm.morph_names) for v in vs]
    still = [b.in_place_turn(0, ALL_AXES) for b in bms]
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
            an.step(moving, 0, ALL_AXES, d_where.ptr, dt=1.0 / hz, model=dm, turn=True, normalize=True)
            sk.solve_motion_set_blend_time_device(in_place, ni, *an.operand_ptrs(), d_pal.ptr, dm)
            dm.place_palettes(ni, d_pal.ptr, d_where.ptr, d_pal.ptr, dev)
        dm.sync()
        pal, walked = d_pal.download((ni, nb, 16), F), d_where.download((ni, 8), F)
        _close(an, d_where, d_pal)
    assert (walked[:, 4:] != where[:, 4:]).any(1).sum() >= ni // 3 and not np.isnan(pal).any()      # the first clip turns bone 0
    norm = np.sqrt((walked[:, 4:].astype(np.float64) ** 2).sum(1))
    assert np.abs(norm[(walked[:, 4:] != where[:, 4:]).any(1)] - 1).max() < 1e-6                     # normalised by the call

    def fnv(a):
        h = 1469598103934665603
        for byte in np.ascontiguousarray(a).view(np.uint8).ravel().tolist():
            h = ((h ^ byte) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
        return h
    want = "turned checksum=%016x where=%016x" % (fnv(pal), fnv(walked))
    assert want in r.stderr, (want, r.stderr)
    _close(moving, in_place, sk, still, bms, mms, vs)


# ---------------------------------------------------------------------------------------- the recorded frame ----
@pytest.mark.gpu
def test_gpu_graph_of_root_turn_advance_solve_and_place():
    """{root turn, advance (one device dt), blend solve of the in-place-turn set, place with the placements on the device} recorded
    once and replayed eight times with dt rewritten: placements and palettes equal the unrecorded sequence on a second animator,
    every bit."""
    m = synth.make_model(2048, 64, 8, 200, 112)
    names = [f"bone{i}" for i in range(m.nb)]
    ni = 9
    sk = vmd.Skeleton(m.bone_pos, np.asarray(m.bone_parent, np.int32))
    vs = [vmd.Vmd(d) for d in ta.scenario_vmds(names)]
    moving = [v.bind_bones(names) for v in vs]
    still = [b.in_place_turn(0, ALL_AXES) for b in moving]
    roots = [v.bind_bones(names[:1]) for v in vs]
    in_place_set = vmd.MotionSet(still)
    root_set = vmd.MotionSet(roots)
    start = ar.initial_state(ni)
    start["clips_a"][:] = [0, 3, 5, NONE, 2, 6, 0, 4, 6]
    start["times_a"][:] = [1.9, 0.6, 0.7, 0.0, 1.4, 0.39, 0.1, 0.2, 0.0]
    start["speed"][:] = [1.0, 1.0, 0.5, 1.0, -1.0, 1.0, -1.0, 1.0, 2.0]
    start["clips_b"][:3] = [2, 0, 6]
    start["fade_rate"][:3] = 2.0
    start["weights"][:3] = [0.2, 0.5, 0.8]
    dts = [1 / 60, 1 / 30, 0.25, 1 / 144, 1 / 60, 0.5, -1 / 30, 1 / 60]
    place0 = headings(ni, 78)
    dev = api.PALETTE_ON_DEVICE | api.OUT_ON_DEVICE
    with DeformModel(m) as dm:
        eager, replayed = (vmd.Animator(in_place_set, ni, ta.rows_for_create()) for _ in range(2))
        d_dt = DeviceBuffer.from_numpy(np.array([0.0], np.float64))
        d_place, d_pal = DeviceBuffer(ni * 32), DeviceBuffer(ni * m.nb * 64)

        def frame(an):
            an.root_turn(root_set, 0, ALL_AXES, d_place.ptr, dt_ptr=d_dt.ptr, model=dm, normalize=True)
            an.advance_device_dt(d_dt.ptr, dm)
            sk.solve_motion_set_blend_time_device(in_place_set, ni, *an.operand_ptrs(), d_pal.ptr, dm)
            dm.place_palettes(ni, d_pal.ptr, d_place.ptr, d_pal.ptr, dev | api.PLACE_ON_DEVICE)

        def results():
            dm.sync()
            return d_place.download((ni, 8), F), d_pal.download((ni, m.nb, 16), F)
        eager.set_state(dm, **start)
        d_place.upload(place0)
        want = []
        for dt in dts:
            d_dt.upload(np.array([dt], np.float64))
            frame(eager)
            want.append(results())
        assert len({w[0].tobytes() for w in want}) == len(dts) and not any(np.isnan(x).any() for w in want for x in w)
        assert (want[-1][0][:, 4:] != place0[:, 4:]).any(1).sum() >= ni - 2
        # the run before recording, as the header requires; then back to the start
        frame(replayed)
        dm.sync()
        replayed.set_state(dm, **start)
        d_place.upload(place0)
        dm.graph_begin()
        frame(replayed)
        g = dm.graph_end()
        gu.assert_bits_equal(d_place.download((ni, 8), F), place0, "recording does not run anything")
        for k, dt in enumerate(dts):
            d_dt.upload(np.array([dt], np.float64))
            d_pal.memset(0)
            g.launch()
            for what, a, b in zip(("placements", "palettes"), results(), want[k]):
                gu.assert_bits_equal(a, b, f"replay {k}: {what}")
        ar.assert_states_equal(replayed.get_state(dm), eager.get_state(dm), "the state after eight replays")
        g.close()
        _close(eager, replayed, d_dt, d_place, d_pal)
    _close(root_set, in_place_set, roots, still, moving, vs, sk)

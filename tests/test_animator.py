"""The crowd animator: mmdx_motion_set_clip_frames and the mmdx_animator_* family (include/mmdx.h).

There is no reference to measure against beyond Motion::GetLength: the contract is the arithmetic the header states, held by
three independent statements that must agree bit for bit, with no tolerance anywhere --
  * csrc/anim_math.hpp compiled for the host (tests/anim_math_driver.cpp, a stand-alone program, plain and sanitized),
  * the numpy restatement tests/animator_ref.py,
  * the gfx950 kernel (the same header compiled for the device),
and on the GPU the animator's arrays feed the existing blend calls unchanged.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from simple_mmd_renderer_amd import _capi as api
from simple_mmd_renderer_amd import synth, vmd
from simple_mmd_renderer_amd.engine import DeformModel, DeviceBuffer
from tests import animator_ref as ar
from tests import golden_util as gu
from tests import host_program as hp
from tests import motion_blend_ref as mb
from tests import motion_time_ref as mt
from tests.test_capi_symbols import declared_symbols

ENTRY_POINTS = ("mmdx_motion_set_clip_frames", "mmdx_animator_create", "mmdx_animator_destroy", "mmdx_animator_get_info",
                "mmdx_animator_operands", "mmdx_animator_device_arrays", "mmdx_animator_set_state", "mmdx_animator_get_state",
                "mmdx_animator_request", "mmdx_animator_advance")
NONE, NO_REQUEST = vmd.CLIP_NONE, vmd.ANIM_NO_REQUEST
ROOT = hp.ROOT
needs_driver = pytest.mark.skipif(not mt.driver_available(), reason="the reference's libmmd headers are not present")


@pytest.fixture(autouse=True)
def _lib(hip_lib):
    return hip_lib


def close_all(*xs):
    for x in xs:
        for y in (x if isinstance(x, (list, tuple)) else [x]):
            y.free() if isinstance(y, DeviceBuffer) else y.close()


# ---------------------------------------------------------------------------------------- CPU ----
def test_animator_entry_points_are_declared_exported_and_bound(hip_lib):
    syms = declared_symbols()
    for name in ENTRY_POINTS:
        assert name in syms and hasattr(hip_lib, name) and name in api.SIGNATURES, name
    hdr = open(os.path.join(ROOT, "include", "mmdx.h")).read()
    for text in ("typedef struct mmdx_animator_desc {", "typedef struct mmdx_animator_clip {", "typedef struct mmdx_animator_arrays {",
                 "typedef struct mmdx_animator_info {", "#define MMDX_ABI_VERSION 3u", "#define MMDX_ANIM_NO_REQUEST 0xFFFFFFFEu",
                 "MMDX_ANIM_DT_ON_DEVICE = 1u << 10", "a recorded graph freezes that value"):
        assert text in hdr, text
    assert hip_lib.mmdx_abi_version() == 3
    assert (ar.NONE, ar.NO_REQUEST, ar.LOOP, ar.HOLD, ar.THEN) == (NONE, NO_REQUEST, vmd.ANIM_LOOP, vmd.ANIM_HOLD, vmd.ANIM_THEN)
    # 64-bit layouts by hand from the header
    assert C.sizeof(vmd.AnimatorClip) == 8 + 4 * 4                        # a double, three u32 / f32, reserved0
    assert C.sizeof(vmd.AnimatorDesc) == 2 * 4 + 8 + 2 * 4                # two u32, a pointer, two u32
    assert C.sizeof(vmd.AnimatorInfo) == 4 * 4
    assert C.sizeof(vmd.AnimatorArrays) == 2 * 4 + 11 * 8                 # two u32, eleven pointers
    assert [k for k, _ in vmd.ANIMATOR_ARRAYS] == [k for k, _ in ar.ARRAYS]
    for name in ("advance", "advance_device_dt", "request", "set_state", "get_state", "operands", "close"):
        assert callable(getattr(vmd.Animator, name)), name
    assert callable(vmd.MotionSet.clip_frames)
    poser = open(os.path.join(ROOT, "simple_mmd_renderer_amd", "host", "mmdx_poser.hpp")).read()
    for call in ("mmdx_animator_create(", "mmdx_animator_advance(", "mmdx_animator_request(", "mmdx_animator_operands(",
                 "mmdx_animator_set_state(", "mmdx_animator_get_state(", "mmdx_motion_set_clip_frames("):
        assert call in poser, call
    assert "class Animator" in poser


def _max_frame(v, bone_names=None, morph_names=None):
    """The largest key frame of a parsed Vmd over the tracks with the given names (None: that side does not take part)."""
    frames = [0]
    if bone_names is not None:
        frames += [k["frame"] for i, n in enumerate(v.bone_track_names) if n in bone_names for k in v.bone_track(i)]
    if morph_names is not None:
        frames += [int(f) for i, n in enumerate(v.morph_track_names) if n in morph_names for f in v.morph_track(i)[0]]
    return max(frames)


def test_clip_frames_is_the_largest_key_frame_of_the_bound_tracks():
    z = mb.fixture()
    bvs, mvs = [vmd.Vmd(p) for p in mb.BONE_VMDS], [vmd.Vmd(p) for p in mb.MORPH_VMDS]
    bms, mms = [v.bind_bones(z["bone_names"]) for v in bvs], [v.bind_morphs(z["morph_names"]) for v in mvs]
    want_b = [_max_frame(v, bone_names=z["bone_names"]) for v in bvs]
    want_m = [_max_frame(v, morph_names=z["morph_names"]) for v in mvs]
    assert min(want_b) > 0 and min(want_m) > 0 and want_b != want_m
    both, bones, morphs = vmd.MotionSet(bms, mms), vmd.MotionSet(bms), vmd.MotionSet(morph_motions=mms)
    assert both.clip_frames().tolist() == [max(b, m) for b, m in zip(want_b, want_m)]
    assert bones.clip_frames().tolist() == want_b and morphs.clip_frames().tolist() == want_m
    # a subset of the tracks: only their keys count; no bound track at all: 0
    few = [n for n in z["bone_names"] if n in bvs[0].bone_track_names][:1]
    sub = [v.bind_bones(few) for v in bvs]
    none = [v.bind_bones(["no such bone"]) for v in bvs]
    s_sub, s_none = vmd.MotionSet(sub), vmd.MotionSet(none)
    assert s_sub.clip_frames().tolist() == [_max_frame(v, bone_names=few) for v in bvs]
    assert s_none.clip_frames().tolist() == [0, 0]
    # every track of one file bound on both sides: the file's max_frame
    v = bvs[1]
    all_b, all_m = v.bind_bones(v.bone_track_names), v.bind_morphs(v.morph_track_names)
    whole = vmd.MotionSet([all_b], [all_m])
    assert whole.clip_frames().tolist() == [v.info["max_frame"]] and v.info["max_frame"] > 0
    # the animator's default table: every clip loops over double(frames) / 30.0
    an = vmd.Animator(both, 3)
    assert an.clip_table() == [(np.float64(f) / np.float64(30.0), vmd.ANIM_LOOP, NONE, 0.0) for f in both.clip_frames()]
    assert api.lib().mmdx_motion_set_clip_frames(None, None) == 1
    close_all(an, whole, all_b, all_m, s_sub, s_none, sub, none, both, bones, morphs, bms, mms, bvs, mvs)


@needs_driver
def test_clip_frames_equals_get_length_of_libmmd():
    """Motion::GetLength() of the real libmmd over the same bytes, every track of the file bound."""
    lib = C.CDLL(hp.build("anim_len", [os.path.join(hp.TESTS, "anim_math_driver.cpp")], strict=False, shared=True, include=[hp.REF_INC],
                          define=["ANIM_DRIVER_LIBMMD"]))
    lib.amd_motion_length.restype, lib.amd_motion_length.argtypes = C.c_longlong, [C.c_char_p]
    for path in sorted(set(mb.BONE_VMDS + mb.MORPH_VMDS)):
        v = vmd.Vmd(path)
        sides = ([v.bind_bones(v.bone_track_names)] if v.info["n_bone_tracks"] else None,
                 [v.bind_morphs(v.morph_track_names)] if v.info["n_morph_tracks"] else None)
        ms = vmd.MotionSet(*sides)
        assert ms.clip_frames().tolist() == [lib.amd_motion_length(path.encode())], path
        close_all(ms, *[s for s in sides if s], v)


def count_events(events, name, where=None):
    return int(sum((ev[name] if where is None else ev[name] & where(ev)).sum() for ev in events))


def check_coverage(table, state, dts, requests, states, events):
    """The sweep provably goes through every case the issue names."""
    nc = table["length"].size
    assert set(table["mode"].tolist()) == {ar.LOOP, ar.HOLD, ar.THEN} and (table["length"] == 0).any()      # every mode, a length 0
    first = [state] + states[:-1]
    played = np.concatenate([s["clips_a"] for s in first])
    assert set(played[played < nc].tolist()) == set(range(nc))                                              # every clip on side a
    a, b, fading = state["clips_a"], state["clips_b"], state["fade_rate"] > 0
    assert (fading & (a == NONE) & (b != NONE)).any() and (fading & (a != NONE) & (b == NONE)).any() and (fading & (a == NONE) & (b == NONE)).any()
    assert ((a == NONE) & ~fading).any()
    want_dts = {0.0, 1 / 144, 1 / 60, 1 / 30, 7.0, -1 / 60}
    assert want_dts <= set(dts.tolist()) and 7.0 == 3.5 * table["length"][0] and table["mode"][0] == ar.LOOP
    assert set(state["speed"].tolist()) == {1.0, 0.5, -1.0, 0.0}
    fades = np.concatenate([r[2] for r in requests])
    assert (fades == 0).any() and ((fades > 0) & (fades < 1 / 144)).any() and (fades > 10 / 60).any()        # at once, < a step, many steps
    n = {k: count_events(events, k) for k in events[0]}
    assert min(n[k] for k in ("fold", "fading", "promote", "request", "request_waits", "then", "then_none", "at_once", "fade_started",
                              "promote_and_go", "on_length")) >= 3, n
    # a step that spans several lengths folds once; a backwards step folds too
    for k, (ev, s0, s1) in enumerate(zip(events, first, states)):
        assert ((s1["loops"] - s0["loops"]) == ev["fold"]).all()
    big = [ev["fold"].sum() for ev, dt in zip(events, dts) if dt == 7.0]
    back = [ev["fold"].sum() for ev, dt in zip(events, dts) if dt < 0]
    assert min(big) > 0 and max(back) > 0
    # a fade shorter than a step is promoted in the step after it starts; THEN -> NONE leaves nothing playing
    assert any((ev["then_none"] & (s1["clips_a"] == NONE)).any() for ev, s1 in zip(events, states))
    return n


def test_host_build_of_the_arithmetic_equals_the_numpy_restatement():
    """300 steps of the sweep through the stand-alone driver of csrc/anim_math.hpp -- built plain, and with AddressSanitizer and
    UBSan -- and through tests/animator_ref.py: every array after every step, as bit patterns."""
    table, state, dts, requests = ar.sweep(96, 300)
    states, events = ar.run_reference(table, state, dts, requests)
    check_coverage(table, state, dts, requests, states, events)
    for sanitize in (False, True):
        got = ar.run_driver(ar.build_driver(sanitize), table, state, dts, requests)
        assert len(got) == 300
        for k, (g, w) in enumerate(zip(got, states)):
            ar.assert_states_equal(g, w, f"{'sanitized' if sanitize else 'plain'} driver, step {k}")
    # a NaN step changes nothing, in both statements
    nan_dts = np.array([1 / 60, np.nan, 1 / 60])
    want, _ = ar.run_reference(table, state, nan_dts, requests[:3])
    ar.assert_states_equal(want[1], {**want[0], **{k: want[1][k] for k in ("req_clip", "req_fade", "req_time")}}, "NaN dt in the restatement")
    got = ar.run_driver(ar.build_driver(False), table, state, nan_dts, requests[:3])
    for k in range(3):
        ar.assert_states_equal(got[k], want[k], f"NaN dt, step {k}")


def tiny_set():
    names = ["センター", "首"]
    v = vmd.Vmd(vmd.write_vmd(synth.make_bone_keys(names, 1, keys_per=3), [("あ", 0, 0.5), ("あ", 9, 1.0)]))
    bm = v.bind_bones(names)
    ms = vmd.MotionSet([bm, bm])
    close_all(bm, v)
    return ms


def test_animator_entry_points_refuse_bad_arguments():
    """Everything that needs no device is decided before the first HIP call, so it is checked here without a GPU."""
    lib = api.lib()
    err = lambda: lib.mmdx_last_error_string().decode()          # noqa: E731
    ms = tiny_set()
    h = C.c_void_p()

    def desc(ni=4, clips=None, n_clips=None, struct_size=None, reserved0=0):
        d = vmd.AnimatorDesc(C.sizeof(vmd.AnimatorDesc) if struct_size is None else struct_size, ni, None, 0, reserved0)
        if clips is not None:
            d.keep = (vmd.AnimatorClip * len(clips))(*[vmd.AnimatorClip(*c) for c in clips])
            d.clips, d.n_clips = C.addressof(d.keep), len(clips) if n_clips is None else n_clips
        return d
    create = lambda s, d: lib.mmdx_animator_create(s, C.byref(d) if d is not None else None, C.byref(h))      # noqa: E731
    ok_rows = [(0.0, vmd.ANIM_LOOP, 0, 0.0, 0), (1.0, vmd.ANIM_THEN, NONE, 0.5, 0)]
    assert lib.mmdx_animator_create(ms.h, C.byref(desc()), None) == 1 and "NULL" in err()
    assert create(None, desc()) == 1 and "NULL" in err()
    assert create(ms.h, None) == 1 and "NULL" in err()
    for size in (0, C.sizeof(vmd.AnimatorDesc) - 8, C.sizeof(vmd.AnimatorDesc) + 8):
        assert create(ms.h, desc(struct_size=size)) == 1 and "struct_size" in err()
    assert create(ms.h, desc(ni=0)) == 1 and "n_instances" in err()
    assert create(ms.h, desc(reserved0=1)) == 1 and "reserved0" in err()
    assert create(ms.h, desc(clips=ok_rows, n_clips=3)) == 1 and "n_clips" in err()
    assert create(ms.h, desc(clips=[ok_rows[0], (1.0, 3, 0, 0.0, 0)])) == 1 and "clips[1].mode" in err()
    assert create(ms.h, desc(clips=[ok_rows[0], (1.0, vmd.ANIM_THEN, 2, 0.0, 0)])) == 2 and "clips[1].next" in err()       # BAD_INDEX
    assert create(ms.h, desc(clips=[ok_rows[0], (1.0, vmd.ANIM_THEN, 0, float("nan"), 0)])) == 1 and "NaN" in err()
    assert create(ms.h, desc(clips=[ok_rows[0], (1.0, vmd.ANIM_HOLD, 0, 0.0, 7)])) == 1 and "reserved0" in err()
    assert h.value is None
    assert create(ms.h, desc(clips=ok_rows)) == 0 and h.value
    ms.close()                                                   # the animator copied what it needs of the set
    info = vmd.AnimatorInfo(C.sizeof(vmd.AnimatorInfo))
    table = (vmd.AnimatorClip * 2)()
    assert lib.mmdx_animator_get_info(h, C.byref(info), table) == 0
    assert (info.n_instances, info.n_clips, info.device_ordinal) == (4, 2, -1)
    assert table[0].length == np.float64(_tiny_frames()) / np.float64(30.0) and table[1].length == 1.0 and table[1].next == NONE
    assert lib.mmdx_animator_get_info(h, C.byref(vmd.AnimatorInfo(8)), None) == 1 and "struct_size" in err()
    assert lib.mmdx_animator_get_info(None, C.byref(info), None) == 1

    # advance
    dt, nan = C.c_double(1 / 60), C.c_double(float("nan"))
    assert lib.mmdx_animator_advance(None, None, C.byref(dt), 0) == 1 and "NULL" in err()
    assert lib.mmdx_animator_advance(h, None, None, 0) == 1 and "NULL" in err()
    assert lib.mmdx_animator_advance(h, None, C.byref(nan), 0) == 1 and "dt is NaN" in err()
    for bad in (1, 4, 1 << 9, 1 << 11, 1 << 31):
        assert lib.mmdx_animator_advance(h, None, C.byref(dt), bad) == 1 and "unknown flag" in err(), bad
    assert lib.mmdx_animator_advance(h, None, C.c_void_p(12), vmd.ANIM_DT_ON_DEVICE) == 1 and "aligned" in err()

    # request
    u32, f32, f64 = (lambda *x: np.array(x, np.uint32)), (lambda *x: np.array(x, np.float32)), (lambda *x: np.array(x, np.float64))

    def request(ids, clips, fades=None, times=None, flags=0, n=None):
        p = lambda a: a.ctypes.data if a is not None else None      # noqa: E731
        return lib.mmdx_animator_request(h, None, len(ids) if n is None else n, p(ids), p(clips), p(fades), p(times), flags)
    assert lib.mmdx_animator_request(None, None, 1, None, None, None, None, 0) == 1 and "NULL" in err()
    assert request(u32(0), None, n=1) == 1 and "NULL" in err()
    assert request(None, u32(0), n=1) == 1 and "NULL" in err()
    for bad in (2, 4, 1 << 10, 1 << 31):
        assert request(u32(0), u32(0), flags=bad) == 1 and "unknown flag" in err(), bad
    assert request(u32(0, 4), u32(0, 1)) == 2 and "ids[1] = 4" in err()                      # an instance id >= NI
    assert request(u32(0, 1), u32(0, 2)) == 2 and "clips[1] = 2" in err()                    # a clip id >= n_clips
    assert request(u32(0, 1), u32(0, NO_REQUEST)) == 2 and "clips[1]" in err()
    assert request(u32(0, 1), u32(0, 1), f32(0, np.nan)) == 1 and "fades[1] is NaN" in err()
    assert request(u32(0, 1), u32(0, NONE), f32(0, 0), f64(np.nan, 0)) == 1 and "start_times[0] is NaN" in err()
    assert request(u32(0, 1, 2, 3, 0), u32(0, 0, 0, 0, 0)) == 1 and "distinct" in err()
    assert request(u32(), u32()) == 0                                                         # nothing to do, no device needed

    # set_state / get_state
    def arrays(ni=4, struct_size=None, **given):
        s = vmd.AnimatorArrays(C.sizeof(vmd.AnimatorArrays) if struct_size is None else struct_size, ni)
        s.keep = given
        for k, a in given.items():
            setattr(s, k, a.ctypes.data)
        return s
    for fn in (lib.mmdx_animator_set_state, lib.mmdx_animator_get_state):
        assert fn(None, None, C.byref(arrays())) == 1 and "NULL" in err()
        assert fn(h, None, None) == 1 and "NULL" in err()
        assert fn(h, None, C.byref(arrays(struct_size=88))) == 1 and "struct_size" in err()
        assert fn(h, None, C.byref(arrays(ni=5))) == 1 and "n_instances" in err()
    st = lib.mmdx_animator_set_state
    assert st(h, None, C.byref(arrays(clips_a=u32(0, 1, NONE, 2)))) == 2 and "clips_a[3] = 2" in err()
    assert st(h, None, C.byref(arrays(clips_b=u32(0, 1, NONE, NO_REQUEST)))) == 2 and "clips_b[3]" in err()
    assert st(h, None, C.byref(arrays(req_clip=u32(0, NO_REQUEST, NONE, 5)))) == 2 and "req_clip[3] = 5" in err()
    for k, a in (("times_a", f64(0, np.nan, 0, 0)), ("times_b", f64(0, np.nan, 0, 0)), ("req_time", f64(0, np.nan, 0, 0)),
                 ("weights", f32(0, np.nan, 0, 0)), ("speed", f32(0, np.nan, 0, 0)), ("fade_rate", f32(0, np.nan, 0, 0)),
                 ("req_fade", f32(0, np.nan, 0, 0))):
        assert st(h, None, C.byref(arrays(**{k: a}))) == 1 and k + "[1] is NaN" in err(), k

    # operands / device arrays
    assert lib.mmdx_animator_operands(None, C.byref(vmd.MotionBlendArgs())) == 1 and "NULL" in err()
    assert lib.mmdx_animator_operands(h, None) == 1 and "NULL" in err()
    assert lib.mmdx_animator_device_arrays(h, None) == 1 and "NULL" in err()
    assert lib.mmdx_animator_device_arrays(h, C.byref(vmd.AnimatorArrays(8, 4))) == 1 and "struct_size" in err()
    lib.mmdx_animator_destroy(h)
    lib.mmdx_animator_destroy(None)
    # the Python face raises the same statuses
    ms = tiny_set()
    with pytest.raises(api.MmdxError) as e:
        vmd.Animator(ms, 4, [(0.0, vmd.ANIM_THEN, 9, 0.0), (0.0, vmd.ANIM_LOOP, 0, 0.0)])
    assert e.value.status == 2
    an = vmd.Animator(ms, 4)
    with pytest.raises(api.MmdxError) as e:
        an.advance(float("nan"))
    assert e.value.status == 1
    with pytest.raises(api.MmdxError) as e:
        an.request([7], [0])
    assert e.value.status == 2
    with pytest.raises(ValueError):
        an.request([0, 1], [0])
    with pytest.raises(ValueError):
        an.set_state(speed=[1.0])
    close_all(an, ms)


def _tiny_frames():
    ms = tiny_set()
    f = int(ms.clip_frames()[0])
    ms.close()
    return f


# ---------------------------------------------------------------------------------------- GPU ----
def scenario_vmds(bone_names, morph_names=()):
    """Seven clips whose last key frames are animator_ref.CLIP_FRAMES (clip 1: a single key at frame 0, length 0)."""
    out = []
    for c, last in enumerate(ar.CLIP_FRAMES):
        rng = np.random.RandomState(100 + c)
        frames = sorted({0, last} | set(rng.randint(0, last + 1, 3).tolist()))
        bone_keys = []
        for n in bone_names[c % 2::2] or bone_names:
            for f in frames:
                q = rng.normal(size=4)
                bone_keys.append((n, f, tuple(rng.uniform(-1, 1, 3)), tuple(q / np.linalg.norm(q)), None))
        morph_keys = [(n, f, float(np.float32(rng.uniform(0, 1)))) for n in morph_names for f in frames]
        out.append(vmd.write_vmd(bone_keys, morph_keys))
    return out


def scenario_set(bone_names, morph_names=()):
    vs = [vmd.Vmd(d) for d in scenario_vmds(bone_names, morph_names)]
    bms = [v.bind_bones(bone_names) for v in vs]
    mms = [v.bind_morphs(morph_names) for v in vs] if morph_names else None
    ms = vmd.MotionSet(bms, mms)
    close_all(bms, mms or [], vs)
    assert ms.clip_frames().tolist() == list(ar.CLIP_FRAMES)
    return ms


def rows_for_create():
    return [(l, m, n, f) for l, m, n, f in ar.CLIP_ROWS]


@pytest.mark.gpu
@pytest.mark.parametrize("device_dt", [False, True], ids=["host_dt", "device_dt"])
@pytest.mark.parametrize("ni", [1, 63, 64, 65, 257])
def test_gpu_advance_equals_the_restatement(ni, device_dt):
    """60 steps of the sweep, requests from host lists before the steps that have them: all eleven arrays after every step."""
    table, state, dts, requests = ar.sweep(ni, 60)
    want, _ = ar.run_reference(table, state, dts, requests)
    ms = scenario_set(["b0", "b1", "b2"])
    an = vmd.Animator(ms, ni, rows_for_create())
    got_table = an.clip_table()
    assert [r[0] for r in got_table] == table["length"].tolist()
    ar.assert_states_equal(an.get_state(), ar.initial_state(ni), "the initial state")
    an.set_state(**state)
    d_dt = DeviceBuffer(8)
    for k, (dt, req) in enumerate(zip(dts, requests)):
        if req[0].size:
            an.request(*req)
        if device_dt:
            d_dt.upload(np.array([dt], np.float64))
            an.advance_device_dt(d_dt.ptr)
        else:
            an.advance(dt)
        ar.assert_states_equal(an.get_state(), want[k], f"NI {ni}, step {k} (dt {dt})")
    close_all(an, ms, d_dt)


@pytest.mark.gpu
def test_gpu_nan_device_dt_changes_nothing_and_device_requests_skip_bad_ids():
    ni = 65
    table, state, dts, requests = ar.sweep(ni, 4)
    ms = scenario_set(["b0", "b1", "b2"])
    an = vmd.Animator(ms, ni, rows_for_create())
    an.set_state(**state)
    d_dt = DeviceBuffer.from_numpy(np.array([np.nan], np.float64))
    an.advance_device_dt(d_dt.ptr)
    ar.assert_states_equal(an.get_state(), state, "after a NaN step")
    # a device list with ids >= NI in the middle: skipped, the neighbours applied
    ids = np.array([3, ni, 64, 0xFFFFFFFF, 0, ni + 1000, 17], np.uint32)
    clips = np.array([1, 2, NONE, 3, 6, 4, 2], np.uint32)
    fades = np.array([0.0, 0.3, 0.005, 0.3, 0.3, 0.0, 0.0], np.float32)
    times = np.array([0.0, 0.1, 0.1, 0.0, 0.1, 0.0, 0.1], np.float64)
    ds = [DeviceBuffer.from_numpy(a) for a in (ids, clips, fades, times)]
    an.request_device(ids.size, *[d.ptr for d in ds])
    want = {k: v.copy() for k, v in state.items()}
    ar.apply_requests(want, ids, clips, fades, times)
    assert (want["req_clip"] != state["req_clip"]).sum() >= 3
    ar.assert_states_equal(an.get_state(), want, "after the device request")
    # without fades / start times: 0
    an.request_device(2, ds[0].ptr, ds[1].ptr)
    ar.apply_requests(want, ids[:2], clips[:2], [0.0, 0.0], [0.0, 0.0])
    ar.assert_states_equal(an.get_state(), want, "after the device request without fades")
    d_dt.upload(np.array([1 / 60], np.float64))
    an.advance_device_dt(d_dt.ptr)
    want, _ = ar.advance(want, table, 1 / 60)
    ar.assert_states_equal(an.get_state(), want, "the step after")
    close_all(an, ms, ds, d_dt)


@pytest.mark.gpu
def test_gpu_set_state_and_get_state_round_trip_and_partial_updates():
    ni = 65
    _, state, _, _ = ar.sweep(ni, 1)
    ms = scenario_set(["b0", "b1", "b2"])
    an = vmd.Animator(ms, ni)
    an.set_state(**state)
    ar.assert_states_equal(an.get_state(), state, "round trip")
    addr = an.device_arrays()
    ops = an.operands()
    assert (ops.clips_a, ops.clips_b, ops.times_a, ops.times_b, ops.weights) == tuple(addr[k] for k in ("clips_a", "clips_b", "times_a", "times_b", "weights"))
    assert ops.struct_size == C.sizeof(vmd.MotionBlendArgs) and ops.n_instances == ni
    assert ops.flags == vmd.TIMES_ON_DEVICE | api.OUT_ON_DEVICE
    spans = sorted((addr[k], addr[k] + ni * np.dtype(t).itemsize) for k, t in ar.ARRAYS)
    assert all(a1 <= b0 for (_, a1), (b0, _) in zip(spans, spans[1:]))
    assert all(addr[k] % np.dtype(t).itemsize == 0 for k, t in ar.ARRAYS)
    # a partial update leaves the other arrays' bytes alone
    speed = np.linspace(-2, 2, ni).astype(np.float32)
    req = np.where(np.arange(ni) % 3 == 0, 2, NO_REQUEST).astype(np.uint32)
    an.set_state(speed=speed, req_clip=req)
    want = dict(state, speed=speed, req_clip=req)
    ar.assert_states_equal(an.get_state(), want, "after a partial update")
    part = an.get_state(names=("loops", "times_b"))
    assert sorted(part) == ["loops", "times_b"]
    gu.assert_bits_equal(part["times_b"], state["times_b"], "times_b alone")
    # the arrays are where device_arrays says
    raw = DeviceBuffer.adopt(addr["speed"], ni * 4)
    gu.assert_bits_equal(raw.download((ni,), np.float32), speed, "speed through its device address")
    raw.ptr = None
    close_all(an, ms)


def _rig(name):
    if name == "ik":
        z = np.load(os.path.join(gu.GOLDEN_DIR, "rig_ik_expect.npz"))
        ik = {k[3:]: z[k] for k in z.files if k.startswith("ik_")}
        return vmd.Skeleton(z["rest"], z["parent"], z["level"], z["flags"], z["append_parent"], z["append_ratio"], ik), vmd.SOLVER_SERIAL
    z = np.load(os.path.join(gu.GOLDEN_DIR, "rig_small_expect.npz"))
    return vmd.Skeleton(z["rest"], z["parent"], z["level"], z["flags"]), vmd.SOLVER_PARALLEL_FK


@pytest.mark.gpu
@pytest.mark.parametrize("rig", ["fk", "ik"])
def test_gpu_operands_feed_the_blend_calls_unchanged(rig):
    """20 steps at NI = 65: the palettes and rates the existing blend calls compute from the animator's device arrays equal those of
    the same calls given the restatement's arrays as host operands."""
    ni = 65
    sk, solver = _rig(rig)
    assert sk.info["solver"] == solver
    names, mnames = [f"b{i}" for i in range(sk.nb)], ["m0", "m1", "m2"]
    ms = scenario_set(names, mnames)
    table, state, dts, requests = ar.sweep(ni, 20)
    want, events = ar.run_reference(table, state, dts, requests)
    assert sum(int(ev["fading"].sum()) for ev in events) > 100 and sum(int(ev["promote"].sum()) for ev in events) > 5
    an = vmd.Animator(ms, ni, rows_for_create())
    an.set_state(**state)
    d_pal, d_w = DeviceBuffer(ni * sk.nb * 64), DeviceBuffer(ni * 3 * 4)
    seen = set()
    for k, (dt, req) in enumerate(zip(dts, requests)):
        if req[0].size:
            an.request(*req)
        an.advance(dt)
        d_pal.memset(0xFF); d_w.memset(0xFF)
        sk.solve_motion_set_blend_time_device(ms, ni, *an.operand_ptrs(), d_pal.ptr)
        ms.blend_morphs_time_device(ni, *an.operand_ptrs(), d_w.ptr)
        w = want[k]
        host = (w["clips_a"], w["times_a"], w["clips_b"], w["times_b"], w["weights"])
        pal = d_pal.download((ni, sk.nb, 16), np.float32)
        gu.assert_bits_equal(pal, sk.solve_motion_set_blend_time(ms, *host), f"{rig}: palettes, step {k}")
        gu.assert_bits_equal(d_w.download((ni, 3), np.float32), ms.blend_morphs_time(*host), f"{rig}: rates, step {k}")
        seen.add(pal.tobytes())
    assert len(seen) >= np.count_nonzero(dts) >= 18               # the crowd moved in every step that was not dt == 0
    close_all(an, ms, sk, d_pal, d_w)


@pytest.mark.gpu
def test_gpu_graph_of_advance_blend_solve_morphs_and_deform():
    """{advance with a device dt, blend solve, blend morphs, mmdx_deform_batched} recorded once and replayed six times, a new dt
    written before every replay and one request between replays 3 and 4: palettes and vertices equal the eager sequence run on a
    second animator.  Destroying the animator invalidates the graph."""
    m = synth.make_model(2048, 64, 8, 200, 112)                                   # the size of g12_mini_model
    names, mnames = [f"bone{i}" for i in range(m.nb)], [f"morph{i}" for i in range(m.nm)]
    ni = 5
    sk = vmd.Skeleton(m.bone_pos, np.asarray(m.bone_parent, np.int32))
    ms = scenario_set(names, mnames)
    flags = api.PALETTE_ON_DEVICE | api.WEIGHTS_ON_DEVICE | api.OUT_ON_DEVICE
    start = ar.initial_state(ni)
    start["clips_a"][:] = [0, 3, 5, NONE, 2]
    start["times_a"][:] = [1.9, 0.6, 0.7, 0.0, 1.4]
    start["speed"][:] = [1.0, 1.0, 0.5, 1.0, -1.0]
    dts = [1 / 60, 1 / 30, 0.25, 1 / 144, 1 / 60, 0.5]
    request = (np.array([3, 0], np.uint32), np.array([6, NONE], np.uint32), np.array([0.0, 0.3], np.float32), np.array([0.1, 0.0]))
    with DeformModel(m) as dm:
        eager, replayed = vmd.Animator(ms, ni, rows_for_create()), vmd.Animator(ms, ni, rows_for_create())
        d_dt = DeviceBuffer.from_numpy(np.array([0.0], np.float64))
        d_pal, d_w = DeviceBuffer(ni * m.nb * 64), DeviceBuffer(ni * m.nm * 4)
        sa, sb = dm.out_sizes(api.OUT_SOA, ni)
        d_a, d_b = DeviceBuffer(sa), DeviceBuffer(sb)

        def frame(an):
            an.advance_device_dt(d_dt.ptr, dm)
            sk.solve_motion_set_blend_time_device(ms, ni, *an.operand_ptrs(), d_pal.ptr, dm)
            ms.blend_morphs_time_device(ni, *an.operand_ptrs(), d_w.ptr, dm)
            dm.deform_batched_raw(ni, d_w.ptr, d_pal.ptr, d_a.ptr, d_b.ptr, api.OUT_SOA, flags)

        def results():
            dm.sync()
            return (d_pal.download((ni, m.nb, 16), np.float32), d_a.download((ni, m.nv, 3), np.float32),
                    d_b.download((ni, m.nv, 3), np.float32))
        eager.set_state(dm, **start)
        want = []
        for k, dt in enumerate(dts):
            if k == 3:
                eager.request(*request, model=dm)
            d_dt.upload(np.array([dt], np.float64))
            frame(eager)
            want.append(results())
        want_state = eager.get_state(dm)
        # the run before recording, as the header requires; then back to the start
        frame(replayed)
        dm.sync()
        replayed.set_state(dm, **start)
        dm.graph_begin()
        frame(replayed)
        g = dm.graph_end()
        ar.assert_states_equal(replayed.get_state(dm), start, "recording does not run anything")
        for k, dt in enumerate(dts):
            if k == 3:
                replayed.request(*request, model=dm)
            d_dt.upload(np.array([dt], np.float64))
            for d in (d_pal, d_a, d_b):
                d.memset(0)
            d_w.memset(0xFF)
            g.launch()
            got = results()
            for what, a, b in zip(("palettes", "positions", "normals"), got, want[k]):
                gu.assert_bits_equal(a, b, f"replay {k}: {what}")
        ar.assert_states_equal(replayed.get_state(dm), want_state, "the state after six replays")
        assert len({w[1].tobytes() for w in want}) == len(dts)                    # six different frames
        replayed.close()                                                          # took part in the recording
        with pytest.raises(api.MmdxError, match="destroyed"):
            g.launch()
        g.close()
        close_all(eager, d_dt, d_pal, d_w, d_a, d_b)
    close_all(ms, sk)


@pytest.mark.gpu
def test_cpp_animator_matches_python_path(tmp_path):
    """host/motion_example.cpp --crowd ends with mmdx::Animator driving the crowd for 60 steps (a request for everybody, a faded
    one for every other instance at step 30): the same sequence from Python gives the same palettes, clock and loop count."""
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
        p.write_bytes(vmd.write_vmd(synth.make_bone_keys(bnames[k:30 + k], 13 + k, keys_per=4, span=24), [(mnames[0], 0, 0.5), (mnames[0], 19, 1.0)]))
        paths.append(str(p))
    ni, hz = 37, 60.0
    exe = build.build_host_example(name="motion_example")
    r = subprocess.run([exe, "--crowd", str(ni), str(hz), str(tmp_path / "m.pmx")] + paths, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "animated checksum=" in r.stderr, r.stdout + r.stderr
    pm = pmx.load_pmx(str(tmp_path / "m.pmx"))
    vs = [vmd.Vmd(p) for p in paths]
    bms, mms = [v.bind_bones(pm.bone_names) for v in vs], [v.bind_morphs(pm.morph_names) for v in vs]
    ms, sk = vmd.MotionSet(bms, mms), pm.skeleton()
    an = vmd.Animator(ms, ni)
    ids = np.arange(ni, dtype=np.uint32)
    an.request(ids, ids % 3)
    d_pal = DeviceBuffer(ni * nb * 64)
    for step in range(60):
        if step == 30:
            an.request(ids[::2], (ids[::2] + 1) % 3, np.full(ids[::2].size, 0.5, np.float32))
        an.advance(1.0 / hz)
        sk.solve_motion_set_blend_time_device(ms, ni, *an.operand_ptrs(), d_pal.ptr)
    pal = d_pal.download((ni, nb, 16), np.float32)
    h = 1469598103934665603
    for byte in pal.view(np.uint8).ravel().tolist():
        h = ((h ^ byte) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    st = an.get_state(names=("times_a", "loops"))
    assert st["loops"][0] >= 1                                    # clips of 24 frames at most: the first instance has wrapped
    want = "animated checksum=%016x clock[0]=%.6f loops[0]=%d" % (h, st["times_a"][0], st["loops"][0])
    assert want in r.stderr, (want, r.stderr)
    close_all(an, ms, sk, bms, mms, vs, d_pal)

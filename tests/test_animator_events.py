"""Clip markers: mmdx_event_set_* and mmdx_animator_events (include/mmdx.h).

There is no libmmd counterpart: as for the animator, the contract is the arithmetic the header states, held by three statements
that must agree bit for bit, with no tolerance anywhere --
  * csrc/events_math.hpp and csrc/events_table.hpp compiled for the host (tests/events_math_driver.cpp, a stand-alone program,
    plain and sanitized),
  * the numpy restatement tests/animator_events_ref.py, written from the header's text,
  * the gfx950 kernels (the same header compiled for the device),
and on the GPU a list the call wrote feeds an existing select call unchanged.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from simple_mmd_renderer_amd import _capi as api
from simple_mmd_renderer_amd import synth, vmd
from simple_mmd_renderer_amd.engine import DeformModel, DeviceBuffer, SocketSet
from tests import animator_events_ref as er
from tests import animator_ref as ar
from tests import test_animator as ta
from tests.test_capi_symbols import declared_symbols

ENTRY_POINTS = ("mmdx_event_set_create", "mmdx_event_set_destroy", "mmdx_event_set_get_info", "mmdx_animator_events")
ROOT = os.path.dirname(er.HERE)
INVALID, BAD_INDEX = 1, 2
U = np.uint32
GUARD = 64                                           # sentinel words in front of and behind every output
SENT = er.SENTINEL
CALLS = [(dt, dom) for dt in er.DTS for dom in (False, True)]
MASKS4 = (0xFFFFFFFF, (1 << 1) | (1 << 14) | (1 << 9), 1 << 20, 0x000000FF)      # everything; three channels; a channel no marker
#                                                                                   has; channels 0-7 (overlaps the first two)
_close = ta.close_all


@pytest.fixture(autouse=True)
def _lib(hip_lib):
    return hip_lib


def _animator(ni):
    ms = ta.scenario_set(["b0"])
    an = vmd.Animator(ms, ni, ta.rows_for_create())
    assert [r[0] for r in an.clip_table()] == er.table()["length"].tolist()
    return ms, an


def _levels(ni, seed=9):
    """mmdx_cull_bounds' out_levels: a third of the crowd culled, the others at levels 0-3."""
    rng = np.random.RandomState(seed + ni)
    return np.where(rng.rand(ni) < 0.33, er.CULLED, rng.randint(0, 4, ni)).astype(U)


# ---------------------------------------------------------------------------------------- CPU ----
def test_events_entry_points_are_declared_exported_and_bound(hip_lib):
    syms = declared_symbols()
    for name in ENTRY_POINTS:
        assert name in syms and hasattr(hip_lib, name) and name in api.SIGNATURES, name
    hdr = open(os.path.join(ROOT, "include", "mmdx.h")).read()
    for text in ("typedef struct mmdx_event_marker {", "typedef struct mmdx_event_set_desc {", "typedef struct mmdx_event_set_info {",
                 "typedef struct mmdx_events_args {", "#define MMDX_ABI_VERSION 3u", "MMDX_EVENTS_DOMINANT_SIDE = (1u << 15)",
                 "#define MMDX_EVENTS_MAX_LISTS 4", "(closed ? u <= m : u < m) && m <= v", "v <= m && (closed ? m <= u : m < u)"):
        assert text in hdr, text
    assert hdr.count("1u << 15") == 1                                     # the bit is nobody else's
    assert hip_lib.mmdx_abi_version() == 3
    assert (api.EVENTS_DOMINANT_SIDE, api.EVENTS_MAX_LISTS, er.CULLED, er.MAX_LISTS) == (1 << 15, 4, api.CULLED, 4)
    # 64-bit layouts by hand from the header
    assert C.sizeof(api.EventMarker) == 8 + 2 * 4 == er.MARKER.itemsize
    assert C.sizeof(api.EventSetDesc) == 2 * 4 + 8
    assert C.sizeof(api.EventSetInfo) == 4 * 4
    assert C.sizeof(api.EventsArgs) == 2 * 4 + 2 * 8 + 2 * 4 + 4 * 4 + 3 * 8
    assert (vmd.EventMarker, vmd.EventSetDesc, vmd.EventsArgs) == (api.EventMarker, api.EventSetDesc, api.EventsArgs)
    assert callable(vmd.Animator.events) and callable(vmd.EventSet.close)
    poser = open(os.path.join(ROOT, "simple_mmd_renderer_amd", "host", "mmdx_poser.hpp")).read()
    for text in ("class EventSet", "mmdx_event_set_create(", "mmdx_event_set_destroy(", "mmdx_animator_events(", "void Animator::Events("):
        assert text in poser, text
    bench = open(os.path.join(ROOT, "include", "mmdx_bench.h")).read()
    assert "mmdx_event_set" not in bench and "mmdx_animator_events" not in bench


def test_event_set_create_refuses_bad_markers_and_reports_itself(hip_lib):
    ms, an = _animator(3)
    err = lambda: (hip_lib.mmdx_last_error_string() or b"").decode()          # noqa: E731
    out = C.c_void_p()
    keep = []

    def create(rows, animator=an.h, struct_size=None, n=None, null_markers=False, out_ptr=C.byref(out)):
        m = er.markers_of(rows)
        keep.append(m)
        d = api.EventSetDesc(C.sizeof(api.EventSetDesc) if struct_size is None else struct_size, len(rows) if n is None else n,
                             None if null_markers or not len(rows) else m.ctypes.data)
        return hip_lib.mmdx_event_set_create(animator, C.byref(d), out_ptr)
    good = [(0.5, 0, 1)]
    assert create(good, out_ptr=None) == INVALID and "NULL" in err()
    assert create(good, animator=None) == INVALID and "NULL" in err()
    assert hip_lib.mmdx_event_set_create(an.h, None, C.byref(out)) == INVALID and "NULL" in err()
    assert create(good, null_markers=True) == INVALID and "markers is NULL" in err()
    assert create(good, struct_size=12) == INVALID and "struct_size" in err()
    assert create([(0.5, 7, 1)]) == BAD_INDEX and "clip = 7" in err()
    assert create([(0.5, er.NONE, 1)]) == BAD_INDEX
    assert create([(0.5, 0, 32)]) == INVALID and "channel = 32" in err()
    for t, c in ((float("nan"), 0), (-0.001, 0), (np.nextafter(2.0, 3.0), 0), (1.6, 2), (0.1, 1), (float("inf"), 6)):
        assert create([(0.25, 0, 0), (t, c, 0)]) == INVALID and "markers[1].time" in err(), (t, c)
    assert out.value is None                                               # a refusal hands out nothing
    # what is allowed: times 0 and L exactly, channel 31, duplicates, no markers at all
    sets = [vmd.EventSet(an, rows) for rows in ([], [(0.0, 0, 0), (2.0, 0, 31), (2.0, 0, 31), (0.0, 1, 5)], er.MARKERS)]
    assert [s.info() for s in sets] == [dict(n_markers=n, n_clips=7, device_ordinal=-1) for n in (0, 4, len(er.MARKERS))]
    info = api.EventSetInfo(8)
    assert hip_lib.mmdx_event_set_get_info(sets[0].h, C.byref(info)) == INVALID and "struct_size" in err()
    assert hip_lib.mmdx_event_set_get_info(None, C.byref(info)) == INVALID
    hip_lib.mmdx_event_set_destroy(None)                                   # like free(NULL)
    an.close()                                                             # the set copied what it needs
    assert sets[2].info()["n_clips"] == 7
    _close(sets, ms)


def test_animator_events_refuses_bad_arguments_before_any_device_call(hip_lib):
    """Every call here carries its defect AND a host NaN dt, the last of the checks, so none of them can reach a device; the calls
    about dt itself have nothing behind them and are the last checks by the header's order."""
    ni = 5
    ms, an = _animator(ni)
    es = vmd.EventSet(an, er.MARKERS)
    ms2 = ta.tiny_set()
    an2 = vmd.Animator(ms2, ni)                                             # another clip count
    assert an2.n_clips != an.n_clips
    err = lambda: (hip_lib.mmdx_last_error_string() or b"").decode()          # noqa: E731
    nan = C.c_double(float("nan"))
    P = 0x10000                                                            # stands for a device address; never dereferenced

    def call(animator=an.h, es_h=es.h, struct_size=None, flags=0, dt=C.addressof(nan), out_fired=P, n_lists=0, stride=ni, levels=None,
             out_ids=P + 0x1000, out_counts=P + 0x2000, null_args=False):
        a = api.EventsArgs(C.sizeof(api.EventsArgs) if struct_size is None else struct_size, flags, dt, out_fired, n_lists, stride)
        a.levels, a.out_ids, a.out_counts = levels, out_ids, out_counts
        return hip_lib.mmdx_animator_events(animator, es_h, None, None if null_args else C.byref(a))
    assert call() == INVALID and "dt is NaN" in err()                       # the guard itself
    assert call(animator=None) == INVALID and "NULL" in err()
    assert call(es_h=None) == INVALID and "NULL" in err()
    assert call(null_args=True) == INVALID and "NULL" in err()
    assert call(dt=None) == INVALID and "dt / out_fired is NULL" in err()
    assert call(out_fired=None) == INVALID and "dt / out_fired is NULL" in err()
    assert call(struct_size=C.sizeof(api.EventsArgs) - 8) == INVALID and "struct_size" in err()
    for bad in (1, 1 << 14, 1 << 16, 1 << 31):
        assert call(flags=bad) == INVALID and "unknown flag bits" in err(), bad
    assert call(flags=api.EVENTS_DOMINANT_SIDE) == INVALID and "dt is NaN" in err()      # a known bit passes on to the guard
    assert call(n_lists=5) == INVALID and "n_lists = 5" in err()
    assert call(n_lists=1, out_ids=None) == INVALID and "out_ids / out_counts is NULL" in err()
    assert call(n_lists=4, out_counts=None) == INVALID and "out_ids / out_counts is NULL" in err()
    assert call(n_lists=1, stride=ni - 1) == INVALID and "list_stride = 4" in err()
    assert call(n_lists=0, stride=0, out_ids=None, out_counts=None) == INVALID and "dt is NaN" in err()      # no lists: none of it is looked at
    assert call(out_fired=P + 2) == INVALID and "4-byte" in err()
    assert call(levels=P + 1) == INVALID and "4-byte" in err()
    assert call(n_lists=1, out_ids=P + 2) == INVALID and "4-byte" in err()
    assert call(n_lists=1, out_counts=P + 3) == INVALID and "4-byte" in err()
    assert call(animator=an2.h) == INVALID and "the event set has 7 clips" in err()
    assert call(flags=vmd.ANIM_DT_ON_DEVICE, dt=P + 4) == INVALID and "8-byte" in err()
    with pytest.raises(ValueError):
        an.events(es, P)
    with pytest.raises(ValueError):
        an.events(es, P, dt=0.1, dt_ptr=P)
    with pytest.raises(api.MmdxError, match="dt is NaN"):
        an.events(es, P, dt=float("nan"), lists=(MASKS4, ni, P, P), levels_ptr=P, dominant=True)
    _close(es, an, an2, ms, ms2)


def _reference_calls(state, masks=(), levels=None):
    t, markers = er.table(), er.markers_of(er.MARKERS)
    out, cases = [], {}
    for dt, dom in CALLS:
        f, c = er.fired(state, t, markers, dt, dom)
        for k, v in c.items():
            cases[k] = cases.get(k, 0) + int(v.sum())
        ids, counts = er.lists_of(f, masks, levels, prefill=0xFFFFFFFF)
        out.append((f, counts, ids))
    return out, cases


def test_case_table_contains_every_case_the_header_names():
    """From the numpy side alone: what the driver and the kernels are about to be compared on."""
    state = er.case_table()
    _, cases = _reference_calls(state)
    assert sorted(cases) == sorted(er.CASES)
    missing = [k for k in er.CASES if cases[k] < 1]
    assert not missing, missing
    s, first = er.sort_markers(er.markers_of(er.MARKERS), 7)
    assert first[5] - first[4] == 0 and first[1] - first[0] == 7           # a clip without markers; clip 0 with its duplicates


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_host_build_of_the_arithmetic_equals_the_numpy_restatement(sanitize):
    state = er.case_table()
    ni = state["speed"].size
    levels = _levels(ni)
    want, _ = _reference_calls(state, MASKS4, levels)
    t, markers = er.table(), er.markers_of(er.MARKERS)
    s, first, got = er.run_driver(er.build_driver(sanitize), t, markers, state, [c[0] for c in CALLS], [c[1] for c in CALLS], MASKS4, levels)
    ws, wfirst = er.sort_markers(markers, 7)
    assert s.tobytes() == ws.tobytes() and first.tolist() == wfirst.tolist()
    for (dt, dom), (gf, gc, gl), (wf, wc, wl) in zip(CALLS, got, want):
        bad = np.flatnonzero(gf != wf)
        assert not bad.size, (dt, dom, bad[:5].tolist(), {k: state[k][bad[0]] for k, _ in er.STATE}, hex(gf[bad[0]]), hex(wf[bad[0]]))
        assert gc.tolist() == wc.tolist(), (dt, dom)
        assert np.array_equal(gl, wl), (dt, dom)
    assert any(wf.any() for wf, _, _ in want) and int(want[0][1][1]) > 0 and int(want[0][1][2]) == 0
    # without lists and levels the driver reads neither
    _, _, bare = er.run_driver(er.build_driver(sanitize), t, markers, state, [er.DT], [0])
    assert np.array_equal(bare[0][0], want[0][0]) and not bare[0][1].any()


def test_the_set_stores_markers_sorted_by_clip_then_time_behind_an_offset_table():
    """The table the driver prints is events_table.hpp's, the lines mmdx_event_set_create runs."""
    rng = np.random.RandomState(12)
    n, nc = 300, 7
    t = er.table()
    m = np.zeros(n, er.MARKER)
    m["clip"] = rng.choice([0, 2, 3, 5, 6], n)                              # clips 1 and 4 stay empty
    m["time"] = np.round(rng.uniform(0, 1, n) * 8) / 8 * t["length"][m["clip"]]      # many equal times
    m["channel"] = rng.randint(0, 32, n)
    state = {k: v[:1] for k, v in er.case_table().items()}
    s, first, _ = er.run_driver(er.build_driver(), t, m, state, [], [])
    assert first[0] == 0 and first[-1] == n and (np.diff(first.astype(np.int64)) >= 0).all()
    for c in range(nc):
        mine = s[first[c]:first[c + 1]]
        assert (mine["clip"] == c).all() and (np.diff(mine["time"]) >= 0).all()
        given = m[m["clip"] == c]
        for time in np.unique(given["time"]):                              # equal times keep the order given
            assert mine["channel"][mine["time"] == time].tolist() == given["channel"][given["time"] == time].tolist()
    assert first[2] - first[1] == 0 and first[5] - first[4] == 0
    ws, wfirst = er.sort_markers(m, nc)
    assert s.tobytes() == ws.tobytes() and first.tolist() == wfirst.tolist()


def _telescoping(fires, loops0, loops1, t_start, t_end, m):
    return fires == (loops1.astype(np.int64) - loops0.astype(np.int64)) + (t_end >= m).astype(np.int64) - (t_start >= m).astype(np.int64)


def test_fires_telescope_over_many_steps():
    """A looping clip with one marker at m, steps 0 < s < L: over N steps the fires are the loops plus [t_end >= m] - [t_start >= m]
    -- no marker is lost or counted twice, at the seam (m = 0 and m = L) or anywhere else."""
    t = er.table()
    rng = np.random.RandomState(21)
    ni, n_steps = 64, 300
    for clip, length in ((0, 2.0), (6, 0.4)):
        for m in (0.0, length, length / 4, 0.1, rng.uniform(0, length)):
            markers = er.markers_of([(m, clip, 3)])
            s = ar.initial_state(ni)
            s["clips_a"][:] = clip
            s["times_a"][:] = rng.uniform(0, length * 0.999, ni)
            s["times_a"][:4] = (0.0, m if m < length else 0.0, length / 2, np.nextafter(length, 0))
            s["speed"][:] = rng.uniform(0.05, 1.0, ni).astype(np.float32)
            start = s
            fires = np.zeros(ni, np.int64)
            for _ in range(n_steps):
                dt = rng.uniform(0.01, 0.95) * length                       # speed <= 1: 0 < s < L
                f, _ = er.fired(s, t, markers, dt)
                assert not (f & ~U(8)).any()
                fires += (f != 0)
                s, _ = ar.advance(s, t, dt)
            ok = _telescoping(fires, start["loops"], s["loops"], start["times_a"], s["times_a"], m)
            assert ok.all(), (clip, m, np.flatnonzero(~ok)[:5])
            assert fires.min() >= 2


def test_kernel_resources_no_spills_no_scratch():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), api.LIB_PATH, "events"],
                         capture_output=True, text=True, check=True).stdout.splitlines()
    names = {l.split(" vgpr ")[0].strip() for l in out}
    assert names == {"animator_events_kernel<true>", "animator_events_kernel<false>", "events_scatter_kernel"}
    for l in out:
        f = l.split(" vgpr ")[1].split()
        res = dict(zip(["vgpr"] + f[1::2], (int(v) for v in f[0::2])))
        assert res["spill"] == 0 and res["scratch"] == 0 and res["vgpr"] <= 64, l
        # the wave counts and nothing else: 16 waves x 4 lists x 4 bytes where lists are made
        assert res["lds"] == (0 if "<false>" in l else 256), l


# ---------------------------------------------------------------------------------------- GPU ----
class Guarded:
    """n u32 words of device memory prefilled with the sentinel, GUARD sentinel words on both sides."""

    def __init__(self, n):
        self.n = n
        self.buf = DeviceBuffer((n + 2 * GUARD) * 4)
        self.ptr = self.buf.ptr + GUARD * 4
        self.fill()

    def fill(self):
        self.buf.upload(np.full(self.n + 2 * GUARD, SENT, U))

    def read(self, what):
        a = self.buf.download((self.n + 2 * GUARD,), U)
        assert (a[:GUARD] == SENT).all() and (a[GUARD + self.n:] == SENT).all(), what + ": a guard word changed"
        return a[GUARD:GUARD + self.n]

    def close(self):
        self.buf.free()


def _poke(an, state):
    """The seven arrays through their device addresses: ids outside the table and NaN clocks are what an adopter's own kernel may
    leave there, and mmdx_animator_set_state would refuse them."""
    addr = an.device_arrays()
    for k, ty in er.STATE:
        a = np.ascontiguousarray(state[k], ty)
        raw = DeviceBuffer.adopt(addr[k], a.nbytes)
        raw.upload(a)
        raw.ptr = None


def _run_and_compare(an, es, state, ni, dt, dom, masks, levels, stride, device_dt, outs, model=None, what=""):
    d_fired, d_ids, d_counts, d_dt, d_levels = outs
    t, markers = er.table(), er.markers_of(er.MARKERS)
    for g in (d_fired, d_ids, d_counts):
        g.fill()
    if levels is not None:
        d_levels.upload(levels)
    lists = (masks, stride, d_ids.ptr, d_counts.ptr) if masks else None
    kw = dict(lists=lists, levels_ptr=d_levels.ptr if levels is not None else None, dominant=dom, model=model)
    if device_dt:
        d_dt.upload(np.array([dt], np.float64))
        an.events(es, d_fired.ptr, dt_ptr=d_dt.ptr, **kw)
    else:
        an.events(es, d_fired.ptr, dt=dt, **kw)
    want, _ = er.fired(state, t, markers, dt, dom)
    got = d_fired.read(what + ": out_fired")
    bad = np.flatnonzero(got != want)
    assert not bad.size, (what, bad[:5].tolist(), hex(got[bad[0]]), hex(want[bad[0]]))
    ids, counts = d_ids.read(what + ": out_ids"), d_counts.read(what + ": out_counts")
    if masks:
        wids, wcounts = er.lists_of(want, masks, levels, stride)
        assert counts.tolist() == wcounts.tolist(), what
        assert np.array_equal(ids[:len(masks) * stride].reshape(len(masks), stride), wids), what      # the sentinel behind every count
        assert (ids[len(masks) * stride:] == SENT).all(), what
    else:
        assert (ids == SENT).all() and (counts == SENT).all(), what
    return want


def _outputs(ni):
    return Guarded(ni), Guarded(4 * (ni + 3)), Guarded(4), DeviceBuffer(8), DeviceBuffer(ni * 4)


@pytest.mark.gpu
@pytest.mark.parametrize("ni", [1, 63, 64, 65, 255, 256, 257, 1025])
def test_gpu_masks_lists_and_counts_equal_the_restatement(ni):
    """The case table, tiled so that the lanes of a wave sit in different cases: host and device dt, 0, 1 and 4 lists with
    overlapping masks and one that nothing matches, levels with culled rows, both flags, strides of NI and more; then a device NaN
    dt.  Every output between guard words, prefilled; the animator's arrays keep their bytes through all of it."""
    state = er.tiled(er.case_table(), ni)
    ms, an = _animator(ni)
    es = vmd.EventSet(an, er.MARKERS)
    _poke(an, state)
    before = an.get_state()
    outs = _outputs(ni)
    levels = _levels(ni)
    assert ni < 8 or (levels == er.CULLED).any()
    fired_any = 0
    plans = [(er.DT, False, (), None, ni, False), (er.DT, False, MASKS4, None, ni + 3, True), (-0.125, True, MASKS4[:1], levels, ni, False),
             (1 / 60, True, MASKS4, levels, ni, True), (0.0, False, MASKS4, None, ni, False), (er.DT, True, MASKS4[1:2], levels, ni + 1, True)]
    for dt, dom, masks, lv, stride, device_dt in plans:
        want = _run_and_compare(an, es, state, ni, dt, dom, masks, lv, stride, device_dt, outs,
                                what=f"NI {ni}, dt {dt}, dominant {dom}, {len(masks)} lists")
        fired_any += int((want != 0).sum())
    assert fired_any >= (1 if ni >= 63 else 0)
    # a device NaN dt: all masks 0, all counts 0, the lists untouched
    d_fired, d_ids, d_counts, d_dt, _ = outs
    for g in (d_fired, d_ids, d_counts):
        g.fill()
    d_dt.upload(np.array([np.nan], np.float64))
    an.events(es, d_fired.ptr, dt_ptr=d_dt.ptr, lists=(MASKS4, ni, d_ids.ptr, d_counts.ptr))
    assert not d_fired.read("NaN dt").any() and not d_counts.read("NaN dt").any() and (d_ids.read("NaN dt") == SENT).all()
    with pytest.raises(api.MmdxError, match="dt is NaN"):
        an.events(es, d_fired.ptr, dt=float("nan"))
    ar.assert_states_equal(dict(an.get_state()), before, "the animator's arrays after every call")
    assert es.info()["device_ordinal"] >= 0
    _close(es, an, ms, list(outs))


@pytest.mark.gpu
@pytest.mark.parametrize("chunk", ["64", "100", "1024", "5000"])
def test_gpu_chunk_override(chunk, monkeypatch):
    """200 instances: MMDX_EVENTS_CHUNK=64 makes four chunks, the last one partial; 100 rounds down to 64; 1 024 and 5 000 (clamped)
    make one partial chunk.  Read per call."""
    ni = 200
    state = er.tiled(er.case_table(), ni, seed=4)
    ms, an = _animator(ni)
    es = vmd.EventSet(an, er.MARKERS)
    _poke(an, state)
    outs = _outputs(ni)
    levels = _levels(ni)
    monkeypatch.setenv("MMDX_EVENTS_CHUNK", chunk)
    want = _run_and_compare(an, es, state, ni, er.DT, False, MASKS4, levels, ni, True, outs, what=f"chunk {chunk}")
    assert (want != 0).sum() > 20
    _run_and_compare(an, es, state, ni, -0.125, True, MASKS4[:2], None, ni + 2, False, outs, what=f"chunk {chunk}, backwards")
    monkeypatch.delenv("MMDX_EVENTS_CHUNK")
    _run_and_compare(an, es, state, ni, er.DT, False, MASKS4, levels, ni, True, outs, what="the default chunk again")
    _close(es, an, ms, list(outs))


@pytest.mark.gpu
def test_gpu_everybody_fires_count_equals_stride():
    ni = 257
    ms, an = _animator(ni)
    es = vmd.EventSet(an, er.MARKERS)
    s = ar.initial_state(ni)
    s["clips_a"][:], s["times_a"][:] = 6, 0.05
    an.set_state(**s)
    outs = _outputs(ni)
    want = _run_and_compare(an, es, {k: s[k] for k, _ in er.STATE}, ni, er.DT, False, (1 << 14, 1 << 20), None, ni, False, outs, what="all fire")
    assert (want & (1 << 14)).all()
    assert outs[2].read("counts").tolist() == [ni, 0, 0, 0]
    assert outs[1].read("ids")[:ni].tolist() == list(range(ni))
    # an empty set: nothing ever fires
    none = vmd.EventSet(an, [])
    outs[0].fill()
    an.events(none, outs[0].ptr, dt=er.DT, lists=((0xFFFFFFFF,), ni, outs[1].ptr, outs[2].ptr))
    assert not outs[0].read("an empty set").any() and not outs[2].read("an empty set").any()
    _close(es, none, an, ms, list(outs))


@pytest.mark.gpu
def test_gpu_graph_of_events_and_advance_replayed_with_a_new_dt():
    """[events, advance] with a device dt recorded once, replayed 40 times with 8 bytes rewritten: every replay against numpy
    stepping the same state; the telescoping identity on the loops and clocks the library itself reports."""
    ni, n_replays = 65, 40
    t, markers = er.table(), er.markers_of(er.MARKERS)
    rng = np.random.RandomState(33)
    start = ar.initial_state(ni)
    start["clips_a"][:] = np.where(np.arange(ni) % 2, 6, 0)
    start["times_a"][:] = rng.uniform(0, 0.39, ni)
    start["speed"][:] = rng.uniform(0.25, 2.0, ni).astype(np.float32)
    start["clips_a"][60:] = (2, 3, 5, er.NONE, 4)                              # a HOLD, THEN chains, nothing, a clip without markers
    dts = rng.uniform(1 / 144, 1 / 30, n_replays)
    dts[7] = np.nan                                                           # a NaN frame in the middle: nothing fires, nothing moves
    with DeformModel(synth.make_model(64, 4, 0, 0, seed=2)) as dm:
        ms, an = _animator(ni)
        es = vmd.EventSet(an, er.MARKERS)
        d_fired, d_ids, d_counts, d_dt, _ = outs = _outputs(ni)

        def frame():
            an.events(es, d_fired.ptr, dt_ptr=d_dt.ptr, lists=(MASKS4, ni, d_ids.ptr, d_counts.ptr), model=dm)
            an.advance_device_dt(d_dt.ptr, dm)
        an.set_state(dm, **start)
        d_dt.upload(np.array([0.0], np.float64))
        frame()                                                               # the run before recording (dt = 0 moves nothing)
        dm.sync()
        an.set_state(dm, **start)
        for g in (d_fired, d_ids, d_counts):
            g.fill()
        dm.graph_begin()
        frame()
        g = dm.graph_end()
        dm.sync()
        ar.assert_states_equal(an.get_state(dm), start, "recording does not run anything")
        assert (d_fired.read("recording") == SENT).all() and (d_counts.read("recording") == SENT).all()
        s = start
        fires14, fires3 = np.zeros(ni, np.int64), np.zeros(ni, np.int64)
        for k, dt in enumerate(dts):
            d_dt.upload(np.array([dt], np.float64))
            d_ids.fill()
            g.launch()
            dm.sync()
            want, _ = er.fired(s, t, markers, dt)
            wids, wcounts = er.lists_of(want, MASKS4)
            got = d_fired.read(f"replay {k}")
            assert np.array_equal(got, want), (k, dt)
            assert d_counts.read(f"replay {k}").tolist() == wcounts.tolist(), k
            assert np.array_equal(d_ids.read(f"replay {k}")[:4 * ni].reshape(4, ni), wids), k
            fires14 += (got >> 14) & 1
            fires3 += (got >> 3) & 1
            s, _ = ar.advance(s, t, dt)
            ar.assert_states_equal(an.get_state(dm), s, f"the state after replay {k}")
        assert not er.fired(start, t, markers, np.nan)[0].any()
        end = an.get_state(dm)
        on6, on0 = np.flatnonzero(start["clips_a"] == 6), np.flatnonzero(start["clips_a"] == 0)
        for rows, fires, m in ((on6, fires14, 0.1), (on0, fires3, 1.0)):
            ok = _telescoping(fires[rows], start["loops"][rows], end["loops"][rows], start["times_a"][rows], end["times_a"][rows], m)
            assert ok.all(), (m, rows[~ok][:5])
        assert fires14[on6].sum() > 40 and end["loops"][on6].sum() > 30
        es.close()                                                            # took part in the recording
        with pytest.raises(api.MmdxError, match="destroyed"):
            g.launch()
        g.close()
        _close(an, ms, list(outs))


@pytest.mark.gpu
def test_gpu_list_0_feeds_palette_sockets_as_it_is():
    """events -> list 0 and its count, unchanged, as the mmdx_instance_select of mmdx_palette_sockets: exactly the listed rows are
    written."""
    ni, nb = 65, 6
    state = er.tiled(er.case_table(), ni, seed=8)
    rng = np.random.RandomState(2)
    with DeformModel(synth.make_model(64, nb, 0, 0, seed=5)) as dm:
        ms, an = _animator(ni)
        es = vmd.EventSet(an, er.MARKERS)
        _poke(an, state)
        outs = _outputs(ni)
        mask = (1 << 1) | (1 << 3) | (1 << 14) | (1 << 8)
        want = _run_and_compare(an, es, state, ni, er.DT, False, (mask,), None, ni, True, outs, model=dm, what="foot plants")
        listed = np.flatnonzero(want & mask)
        assert 3 <= listed.size < ni
        sset = SocketSet(dm, [1, 4], rng.uniform(-1, 1, (2, 3)).astype(np.float32))
        pal = rng.uniform(-2, 2, (ni, nb, 16)).astype(np.float32)
        d_pal = DeviceBuffer.from_numpy(pal)
        full, some = DeviceBuffer(2 * ni * 64), DeviceBuffer(2 * ni * 64)
        some.memset(0xEE)
        sset.sockets(d_pal, full, n_instances=ni)
        sset.sockets(d_pal, some, select=vmd.instance_select(outs[1].ptr, ni, outs[2].ptr), n_instances=ni)
        dm.sync()
        a, b = full.download((2, ni, 64), np.uint8), some.download((2, ni, 64), np.uint8)
        exp = np.full_like(a, 0xEE)
        exp[:, listed] = a[:, listed]
        assert np.array_equal(b, exp)
        _close(sset, es, an, ms, list(outs), d_pal, full, some)

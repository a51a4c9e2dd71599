"""Clip markers (mmdx_animator_events, include/mmdx.h): what the tests share.

  * fired() / lists_of(): a restatement of the header's steps 1-9 in numpy -- whole arrays at a time, masks instead of branches,
    comparisons of float64 arrays.  It is written from the header's text, not from csrc/events_math.hpp; the clock of a side is
    animator_ref.wrap, the restatement of advance's wrap.  fired() also reports which of the header's cases every instance went
    through, so a test can prove its coverage;
  * sort_markers(): the (clip, time) order and the offset table the header describes;
  * case_table(): the generated state table of the CPU and GPU tests, and MARKERS, the marker set it is made for;
  * the stand-alone CPU driver of csrc/events_math.hpp (tests/events_math_driver.cpp): built with g++ at test time, plain and with
    the sanitizers, by tests/host_program.py.
"""
import os

import numpy as np

from tests import animator_ref as ar
from tests import host_program as hp

HERE = hp.TESTS
NONE, CULLED, MAX_LISTS = ar.NONE, 0xFFFFFFFF, 4
STATE = (("clips_a", np.uint32), ("clips_b", np.uint32), ("times_a", np.float64), ("times_b", np.float64),
         ("weights", np.float32), ("speed", np.float32), ("fade_rate", np.float32))      # the seven arrays the call reads
MARKER = np.dtype([("time", np.float64), ("clip", np.uint32), ("channel", np.uint32)])   # mmdx_event_marker, 16 bytes
SENTINEL = 0xA5A5A5A5


def markers_of(rows):
    """(time, clip, channel) rows -> a MARKER array."""
    m = np.zeros(len(rows), MARKER)
    for j, (t, c, ch) in enumerate(rows):
        m[j] = (t, c, ch)
    return m


def sort_markers(markers, n_clips):
    """-> (the markers sorted by (clip, time), equal ones in the order given; first[n_clips + 1])."""
    order = np.lexsort((np.arange(markers.size), markers["time"], markers["clip"]))
    s = markers[order]
    first = np.zeros(n_clips + 1, np.uint32)
    first[1:] = np.cumsum(np.bincount(s["clip"], minlength=n_clips)[:n_clips])
    return s, first


def _leg(u, v, closed, m):
    """Step 3 for whole arrays."""
    up = u <= v
    lo = np.where(closed, u <= m, u < m) & (m <= v)
    hi = (v <= m) & np.where(closed, m <= u, m < u)
    return np.where(up, lo, hi)


def _side(table, markers, clip, t0, s):
    """Steps 2, 4, 5 for whole arrays -> (masks u32, cases: name -> bool array)."""
    nc = table["length"].size
    n = clip.size
    has = clip < nc
    row = np.where(has, clip, 0)
    length, mode = table["length"][row], table["mode"][row]
    with np.errstate(all="ignore"):
        raw = t0 + s
        t1, fold = ar.wrap(table, clip, raw)
        forwards = raw >= length
        near = np.where(forwards, length, 0.0)
        far = np.where(forwards, 0.0, length)
        nan_step = s != s
        out = np.zeros(n, np.uint32)
        at = {k: np.zeros(n, bool) for k in ("marker_at_t0", "marker_at_t1", "marker_at_0_fired", "marker_at_L_fired", "duplicate_fired")}
        seen = {}
        for time, c, ch in markers.tolist():
            mine = has & (clip == c) & ~nan_step
            one = _leg(t0, t1, False, time)
            two = _leg(t0, near, False, time) | _leg(far, t1, True, time)
            hit = mine & np.where(fold, two, one)
            out |= np.where(hit, np.uint32(1) << np.uint32(ch), np.uint32(0)).astype(np.uint32)
            at["marker_at_t0"] |= mine & (t0 == time)
            at["marker_at_t1"] |= mine & (t1 == time)
            at["marker_at_0_fired"] |= hit & (time == 0.0)
            at["marker_at_L_fired"] |= hit & (time == length) & (length > 0.0)
            if (time, c, ch) in seen:
                at["duplicate_fired"] |= hit
            seen[(time, c, ch)] = True
        marked = np.isin(clip, np.unique(markers["clip"])) if markers.size else np.zeros(n, bool)
        loop = has & (mode == ar.LOOP)
        cases = dict(at, forwards=has & (s > 0), backwards=has & (s < 0), zero_step=has & (s == 0), no_fold=has & ~fold & (s != 0) & ~nan_step,
                     fold_forwards=fold & forwards, fold_backwards=fold & ~forwards,
                     more_than_a_lap=fold & (np.abs(s) > length),
                     hold_reaches_L=has & (mode == ar.HOLD) & (t0 < length) & (t1 == length),
                     hold_sits_on_L=has & (mode == ar.HOLD) & (t0 == length) & (s > 0),
                     clamp_at_0=has & ~loop & (raw < 0.0) & (t1 == 0.0), then=has & (mode == ar.THEN) & (s != 0),
                     loop_of_length_0=loop & (length == 0.0), none=clip == NONE, out_of_range=~has & (clip != NONE),
                     clip_without_markers=has & ~marked, nan_clock=has & np.isnan(t0), inf_clock=has & np.isinf(t0), nan_step=has & nan_step,
                     clock_outside=has & ((t0 < 0.0) | (t0 > length)) & np.isfinite(t0), fired=out != 0)
    return out, cases


def fired(state, table, markers, dt, dominant=False):
    """Steps 1-6 and 9 -> (out_fired u32 [ni], cases: name -> bool [ni])."""
    with np.errstate(all="ignore"):
        s = state["speed"].astype(np.float64) * np.float64(dt)
    a, ca = _side(table, markers, state["clips_a"], state["times_a"], s)
    b, cb = _side(table, markers, state["clips_b"], state["times_b"], s)
    fading = state["fade_rate"] > np.float32(0)
    w = state["weights"]
    if dominant:
        use_b = fading & (w > np.float32(0.5))
        use_a = ~use_b
    else:
        use_a, use_b = np.ones(fading.size, bool), fading
    out = (np.where(use_a, a, 0) | np.where(use_b, b, 0)).astype(np.uint32)
    cases = {k: (ca[k] & use_a) | (cb[k] & use_b) for k in ca}
    flag = "dominant" if dominant else "both"
    cases.update({f"fading_w_below_half_{flag}": fading & (w < np.float32(0.5)), f"fading_w_half_{flag}": fading & (w == np.float32(0.5)),
                  f"fading_w_above_half_{flag}": fading & (w > np.float32(0.5)),
                  f"sides_differ_{flag}": fading & (a != b), "side_b_ignored_not_fading": ~fading & (b != 0)})
    return out, cases


def lists_of(out_fired, masks, levels=None, stride=None, prefill=SENTINEL):
    """Step 7 -> (out_ids u32 [len(masks), stride] with `prefill` behind each count, out_counts u32 [4])."""
    ni = out_fired.size
    stride = ni if stride is None else stride
    ids = np.full((len(masks), stride), prefill, np.uint32)
    counts = np.zeros(MAX_LISTS, np.uint32)
    for l, m in enumerate(masks):
        member = (out_fired & np.uint32(m)) != 0
        if levels is not None:
            member &= levels != CULLED
        got = np.flatnonzero(member).astype(np.uint32)
        ids[l, :got.size] = got
        counts[l] = got.size
    return ids, counts


# ---- the marker set and the state table -----------------------------------------------------------------------------------------
# The clips are animator_ref's scenario: 0 LOOP 2.0 s, 1 LOOP of length 0, 2 HOLD 1.5, 3 THEN 1.0, 4 THEN 0.5, 5 THEN 0.75, 6 LOOP 0.4.
# Given out of order; clip 0 has two markers at one time on different channels and one marker twice; clip 4 has none.
MARKERS = ((1.0, 0, 3), (0.75, 2, 8), (0.0, 6, 16), (0.5, 0, 1), (2.0, 0, 4), (0.3, 6, 15), (0.0, 0, 0), (0.5, 0, 2), (1.5, 2, 9),
           (0.0, 1, 6), (0.5, 3, 10), (0.75, 5, 12), (0.5, 0, 1), (0.1, 6, 14), (1.0, 3, 11), (0.0, 2, 7), (1.25, 0, 5), (0.4, 6, 31),
           (0.0, 5, 13))
DT = 0.25                                            # exact in binary: t0 = m - 0.25 lands on m
DTS = (DT, -0.125, 0.0, 1.0 / 60.0)
SPEEDS = (1.0, -1.0, 0.0, 2.0, 10.0, -10.0, float("nan"))
CASES = ("forwards", "backwards", "zero_step", "no_fold", "fold_forwards", "fold_backwards", "more_than_a_lap", "hold_reaches_L",
         "hold_sits_on_L", "clamp_at_0", "then", "loop_of_length_0", "none", "out_of_range", "marker_at_t0", "marker_at_t1",
         "marker_at_0_fired", "marker_at_L_fired", "duplicate_fired", "clip_without_markers", "nan_clock", "inf_clock", "nan_step",
         "clock_outside", "fired", "fading_w_below_half_both", "fading_w_half_both", "fading_w_above_half_both",
         "fading_w_below_half_dominant", "fading_w_half_dominant", "fading_w_above_half_dominant", "sides_differ_both",
         "sides_differ_dominant", "side_b_ignored_not_fading")


def table():
    return ar.table_of(ar.resolved_rows())


def case_table():
    """-> the state (the seven arrays, one row per case).  Side a alone: every clip (and no clip, and an id out of range) x the
    times that matter for it x every speed.  Then pairs of those sides mid-fade at weights below, at and above 0.5, and the same
    pairs with fade_rate == 0."""
    t = table()
    nc = t["length"].size
    sides = []
    for c in list(range(nc)) + [NONE, nc + 2]:
        length = float(t["length"][c]) if c < nc else 1.0
        times = {0.0, length, length - 0.1, 0.05, -0.3, length + 0.5, float("nan"), float("inf"), float("-inf")}
        for m, mc, _ in MARKERS:
            if mc == c:
                times |= {m, m - DT, m + DT, m - 0.125, m + 0.125}
        for t0 in sorted(times, key=lambda x: (x != x, x)):
            sides.append((c, t0))
    rows = [(c, t0, NONE, 0.0, 0.0, sp, 0.0) for c, t0 in sides for sp in SPEEDS]
    rng = np.random.RandomState(5)
    live = [s for s in sides if s[0] < nc and np.isfinite(s[1])]
    for k in range(240):
        (ca, ta), (cb, tb) = live[rng.randint(len(live))], live[rng.randint(len(live))]
        w = (0.25, 0.5, 0.75, 0.0, 1.0, 0.49999997)[k % 6]
        rate = (2.0, 2.0, 2.0, 0.0)[k % 4]                      # every fourth pair does not fade: side b must not fire
        rows.append((ca, ta, cb, tb, w, (1.0, -1.0, 2.0)[k % 3], rate))
    cols = dict(zip(("clips_a", "times_a", "clips_b", "times_b", "weights", "speed", "fade_rate"), zip(*rows)))
    return {k: np.array(cols[k], ty) for k, ty in STATE}


def tiled(state, ni, seed=3):
    """ni instances from the rows of a state, in a fixed shuffled order (repeated when ni is larger): neighbours are different cases."""
    n = state["speed"].size
    perm = np.random.RandomState(seed).permutation(n)
    pick = perm[np.arange(ni) % n]
    return {k: v[pick].copy() for k, v in state.items()}


# ---- the CPU driver -------------------------------------------------------------------------------------------------------------
def build_driver(sanitize=False):
    return hp.build("events_math_driver", [os.path.join(HERE, "events_math_driver.cpp")], sanitize=sanitize)


def run_driver(exe, t, markers, state, dts, dominant, masks=(), levels=None):
    """-> (sorted markers, first, per call: (fired, counts, lists [4, ni] with 0xFFFFFFFF behind a count))."""
    ni, nc = state["speed"].size, t["length"].size

    def write(f):
        np.array([ni, nc, markers.size, len(dts), len(masks), levels is not None], np.uint32).tofile(f)
        for k in ("length", "mode", "next", "fade"):
            t[k].tofile(f)
        markers.tofile(f)
        for k, ty in STATE:
            np.ascontiguousarray(state[k], ty).tofile(f)
        np.asarray(dts, np.float64).tofile(f)
        np.asarray(dominant, np.uint32).tofile(f)
        np.array(list(masks) + [0] * (MAX_LISTS - len(masks)), np.uint32).tofile(f)
        if levels is not None:
            np.ascontiguousarray(levels, np.uint32).tofile(f)

    def read(f):
        s = np.fromfile(f, MARKER, markers.size)
        first = np.fromfile(f, np.uint32, nc + 1)
        return s, first, [(np.fromfile(f, np.uint32, ni), np.fromfile(f, np.uint32, MAX_LISTS),
                           np.fromfile(f, np.uint32, MAX_LISTS * ni).reshape(MAX_LISTS, ni)) for _ in dts]
    return hp.run_files(exe, write, read)

"""The crowd animator (mmdx_animator_advance, include/mmdx.h): what the tests share.

  * advance(): a restatement of the step in numpy -- whole arrays at a time, masks instead of branches, float32 / float64 array
    arithmetic (every numpy operation is one IEEE rounding, nothing is fused).  It is written from the header's text, not from
    csrc/anim_math.hpp, and reports which of the header's cases every instance went through, so a test can prove its coverage;
  * sweep(): the seeded scenario of the CPU and GPU tests -- a clip table with every mode, a crowd with every kind of start, a dt
    per step and the requests that arrive before each step;
  * the stand-alone CPU driver of csrc/anim_math.hpp (tests/anim_math_driver.cpp): built with g++ at test time, plain and with
    the sanitizers, by tests/host_program.py.
"""
import os

import numpy as np

from tests import host_program as hp

HERE = hp.TESTS
NONE, NO_REQUEST = 0xFFFFFFFF, 0xFFFFFFFE           # MMDX_CLIP_NONE, MMDX_ANIM_NO_REQUEST
LOOP, HOLD, THEN = 0, 1, 2                          # MMDX_ANIM_*
ARRAYS = (("clips_a", np.uint32), ("clips_b", np.uint32), ("times_a", np.float64), ("times_b", np.float64),
          ("weights", np.float32), ("speed", np.float32), ("fade_rate", np.float32), ("req_clip", np.uint32),
          ("req_fade", np.float32), ("req_time", np.float64), ("loops", np.uint32))      # the order of mmdx_animator_arrays
ROW_IS_B = np.float32(1.0) - np.float32(1e-7)       # the blend's threshold, a float subtraction


def initial_state(ni):
    """What mmdx_animator_create leaves: nothing plays, speed 1, no request."""
    s = {k: np.zeros(ni, t) for k, t in ARRAYS}
    s["clips_a"][:] = NONE
    s["clips_b"][:] = NONE
    s["speed"][:] = 1.0
    s["req_clip"][:] = NO_REQUEST
    return s


def table_of(rows):
    """rows: (length seconds, mode, next, fade) per clip -> the table as arrays."""
    return dict(length=np.array([r[0] for r in rows], np.float64), mode=np.array([r[1] for r in rows], np.uint32),
                next=np.array([r[2] for r in rows], np.uint32), fade=np.array([r[3] for r in rows], np.float32))


def _clamp(t, length):
    return np.where(t > length, length, np.where(t >= 0.0, t, 0.0))


def wrap(table, clip, t):
    """wrap(c, t) of the header for whole arrays -> (new clocks, which of them folded)."""
    nc = table["length"].size
    has = clip < nc
    row = np.where(has, clip, 0)
    length, loops = table["length"][row], table["mode"][row] == LOOP
    fold = has & loops & (length > 0.0) & ((t < 0.0) | (t >= length))
    safe = np.where(length > 0.0, length, 1.0)                  # lanes that do not fold: any divisor, the quotient is dropped
    folded = _clamp(t - np.floor(t / safe) * safe, length)
    out = np.where(fold, folded, t)                              # LOOP inside [0, L): unchanged
    out = np.where(has & loops & ~(length > 0.0), 0.0, out)
    out = np.where(has & ~loops, _clamp(t, length), out)
    return out, fold


def advance(state, table, dt):
    """One step -> (the new state, events: name -> bool [ni]).  `state` is not modified."""
    s = {k: v.copy() for k, v in state.items()}
    ni = s["loops"].size
    ev = {k: np.zeros(ni, bool) for k in ("fold", "fading", "promote", "request", "request_waits", "then", "then_none", "at_once",
                                         "fade_started", "promote_and_go", "on_length")}
    if dt != dt:
        return s, ev
    nc = table["length"].size
    with np.errstate(all="ignore"):
        step = s["speed"].astype(np.float64) * np.float64(dt)
        s["times_a"], ev["fold"] = wrap(table, s["clips_a"], s["times_a"] + step)
        s["loops"] = s["loops"] + ev["fold"].astype(np.uint32)
        fading = s["fade_rate"] > np.float32(0)
        ev["fading"] = fading
        ev["request_waits"] = fading & (s["req_clip"] != NO_REQUEST)
        tb, _ = wrap(table, s["clips_b"], s["times_b"] + step)
        s["times_b"] = np.where(fading, tb, s["times_b"])
        w = s["weights"] + np.float32(dt) * s["fade_rate"]
        w = np.where(w >= np.float32(0), w, np.float32(0))
        s["weights"] = np.where(fading, w, s["weights"]).astype(np.float32)
        promote = fading & (s["weights"] > ROW_IS_B)
        ev["promote"] = promote
        s["clips_a"] = np.where(promote, s["clips_b"], s["clips_a"])
        s["times_a"] = np.where(promote, s["times_b"], s["times_a"])
        s["clips_b"] = np.where(promote, np.uint32(NONE), s["clips_b"])
        s["times_b"] = np.where(promote, 0.0, s["times_b"])
        s["weights"] = np.where(promote, np.float32(0), s["weights"])
        s["fade_rate"] = np.where(promote, np.float32(0), s["fade_rate"])
        idle = s["fade_rate"] == np.float32(0)
        request = idle & (s["req_clip"] != NO_REQUEST)
        has = s["clips_a"] < nc
        row = np.where(has, s["clips_a"], 0)
        then = (idle & ~request & has & (table["mode"][row] == THEN) &
                (s["times_a"] >= table["length"][row] - table["fade"][row].astype(np.float64)))
        go = request | then
        clip = np.where(request, s["req_clip"], table["next"][row])
        fade = np.where(request, s["req_fade"], table["fade"][row]).astype(np.float32)
        start = np.where(request, s["req_time"], 0.0)
        soft = go & (fade > np.float32(0))
        hard = go & ~soft
        ev.update(request=request, then=then, then_none=then & (clip == NONE), at_once=hard, fade_started=soft, promote_and_go=promote & go)
        s["clips_a"] = np.where(hard, clip, s["clips_a"])
        s["times_a"] = np.where(hard, start, s["times_a"])
        s["clips_b"] = np.where(soft, clip, s["clips_b"])
        s["times_b"] = np.where(soft, start, s["times_b"])
        s["weights"] = np.where(soft, np.float32(0), s["weights"])
        s["fade_rate"] = np.where(soft, np.float32(1) / np.where(soft, fade, np.float32(1)), s["fade_rate"])
        s["req_clip"] = np.where(go, np.uint32(NO_REQUEST), s["req_clip"])
        has = s["clips_a"] < nc
        ev["on_length"] = has & (s["times_a"] == table["length"][np.where(has, s["clips_a"], 0)]) & (s["times_a"] > 0.0)
    return {k: s[k].astype(t) for k, t in ARRAYS}, ev


def apply_requests(state, ids, clips, fades, times):
    """mmdx_animator_request: the scatter; an id >= ni is skipped.  In place."""
    ni = state["loops"].size
    for i, c, f, t in zip(ids, clips, fades, times):
        if i < ni:
            state["req_clip"][i], state["req_fade"][i], state["req_time"][i] = c, f, t


# ---- the scenario ---------------------------------------------------------------------------------------------------------------
CLIP_FRAMES = (60, 0, 45, 30, 15, 23, 15)           # the last key frame of the seven clips of the scenario's motion set
STEP = 1.0 / 60.0
# clip 0 loops over its own length (2 s), 1 has length 0, 2 holds, 3 fades to 0 over many steps, 4 ends in the rest pose at once,
# 5 fades to 2 in less than a step, 6 is a short loop with a stated length
CLIP_ROWS = ((0.0, LOOP, NONE, 0.0), (0.0, LOOP, NONE, 0.0), (1.5, HOLD, NONE, 0.0), (0.0, THEN, 0, 0.25), (0.0, THEN, NONE, 0.0),
             (0.75, THEN, 2, 0.01), (0.4, LOOP, NONE, 0.0))
DTS = (STEP, 1.0 / 144.0, 1.0 / 30.0, 0.0, STEP, 7.0, STEP, -STEP, STEP, 1.0 / 30.0)     # 7.0 = 3.5 lengths of clip 0
SPEEDS = (1.0, 0.5, -1.0, 0.0)
FADES = (0.0, 0.005, 0.3)                           # at once, shorter than one step, many steps


def resolved_rows(rows=CLIP_ROWS, frames=CLIP_FRAMES):
    """The table as mmdx_animator_create resolves it: a length <= 0 is the clip's own, double(last_frame) / 30.0."""
    return [(l if l > 0 else np.float64(f) / np.float64(30.0), m, n, fd) for (l, m, n, fd), f in zip(rows, frames)]


def sweep(ni, n_steps, seed=7):
    """-> (table, initial state, dt per step, requests per step: (ids, clips, fades, times))."""
    rng = np.random.RandomState(seed + ni)
    table = table_of(resolved_rows())
    nc = len(CLIP_ROWS)
    s = initial_state(ni)
    pick = lambda: np.where(rng.rand(ni) < 0.15, NONE, rng.randint(0, nc, ni)).astype(np.uint32)      # noqa: E731
    s["clips_a"], s["clips_b"] = pick(), pick()
    s["times_a"], s["times_b"] = rng.uniform(-0.1, 2.2, ni), rng.uniform(0.0, 1.0, ni)
    fading = rng.rand(ni) < 0.3
    s["weights"] = np.where(fading, rng.uniform(0, 0.9, ni), 0).astype(np.float32)
    s["fade_rate"] = np.where(fading, rng.choice([0.5, 3.0, 200.0], ni), 0).astype(np.float32)
    s["clips_b"] = np.where(fading, s["clips_b"], NONE).astype(np.uint32)
    s["times_b"] = np.where(fading, s["times_b"], 0.0)
    s["speed"] = np.asarray(SPEEDS, np.float32)[rng.randint(0, len(SPEEDS), ni)]
    if ni >= 8:                                      # the corners by hand, whatever the seed gives the rest
        s["clips_a"][0], s["clips_b"][0], s["fade_rate"][0], s["weights"][0] = NONE, NONE, 0, 0                 # nothing plays
        s["clips_a"][1], s["clips_b"][1], s["fade_rate"][1], s["weights"][1] = NONE, 0, 3.0, 0.1                # rest -> clip
        s["clips_a"][2], s["clips_b"][2], s["fade_rate"][2], s["weights"][2] = 0, NONE, 3.0, 0.1                # clip -> rest
        s["clips_a"][3], s["clips_b"][3], s["fade_rate"][3], s["weights"][3] = NONE, NONE, 3.0, 0.1             # rest -> rest
        s["clips_a"][4], s["times_a"][4], s["speed"][4], s["fade_rate"][4] = 2, 1.5 - 3 * STEP, 1.0, 0          # HOLD lands on L
        s["clips_a"][5], s["times_a"][5], s["speed"][5], s["fade_rate"][5] = 4, 0.0, 1.0, 0                     # THEN -> NONE
        s["clips_a"][6], s["times_a"][6], s["speed"][6], s["fade_rate"][6] = 1, 0.3, 1.0, 0                     # a clip of length 0
        s["clips_a"][7], s["times_a"][7], s["speed"][7], s["fade_rate"][7] = 5, 0.0, 1.0, 0                     # a fade inside one step
    dts = np.array([DTS[k % len(DTS)] for k in range(n_steps)], np.float64)
    requests = []
    for k in range(n_steps):
        n = rng.randint(0, max(2, ni // 6)) if k % 3 else 0
        ids = rng.choice(ni, min(n, ni), replace=False).astype(np.uint32)
        clips = np.where(rng.rand(ids.size) < 0.2, NONE, rng.randint(0, nc, ids.size)).astype(np.uint32)
        fades = np.asarray(FADES, np.float32)[rng.randint(0, len(FADES), ids.size)]
        times = np.asarray([0.0, 0.1], np.float64)[rng.randint(0, 2, ids.size)]
        requests.append((ids, clips, fades, times))
    return table, s, dts, requests


def run_reference(table, state, dts, requests):
    """-> (the state after every step, the events of every step)."""
    states, events = [], []
    s = state
    for dt, req in zip(dts, requests):
        s = {k: v.copy() for k, v in s.items()}                  # the state stored for the previous step stays as it was
        apply_requests(s, *req)
        s, ev = advance(s, table, dt)
        states.append(s)
        events.append(ev)
    return states, events


# ---- the CPU driver -------------------------------------------------------------------------------------------------------------
def build_driver(sanitize=False):
    return hp.build("anim_math_driver", [os.path.join(HERE, "anim_math_driver.cpp")], sanitize=sanitize)


def run_driver(exe, table, state, dts, requests):
    """The stand-alone program over the same scenario -> the state after every step."""
    ni, nc = state["loops"].size, table["length"].size
    flat = [(np.full(len(r[0]), k, np.uint32),) + tuple(r) for k, r in enumerate(requests)]
    cat = lambda j, t: np.concatenate([f[j] for f in flat]).astype(t) if flat else np.zeros(0, t)      # noqa: E731
    r_step, r_id, r_clip, r_fade, r_time = cat(0, np.uint32), cat(1, np.uint32), cat(2, np.uint32), cat(3, np.float32), cat(4, np.float64)

    def write(f):
        np.array([ni, nc, len(dts), r_step.size], np.uint32).tofile(f)
        for k in ("length", "mode", "next", "fade"):
            table[k].tofile(f)
        for k, t in ARRAYS:
            np.ascontiguousarray(state[k], t).tofile(f)
        np.ascontiguousarray(dts, np.float64).tofile(f)
        for a in (r_step, r_id, r_clip, r_fade, r_time):
            a.tofile(f)
    return hp.run_files(exe, write, lambda f: [{k: np.fromfile(f, t, ni) for k, t in ARRAYS} for _ in dts])


def assert_states_equal(got, want, what):
    """Every array, as bit patterns."""
    for k, t in ARRAYS:
        bits = np.uint64 if np.dtype(t).itemsize == 8 else np.uint32
        a, b = np.ascontiguousarray(got[k], t).view(bits), np.ascontiguousarray(want[k], t).view(bits)
        bad = np.flatnonzero(a != b)
        assert bad.size == 0, f"{what}: {k} differs at {bad.size} instances, first {bad[0]}: got {got[k][bad[0]]!r}, want {want[k][bad[0]]!r}"

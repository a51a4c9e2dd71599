#!/usr/bin/env python3
"""What mmdx_animator_events costs next to mmdx_animator_advance on the same state and next to what it replaces, the read-back of
the crowd's clocks, in ONE process, interleaved, median of R rounds.

    timeout -k 10 600 python tools/events_ab.py            (AB_ROUNDS=7 AB_ITERS=200)

Shape: a set of 8 clips (4 bones, 20 keys per bone over 600 frames: the animator reads lengths only), every clip looping, 8 markers
per clip on 8 channels, at 1 024 and at 16 384 instances; a third of the crowd is mid-fade, speeds 1, 0.5 and -1.  Rows, microseconds
per call (AB_ITERS back-to-back calls between two syncs of the model's stream, host clock, so launch overhead is included):
    masks            mmdx_animator_events, n_lists = 0, a host dt (one launch)
    masks (dev dt)   the same with MMDX_ANIM_DT_ON_DEVICE
    no markers       the masks call with an empty event set: the state loads, the clocks and the offset-table gather, no marker scan
    + 1 list         masks plus one list of two channels (two launches)
    + 4 lists        masks plus four lists, with levels (a third culled)
    advance          mmdx_animator_advance with a host dt, on the same state
    get_state        mmdx_animator_get_state of clips_a, times_a and loops into host memory: what an adopter reads back every frame
                     today before searching the key times on the CPU (the search itself is not counted)
The event rows and advance are also timed by HIP events on the model's stream (mmdx_timer_*), which leaves the host's share of
a call -- building the argument struct in Python -- out: the second table.  Nothing here is a pass / fail number."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from simple_mmd_renderer_amd import synth, vmd  # noqa: E402
from simple_mmd_renderer_amd.engine import DeformModel, DeviceBuffer  # noqa: E402

SIZES = (1024, 16384)
NCLIPS, NMARK = 8, 8
ROWS = ("masks", "masks (dev dt)", "no markers", "+ 1 list", "+ 4 lists", "advance", "get_state")


def main():
    rounds, iters = int(os.environ.get("AB_ROUNDS", "7")), int(os.environ.get("AB_ITERS", "200"))
    names = [f"b{i}" for i in range(4)]
    dm = DeformModel(synth.make_model(256, 4, 0, 0, seed=1))
    vs = [vmd.Vmd(vmd.write_vmd(synth.make_bone_keys(names, 303 + c, keys_per=20, span=600), [])) for c in range(NCLIPS)]
    bms = [v.bind_bones(names) for v in vs]
    ms = vmd.MotionSet(bms)
    res = {}
    for ni in SIZES:
        rng = np.random.default_rng(2027 + ni)
        an = vmd.Animator(ms, ni)
        lengths = [r[0] for r in an.clip_table()]
        markers = [(lengths[c] * (j + 0.5) / NMARK, c, j) for c in range(NCLIPS) for j in range(NMARK)]
        es, empty = vmd.EventSet(an, markers), vmd.EventSet(an, [])
        fading = rng.random(ni) < 1 / 3
        clips_a, clips_b = rng.integers(0, NCLIPS, ni), rng.integers(0, NCLIPS, ni)
        state = dict(clips_a=clips_a, clips_b=np.where(fading, clips_b, vmd.CLIP_NONE),
                     times_a=rng.uniform(0, 1, ni) * np.asarray(lengths)[clips_a],
                     times_b=np.where(fading, rng.uniform(0, 1, ni) * np.asarray(lengths)[clips_b], 0.0),
                     weights=np.where(fading, rng.uniform(0, 1, ni), 0.0), fade_rate=np.where(fading, 0.01, 0.0),
                     speed=rng.choice([1.0, 0.5, -1.0], ni))
        an.set_state(dm, **state)
        levels = np.where(rng.random(ni) < 1 / 3, 0xFFFFFFFF, 0).astype(np.uint32)
        d_dt = DeviceBuffer.from_numpy(np.array([1 / 60], np.float64))
        d_fired, d_ids, d_counts, d_levels = DeviceBuffer(ni * 4), DeviceBuffer(4 * ni * 4), DeviceBuffer(16), DeviceBuffer.from_numpy(levels)
        one = ((0x03,), ni, d_ids.ptr, d_counts.ptr)
        four = ((0x03, 0x0C, 0x30, 0xFF), ni, d_ids.ptr, d_counts.ptr)
        runs = {"masks": lambda: an.events(es, d_fired.ptr, dt=1 / 60, model=dm),
                "masks (dev dt)": lambda: an.events(es, d_fired.ptr, dt_ptr=d_dt.ptr, model=dm),
                "no markers": lambda: an.events(empty, d_fired.ptr, dt=1 / 60, model=dm),
                "+ 1 list": lambda: an.events(es, d_fired.ptr, dt=1 / 60, lists=one, model=dm),
                "+ 4 lists": lambda: an.events(es, d_fired.ptr, dt=1 / 60, lists=four, levels_ptr=d_levels.ptr, model=dm),
                "advance": lambda: an.advance(1 / 60, dm),
                "get_state": lambda: an.get_state(dm, names=("clips_a", "times_a", "loops"))}
        runs["+ 4 lists"]()
        dm.sync()
        fired = d_fired.download((ni,), np.uint32)
        counts = d_counts.download((4,), np.uint32)
        print(f"NI={ni}: {int((fired != 0).sum())} instances fire in a step of 1/60 s; list lengths {counts.tolist()}", flush=True)

        def timed(run, n):
            for _ in range(5):
                run()
            dm.sync()
            t0 = time.perf_counter()
            for _ in range(n):
                run()
            dm.sync()
            return (time.perf_counter() - t0) / n * 1e6

        def by_events(run, n):
            dm.sync()
            dm.timer_start()
            for _ in range(n):
                run()
            return dm.timer_stop() / n * 1e3
        for r in range(rounds + 1):
            for name in ROWS:                              # back to back inside a round: interleaved
                us = timed(runs[name], iters if name != "get_state" else max(iters // 10, 3))
                ev = by_events(runs[name], iters) if name != "get_state" else None
                if r >= 1:                                 # round 0 warms every row up
                    res.setdefault((ni, name), []).append(us)
                    if ev is not None:
                        res.setdefault((ni, name, "events"), []).append(ev)
        for x in (es, empty, an, d_dt, d_fired, d_ids, d_counts, d_levels):
            x.free() if isinstance(x, DeviceBuffer) else x.close()
    print(f"\nus per call, median of {rounds} rounds of {iters} calls (min-max of the rounds); get_state: rounds of {max(iters // 10, 3)}")
    print(f"{'NI':>6s} " + " ".join(f"{n:>22s}" for n in ROWS))
    for ni in SIZES:
        cells = []
        for name in ROWS:
            a = np.array(res[(ni, name)])
            cells.append("%8.2f (%.2f-%.2f)" % (float(np.median(a)), a.min(), a.max()))
        print(f"{ni:6d} " + " ".join(f"{c:>22s}" for c in cells), flush=True)
    print(f"\nthe same by HIP events on the stream")
    print(f"{'NI':>6s} " + " ".join(f"{n:>22s}" for n in ROWS[:-1]))
    for ni in SIZES:
        cells = []
        for name in ROWS[:-1]:
            a = np.array(res[(ni, name, "events")])
            cells.append("%8.2f (%.2f-%.2f)" % (float(np.median(a)), a.min(), a.max()))
        print(f"{ni:6d} " + " ".join(f"{c:>22s}" for c in cells), flush=True)
    for x in [ms] + bms + vs:
        x.close()
    dm.close()


if __name__ == "__main__":
    main()

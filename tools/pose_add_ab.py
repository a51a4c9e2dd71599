#!/usr/bin/env python3
"""Interleaved timings of mmdx_pose_add (additive layers) next to the track call it follows, to mmdx_pose_blend on the same operands
and to a device-to-device copy of the bytes it moves, in ONE process, on the same arrays, median of R rounds.

    timeout -k 10 900 python tools/pose_add_ab.py            (AB_ROUNDS=7 AB_ITERS=100 AB_SIZES=1024,16384)

Shape: 1 024 and 16 384 instances x 300 bones (the config-3 crowd), a set of 8 clips as in tools/motion_set_ab.py, every operand in
HBM, in place (out == a).  The reference rows are the set's clips at time 0 (mmdx_motion_set_eval_bones_time with clips[i] = i).
Rows, in microseconds per call by HIP events around AB_ITERS back-to-back calls on the model's stream (mmdx_timer_*, the clock
mmdx_bench_copy uses, the launch included):
    (a) mmdx_motion_set_blend_bones_time for the crowd: the track call this one follows
    (b) mmdx_pose_blend on the same operands, weight 0.5, half the bones masked in
    (c) mmdx_pose_add, every weight 0: nothing to do, every workgroup returns after reading its weight
    (d) every item mixing (weight 0.5, no mask), without a reference: one acos and three sin through double per item
    (e) every item mixing, with a reference: + the reference's 32 bytes, an inverse and a quaternion product
    (f) (e) for 10 % of the instances, scattered; the others have weight 0
    (g) (f) through a select list of those 10 %
    copy: mmdx_bench_copy of the bytes (d) moves -- A and B read, out written: NI x NB x 32 bytes x 3
Every row is also given as a ratio to (b) and to (a), with the min-max of the per-round ratio.  Because the calls run in place the
base rows drift from call to call (they stay finite: unit quaternions multiply to unit quaternions); the work per call does not
depend on the values.  Nothing here is a pass / fail number."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from simple_mmd_renderer_amd import _capi as api  # noqa: E402
from simple_mmd_renderer_amd import synth, vmd  # noqa: E402
from simple_mmd_renderer_amd.engine import DeformModel, DeviceBuffer  # noqa: E402
from tools.motion_set_ab import NCLIPS, NM, make_clip  # noqa: E402


def run_size(dm, ms, nb, ni, rounds, iters):
    rng = np.random.default_rng(2026 + ni)
    ops = [rng.integers(0, NCLIPS, ni).astype(np.uint32), rng.uniform(0, 20, ni), rng.integers(0, NCLIPS, ni).astype(np.uint32),
           rng.uniform(0, 20, ni), rng.uniform(0, 1, ni).astype(np.float32)]
    d_ops = [DeviceBuffer.from_numpy(x) for x in ops]
    nbytes = ni * nb * 32
    d_a, d_b, d_refs = DeviceBuffer(nbytes), DeviceBuffer(nbytes), DeviceBuffer(NCLIPS * nb * 32)
    ptrs = [d.ptr for d in d_ops]
    layer_clips = rng.integers(0, NCLIPS, ni).astype(np.uint32)
    d_lc, d_lt = DeviceBuffer.from_numpy(layer_clips), DeviceBuffer.from_numpy(rng.uniform(0, 20, ni))
    ms.eval_bones_time_device(ni, d_lc.ptr, d_lt.ptr, d_b.ptr, dm)            # the layer's rows: one clip each, finite poses
    d_every, d_zero = DeviceBuffer.from_numpy(np.arange(NCLIPS, dtype=np.uint32)), DeviceBuffer.from_numpy(np.zeros(NCLIPS))
    ms.eval_bones_time_device(NCLIPS, d_every.ptr, d_zero.ptr, d_refs.ptr, dm)  # the reference rows: every clip at time 0
    mask = np.zeros((1, nb), np.float32)
    mask[0, nb // 2:] = 1                                                    # the upper half of the bone list
    worn = np.sort(rng.permutation(ni)[:ni // 10]).astype(np.uint32)         # who wears the layer in (f) and (g)
    w_tenth = np.zeros(ni, np.float32)
    w_tenth[worn] = 0.5
    d_w0, d_wh, d_wt = (DeviceBuffer.from_numpy(x) for x in (np.zeros(ni, np.float32), np.full(ni, 0.5, np.float32), w_tenth))
    d_mask, d_ids, d_list = DeviceBuffer.from_numpy(mask), DeviceBuffer.from_numpy(np.zeros(ni, np.uint32)), DeviceBuffer.from_numpy(worn)
    sel = vmd.instance_select(d_list.ptr, worn.size)
    moved = nbytes * 3 // 2                                                  # the copy reads and writes `moved` each: 3 arrays in all
    d_src, d_dst = DeviceBuffer(moved), DeviceBuffer(moved)

    def add(d_w, ref=False, select=None):
        vmd.add_poses_device(ni, nb, d_a.ptr, d_b.ptr, d_w.ptr, d_a.ptr, refs_ptr=d_refs.ptr if ref else None,
                             n_refs=NCLIPS if ref else 0, ref_ids_ptr=d_lc.ptr if ref else None, model=dm, select=select)
    variants = {"a": lambda: ms.blend_bones_time_device(ni, *ptrs, d_a.ptr, dm),
                "b": lambda: vmd.blend_poses_device(ni, nb, d_a.ptr, d_b.ptr, d_wh.ptr, d_a.ptr, d_mask.ptr, 1, d_ids.ptr, model=dm),
                "c": lambda: add(d_w0, True), "d": lambda: add(d_wh), "e": lambda: add(d_wh, True), "f": lambda: add(d_wt, True),
                "g": lambda: add(d_wt, True, sel)}

    def timed(run):
        for _ in range(3):
            run()
        dm.sync()
        dm.timer_start()
        for _ in range(iters):
            run()
        return dm.timer_stop() / iters * 1e3

    def copy_us():
        ms_avg = C.c_float(0)
        api.check(api.lib().mmdx_bench_copy(d_dst.ptr, d_src.ptr, moved, iters, C.byref(ms_avg)))
        return float(ms_avg.value) * 1e3
    res = {}
    for r in range(rounds + 1):
        row = {}
        for k, run in variants.items():                                      # back to back inside a round: interleaved
            if k in "defg":
                variants["a"]()                                              # fresh base rows: the adds before left theirs in d_a
            row[k] = timed(run)
        row["copy"] = copy_us()
        if r >= 1:                                                           # round 0 warms every row up
            for k, us in row.items():
                res.setdefault(k, []).append(us)
    dm.sync()
    finite = bool(np.isfinite(d_a.download((ni, nb, 8), np.float32)).all())
    t = {k: np.array(v) for k, v in res.items()}
    med = lambda x: float(np.median(x))                                      # noqa: E731
    span = lambda x: "%.3f-%.3f" % (x.min(), x.max())                        # noqa: E731
    print(f"\nNI={ni} NB={nb}: pose array {nbytes / 1e6:.1f} MB, (d) moves {3 * nbytes / 1e6:.1f} MB; us per call, median of {rounds} "
          f"rounds of {iters} calls, HIP events, in place; base rows finite at the end: {finite}")
    names = {"a": "(a) motion_set_blend_bones_time", "b": "(b) pose_blend, w 0.5, half masked", "c": "(c) pose_add, weights 0",
             "d": "(d) every item mixing, no reference", "e": "(e) every item mixing, reference", "f": "(f) (e) for 10 % of the instances",
             "g": "(g) (f) through a select list", "copy": "copy of the bytes (d) moves"}
    for k in ("a", "b", "c", "d", "e", "f", "g", "copy"):
        print(f"{names[k]:38s} {med(t[k]):9.2f}   /(b) {med(t[k]) / med(t['b']):7.3f} per round {span(t[k] / t['b'])}   "
              f"/(a) {med(t[k]) / med(t['a']):7.3f} per round {span(t[k] / t['a'])}")
    print(f"(d) moves {3 * nbytes / med(t['d']) / 1e6:.2f} TB/s read + written, the copy {2 * moved / med(t['copy']) / 1e6:.2f} TB/s: "
          f"(d) runs at {med(t['copy']) / med(t['d']):.3f} of the copy's rate  per round {span(t['copy'] / t['d'])}", flush=True)
    for x in d_ops + [d_a, d_b, d_refs, d_lc, d_lt, d_every, d_zero, d_w0, d_wh, d_wt, d_mask, d_ids, d_list, d_src, d_dst]:
        x.free()


def main():
    rounds, iters = int(os.environ.get("AB_ROUNDS", "7")), int(os.environ.get("AB_ITERS", "100"))
    sizes = [int(s) for s in os.environ.get("AB_SIZES", "1024,16384").split(",")]
    m = synth.make_config("config3_crowd")
    names = [f"b{i}" for i in range(m.nb)]
    mnames = [f"m{i}" for i in range(NM)]
    dm = DeformModel(m)
    vs = [make_clip(303 + c, names, mnames) for c in range(NCLIPS)]
    bms = [v.bind_bones(names) for v in vs]
    ms = vmd.MotionSet(bms)
    print(f"NB={m.nb}; set of {NCLIPS}: {ms.info}", flush=True)
    for ni in sizes:
        run_size(dm, ms, m.nb, ni, rounds, iters)
    for x in [ms] + bms + vs:
        x.close()
    dm.close()


if __name__ == "__main__":
    main()

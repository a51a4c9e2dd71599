#!/usr/bin/env python3
"""Interleaved timings of mmdx_pose_blend (layers: the masked blend of two evaluated pose arrays) next to the track call it follows
and to a device-to-device copy of the bytes it moves, in ONE process, on the same arrays, median of R rounds.

    timeout -k 10 900 python tools/row_blend_ab.py            (AB_ROUNDS=7 AB_ITERS=100 AB_SIZES=1024,16384)

Shape: 1 024 and 16 384 instances x 300 bones (the config-3 crowd; + 200 morphs in the motion set), a set of 8 clips as in
tools/motion_set_ab.py, every operand in HBM.  Rows, in microseconds per call by HIP events around AB_ITERS back-to-back calls on
the model's stream (mmdx_timer_*, the clock mmdx_bench_copy uses):
    (a) mmdx_motion_set_blend_bones_time for the crowd: the call this one sits next to
    (b) pose blend in place (out == a), every weight 0: nothing to do, every workgroup returns after reading its weight
    (c) in place, every weight 1 under an upper-body mask in which half the bones are 1: half the items become B
    (d) as (c) for 10 % of the instances, scattered; the others have weight 0
    (e) (d) through a select list of those 10 %
    copy: mmdx_bench_copy of the bytes (c) moves -- B read and out written for the masked half; the other half is neither read nor
          written in place: NI x NB/2 x 32 bytes each way
then (c) as a fraction of the copy's rate, and (b), (d), (e) relative to (c), each with the min-max of the per-round ratio.  Nothing
here is a pass / fail number."""
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
    d_a, d_b = DeviceBuffer(nbytes), DeviceBuffer(nbytes)
    ptrs = [d.ptr for d in d_ops]
    ms.blend_bones_time_device(ni, *ptrs, d_b.ptr, dm)                       # the layer's rows: finite poses
    mask = np.zeros((1, nb), np.float32)
    mask[0, nb // 2:] = 1                                                    # the upper half of the bone list
    worn = np.sort(rng.permutation(ni)[:ni // 10]).astype(np.uint32)         # who wears the layer in (d) and (e)
    w_tenth = np.zeros(ni, np.float32)
    w_tenth[worn] = 1
    d_w0, d_w1, d_wt = (DeviceBuffer.from_numpy(x) for x in (np.zeros(ni, np.float32), np.ones(ni, np.float32), w_tenth))
    d_mask, d_ids, d_list = DeviceBuffer.from_numpy(mask), DeviceBuffer.from_numpy(np.zeros(ni, np.uint32)), DeviceBuffer.from_numpy(worn)
    sel = vmd.instance_select(d_list.ptr, worn.size)
    moved = ni * (nb - nb // 2) * 32                                         # (c): bytes read of B = bytes written of out
    d_src, d_dst = DeviceBuffer(moved), DeviceBuffer(moved)

    def layer(d_w, select=None):
        vmd.blend_poses_device(ni, nb, d_a.ptr, d_b.ptr, d_w.ptr, d_a.ptr, d_mask.ptr, 1, d_ids.ptr, model=dm, select=select)
    variants = {"a": lambda: ms.blend_bones_time_device(ni, *ptrs, d_a.ptr, dm), "b": lambda: layer(d_w0), "c": lambda: layer(d_w1),
                "d": lambda: layer(d_wt), "e": lambda: layer(d_wt, sel)}

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
        row = {k: timed(run) for k, run in variants.items()}                 # back to back inside a round: interleaved
        row["copy"] = copy_us()
        if r >= 1:                                                           # round 0 warms every row up
            for k, us in row.items():
                res.setdefault(k, []).append(us)
    t = {k: np.array(v) for k, v in res.items()}
    med = lambda x: float(np.median(x))                                      # noqa: E731
    span = lambda x: "%.3f-%.3f" % (x.min(), x.max())                        # noqa: E731
    print(f"\nNI={ni} NB={nb}: pose array {nbytes / 1e6:.1f} MB, (c) moves {2 * moved / 1e6:.1f} MB; us per call, median of {rounds} "
          f"rounds of {iters} calls, HIP events")
    print(f"(a) motion_set_blend_bones_time        {med(t['a']):9.2f}   spread {span(t['a'] / med(t['a']))}")
    print(f"(b) pose blend in place, weights 0     {med(t['b']):9.2f}   (b)/(c) {med(t['b']) / med(t['c']):.3f}  per round {span(t['b'] / t['c'])}")
    print(f"(c) weights 1, half the bones masked   {med(t['c']):9.2f}   {2 * moved / med(t['c']) / 1e6:.2f} TB/s read + written;  (c)/(a) "
          f"{med(t['c']) / med(t['a']):.3f}")
    print(f"(d) (c) for 10 % of the instances      {med(t['d']):9.2f}   (d)/(c) {med(t['d']) / med(t['c']):.3f}  per round {span(t['d'] / t['c'])}")
    print(f"(e) (d) through a select list          {med(t['e']):9.2f}   (e)/(c) {med(t['e']) / med(t['c']):.3f}  per round {span(t['e'] / t['c'])}")
    print(f"copy of the bytes (c) moves            {med(t['copy']):9.2f}   {2 * moved / med(t['copy']) / 1e6:.2f} TB/s read + written")
    print(f"(c) runs at {med(t['copy']) / med(t['c']):.3f} of the copy's rate  per round {span(t['copy'] / t['c'])}", flush=True)
    for x in d_ops + [d_a, d_b, d_w0, d_w1, d_wt, d_mask, d_ids, d_list, d_src, d_dst]:
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

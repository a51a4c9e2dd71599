#!/usr/bin/env python3
"""Interleaved A/B of mmdx_palette_place against the solve it follows and against a device-to-device copy of the same array, in ONE
process, on the same arrays, median of R rounds.

    timeout -k 10 600 python tools/place_ab.py            (AB_ROUNDS=7 AB_ITERS=200)

Shape: 1 024 instances x 300 bones (the config-3 crowd, a 19.7 MB palette array), a motion set of 8 clips as in
tools/motion_set_ab.py, every operand in HBM.  Rows, in microseconds per call (AB_ITERS back-to-back calls between two
synchronisations of the model's stream, timed by the host clock, so launch overhead is included -- the calls are a few
microseconds long):
    (a) mmdx_skeleton_solve_motion_set_time alone
    (b) (a) + mmdx_palette_place in pose form, in place
    (c) (a) + mmdx_palette_place in matrix form, out of place
    (d) the place call alone (pose form, in place)
    (e) a device-to-device copy of the same array (mmdx_bench_copy, HIP events around AB_ITERS copies): the yardstick for (d) -- the
        kernel moves exactly a copy's bytes and adds 28 float operations per 16 of them
then (b)/(a) and (c)/(a) -- what placing costs an adopter per frame -- and (d)/(e), each with the min-max of the per-round ratio,
next to the min-max spread of (a) itself.  (d) is also given by HIP events (mmdx_timer_*), the clock (e) uses.  Nothing here is a
pass / fail number."""
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from simple_mmd_renderer_amd import _capi as api  # noqa: E402
from simple_mmd_renderer_amd import synth, vmd  # noqa: E402
from simple_mmd_renderer_amd.engine import DeformModel, DeviceBuffer  # noqa: E402
from tools.motion_set_ab import NCLIPS, NI, NM, make_clip  # noqa: E402

ALL_DEV = api.PALETTE_ON_DEVICE | api.PLACE_ON_DEVICE | api.OUT_ON_DEVICE


def main():
    rounds, iters = int(os.environ.get("AB_ROUNDS", "7")), int(os.environ.get("AB_ITERS", "200"))
    m = synth.make_config("config3_crowd")
    names = [f"b{i}" for i in range(m.nb)]
    mnames = [f"m{i}" for i in range(NM)]
    dm = DeformModel(m)
    sk = vmd.Skeleton(m.bone_pos, np.asarray(m.bone_parent, np.int32))
    assert sk.info["solver"] == vmd.SOLVER_PARALLEL_FK
    vs = [make_clip(303 + c, names, mnames) for c in range(NCLIPS)]
    bms = [v.bind_bones(names) for v in vs]
    ms = vmd.MotionSet(bms)
    nbytes = NI * m.nb * 64
    print(f"NI={NI} NB={m.nb}; palette array {nbytes / 1e6:.1f} MB; set of {NCLIPS}: {ms.info}", flush=True)
    rng = np.random.default_rng(2026)
    times = ((np.arange(NI) * 7) % 600) / 30.0 + (np.arange(NI) % 5) / 144.0
    clips = rng.integers(0, NCLIPS, NI).astype(np.uint32)
    poses = np.zeros((NI, 8), np.float32)
    poses[:, 0], poses[:, 2] = (np.arange(NI) % 32) * 12.0, (np.arange(NI) // 32) * 12.0
    yaw = rng.uniform(-np.pi, np.pi, NI)
    poses[:, 5], poses[:, 7] = np.sin(yaw / 2), np.cos(yaw / 2)
    mats = np.tile(np.eye(4, dtype=np.float32).reshape(16), (NI, 1))
    mats[:, 0], mats[:, 2], mats[:, 8], mats[:, 10] = np.cos(yaw), -np.sin(yaw), np.sin(yaw), np.cos(yaw)
    mats[:, 12:15] = poses[:, :3]
    d_c, d_t, d_pose, d_mat = (DeviceBuffer.from_numpy(x) for x in (clips, times, poses, mats))
    d_pal, d_out = DeviceBuffer(nbytes), DeviceBuffer(nbytes)

    def solve():
        sk.solve_motion_set_time_device(ms, NI, d_c.ptr, d_t.ptr, d_pal.ptr, dm)

    def place_pose():
        dm.place_palettes(NI, d_pal.ptr, d_pose.ptr, d_pal.ptr, ALL_DEV)

    def place_matrix():
        dm.place_palettes(NI, d_pal.ptr, d_mat.ptr, d_out.ptr, ALL_DEV | api.PLACE_MATRIX)
    variants = {"a": solve, "b": lambda: (solve(), place_pose()), "c": lambda: (solve(), place_matrix()), "d": place_pose}

    def timed(run):
        for _ in range(5):
            run()
        dm.sync()
        t0 = time.perf_counter()
        for _ in range(iters):
            run()
        dm.sync()
        return (time.perf_counter() - t0) / iters * 1e6

    def place_by_events():
        d_pal.memset(0)                                # in place 200 times over: keep the values finite
        dm.sync()
        dm.timer_start()
        for _ in range(iters):
            place_pose()
        return dm.timer_stop() / iters * 1e3

    def copy_us():
        ms_avg = C.c_float(0)
        api.check(api.lib().mmdx_bench_copy(d_out.ptr, d_pal.ptr, nbytes, iters, C.byref(ms_avg)))
        return float(ms_avg.value) * 1e3
    res = {}
    for r in range(rounds + 1):
        row = {}
        for v, run in variants.items():                # a, b, c, d, e back to back inside a round: interleaved
            if v == "d":
                d_pal.memset(0)
            row[v] = timed(run)
        row["d_ev"] = place_by_events()
        row["e"] = copy_us()
        if r >= 1:                                     # round 0 warms every row up
            for k, us in row.items():
                res.setdefault(k, []).append(us)
    a, b, c, d, d_ev, e = (np.array(res[k]) for k in ("a", "b", "c", "d", "d_ev", "e"))
    med = lambda x: float(np.median(x))                # noqa: E731
    span = lambda x: "%.3f-%.3f" % (x.min(), x.max())  # noqa: E731
    print(f"\nus per call, median of {rounds} rounds of {iters} calls")
    print(f"(a) solve_motion_set_time            {med(a):9.2f}   spread of (a) {span(a / med(a))}")
    print(f"(b) (a) + place, pose, in place      {med(b):9.2f}   (b)/(a) {med(b) / med(a):.3f}  per round {span(b / a)}")
    print(f"(c) (a) + place, matrix, out of place{med(c):9.2f}   (c)/(a) {med(c) / med(a):.3f}  per round {span(c / a)}")
    print(f"(d) place alone, host clock          {med(d):9.2f}")
    print(f"(d) place alone, HIP events          {med(d_ev):9.2f}   {2 * nbytes / med(d_ev) / 1e6:.2f} TB/s read + written")
    print(f"(e) device-to-device copy, HIP events{med(e):9.2f}   {2 * nbytes / med(e) / 1e6:.2f} TB/s read + written")
    print(f"(d)/(e) by events {med(d_ev) / med(e):.3f}  per round {span(d_ev / e)};  host clock over events {med(d) / med(e):.3f}", flush=True)
    for x in [ms, sk] + bms + vs + [d_c, d_t, d_pose, d_mat, d_pal, d_out]:
        x.free() if isinstance(x, DeviceBuffer) else x.close()
    dm.close()


if __name__ == "__main__":
    main()

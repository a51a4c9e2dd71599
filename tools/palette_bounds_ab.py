#!/usr/bin/env python3
"""What mmdx_palette_bounds costs and how loose its boxes are, on the config-3 crowd (1 024 instances x 300 bones, a 19.7 MB palette
array, 50 000 vertices), every operand in HBM.  Three steps, each a process of its own so that each runs under its own time limit:

    timeout -k 10 300 python tools/palette_bounds_ab.py kernel       (AB_ROUNDS=7 AB_ITERS=200)
    timeout -k 10 600 python tools/palette_bounds_ab.py deform       (AB_ROUNDS=7 AB_ITERS=40 AB_TRIES=16)
    timeout -k 10 300 python tools/palette_bounds_ab.py looseness

kernel     (a) mmdx_palette_bounds alone and (b) a device-to-device copy of the same palette array (mmdx_bench_copy), interleaved
           inside every round, both timed by HIP events around AB_ITERS back-to-back calls; (a) also by the host clock (launch
           overhead included).  The kernel reads a copy's bytes and writes 24 KB, so (a) should not exceed (b).
deform     (c) mmdx_deform_batched_bounds minus mmdx_deform_batched on the same arrays (SoA, shared rates, arrays from
           mmdx_crowd_output_alloc as bench.py takes them), interleaved: the per-frame cost the new call replaces.
looseness  (d) per axis, median and maximum over the instances of (palette-box extent) / (deform-box extent), with morph_scale 0
           (zero rates) and morph_scale 1 (the crowd's shared rates).
Medians of AB_ROUNDS rounds after one warm-up round, with the min-max over the rounds.  Nothing here is a pass / fail number."""
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from simple_mmd_renderer_amd import _capi as api, synth  # noqa: E402
from simple_mmd_renderer_amd.crowd import crowd_frames  # noqa: E402
from simple_mmd_renderer_amd.engine import DeformModel, DeviceBuffer  # noqa: E402

NI = 1024
DEV = api.PALETTE_ON_DEVICE | api.OUT_ON_DEVICE
med = lambda x: float(np.median(x))                    # noqa: E731
span = lambda x: "%.3f-%.3f" % (np.min(x), np.max(x))  # noqa: E731


def setup():
    m = synth.make_config("config3_crowd")
    dm = DeformModel(m)
    pals = synth.make_palettes(m, crowd_frames(0, NI))
    return m, dm, pals


def step_kernel():
    rounds, iters = int(os.environ.get("AB_ROUNDS", "7")), int(os.environ.get("AB_ITERS", "200"))
    m, dm, pals = setup()
    t = dm.bone_boxes()
    print(f"NI={NI} NB={m.nb} n_boxes={t['n_boxes']} eps={t['eps']:.3e}; palette array {pals.nbytes / 1e6:.1f} MB", flush=True)
    d_pal, d_copy, d_bnd = DeviceBuffer.from_numpy(pals), DeviceBuffer(pals.nbytes), DeviceBuffer(NI * 24)
    run = lambda: dm.palette_bounds_raw(NI, d_pal.ptr, d_bnd.ptr, DEV, 0.1, 1.0)       # noqa: E731
    res = {"a_ev": [], "a_host": [], "b": []}
    for r in range(rounds + 1):
        for _ in range(5):
            run()
        dm.sync()
        dm.timer_start()
        for _ in range(iters):
            run()
        a_ev = dm.timer_stop() / iters * 1e3
        t0 = time.perf_counter()
        for _ in range(iters):
            run()
        dm.sync()
        a_host = (time.perf_counter() - t0) / iters * 1e6
        ms_avg = C.c_float(0)
        api.check(api.lib().mmdx_bench_copy(d_copy.ptr, d_pal.ptr, pals.nbytes, iters, C.byref(ms_avg)))
        if r >= 1:
            res["a_ev"].append(a_ev)
            res["a_host"].append(a_host)
            res["b"].append(float(ms_avg.value) * 1e3)
    a, ah, b = (np.array(res[k]) for k in ("a_ev", "a_host", "b"))
    print(f"\nus per call, median of {rounds} rounds of {iters} calls")
    print(f"(a) mmdx_palette_bounds, HIP events   {med(a):9.2f}   {pals.nbytes / med(a) / 1e6:.2f} TB/s read   per round {span(a)}")
    print(f"(a) mmdx_palette_bounds, host clock   {med(ah):9.2f}")
    print(f"(b) device-to-device copy, HIP events {med(b):9.2f}   {2 * pals.nbytes / med(b) / 1e6:.2f} TB/s read + written   per round {span(b)}")
    print(f"(a)/(b) {med(a) / med(b):.3f}  per round {span(a / b)}", flush=True)
    for x in (d_pal, d_copy, d_bnd):
        x.free()
    dm.close()


def step_deform():
    rounds, iters = int(os.environ.get("AB_ROUNDS", "7")), int(os.environ.get("AB_ITERS", "40"))
    tries = int(os.environ.get("AB_TRIES", "16"))
    m, dm, pals = setup()
    d_a, d_b, pl = dm.alloc_outputs(api.OUT_SOA, NI, tries)
    d_pal, d_w, d_bnd = DeviceBuffer.from_numpy(pals), DeviceBuffer.from_numpy(synth.morph_weights(m.nm, 30)[0]), DeviceBuffer(NI * 24)
    flags = DEV | api.WEIGHTS_ON_DEVICE | api.WEIGHTS_SHARED | pl["store_flags"]
    print(f"NV={m.nv} NI={NI} placement {pl}", flush=True)
    res = {"plain": [], "bounds": []}
    for r in range(rounds + 1):
        for form in ("plain", "bounds"):
            run = lambda: dm.deform_batched_raw(NI, d_w.ptr, d_pal.ptr, d_a.ptr, d_b.ptr, api.OUT_SOA, flags, 1.0, 0,      # noqa: E731
                                                d_bnd.ptr if form == "bounds" else None)
            for _ in range(5):
                run()
            dm.sync()
            t0 = time.perf_counter()
            for _ in range(iters):
                run()
            dm.sync()
            if r >= 1:
                res[form].append((time.perf_counter() - t0) / iters * 1e3)
    p, b = np.array(res["plain"]), np.array(res["bounds"])
    print(f"\nms per call, median of {rounds} rounds of {iters} calls")
    print(f"mmdx_deform_batched         {med(p):8.4f}   per round {span(p)}")
    print(f"mmdx_deform_batched_bounds  {med(b):8.4f}   per round {span(b)}")
    print(f"(c) bounds - plain          {(med(b) - med(p)) * 1e3:8.1f} us   ratio {med(b) / med(p):.3f}  per round {span(b / p)}", flush=True)
    for x in (d_a, d_b, d_pal, d_w, d_bnd):
        x.free()
    dm.close()


def step_looseness():
    m, dm, pals = setup()
    d_a, d_b, pl = dm.alloc_outputs(api.OUT_SOA, NI, 1)
    d_pal, d_bnd, d_box = DeviceBuffer.from_numpy(pals), DeviceBuffer(NI * 24), DeviceBuffer(NI * 24)
    flags = DEV | api.WEIGHTS_ON_DEVICE | api.WEIGHTS_SHARED
    print("(d) palette-box extent / deform-box extent over %d instances, pos_scale 0.1" % NI)
    for ms, w in ((0.0, np.zeros(m.nm, np.float32)), (1.0, synth.morph_weights(m.nm, 30)[0])):
        d_w = DeviceBuffer.from_numpy(w)
        dm.deform_batched_raw(NI, d_w.ptr, d_pal.ptr, d_a.ptr, d_b.ptr, api.OUT_SOA, flags, 0.1, 0, d_bnd.ptr)
        dm.palette_bounds_raw(NI, d_pal.ptr, d_box.ptr, DEV, 0.1, ms)
        dm.sync()
        bnd, box = d_bnd.download((NI, 6), np.float32), d_box.download((NI, 6), np.float32)
        inside = bool((box[:, :3] <= bnd[:, :3]).all() and (box[:, 3:] >= bnd[:, 3:]).all())
        ratio = (box[:, 3:] - box[:, :3]) / (bnd[:, 3:] - bnd[:, :3])
        print("morph_scale %g: median x %.3f y %.3f z %.3f   max x %.3f y %.3f z %.3f   every deform box inside: %s" %
              ((ms,) + tuple(np.median(ratio, axis=0)) + tuple(ratio.max(axis=0)) + (inside,)), flush=True)
        d_w.free()
    for x in (d_a, d_b, d_pal, d_bnd, d_box):
        x.free()
    dm.close()


if __name__ == "__main__":
    steps = {"kernel": step_kernel, "deform": step_deform, "looseness": step_looseness}
    if len(sys.argv) != 2 or sys.argv[1] not in steps:
        sys.exit("usage: palette_bounds_ab.py kernel | deform | looseness")
    steps[sys.argv[1]]()

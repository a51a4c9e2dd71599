#!/usr/bin/env python3
"""Interleaved A/B of the two forms of mmdx_cull_bounds (one workgroup walking the crowd / a count and a scatter launch) in ONE
process, on synthetic bounds, median of R rounds -- and, in the same run, the cost the cull is there to save: the parent's
mmdx_deform_batched_select at k = 256 of 1 024 on the config-3 shape.

    python tools/cull_ab.py            (AB_ROUNDS=7 AB_ITERS=40 AB_TRIES=16 AB_NI=1024,4096,16384,262144)

Per crowd size: both forms (MMDX_CULL_FORM, each with its default chunk), n_lods 1 and 4, a device view of six planes that keeps
about half the crowd, LOD rings that split the survivors about evenly.  ms per call = host clock around AB_ITERS back-to-back calls
ending in a stream synchronise.  The last line names the smallest swept crowd at which form 2 is faster at both list counts: the
planner's crossover (cull_shape.hpp kCullCrossover) is set from it."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from simple_mmd_renderer_amd import _capi as api, synth  # noqa: E402
from simple_mmd_renderer_amd.crowd import crowd_frames  # noqa: E402
from simple_mmd_renderer_amd.engine import DeformModel, DeviceBuffer, make_cull_view  # noqa: E402


def make_scene(ni, rng):
    c = rng.uniform(-100, 100, (ni, 3))
    h = rng.uniform(0.5, 2, (ni, 3))
    return np.concatenate([c - h, c + h], axis=1).astype(np.float32)


def make_view(n_lods):
    # x >= 0 keeps half; the other five planes of the box never cull.  Distances from the eye at the centre of the kept half:
    # thirds of the way out, so the four lists are of the same order.
    planes = [[1, 0, 0, 0], [-1, 0, 0, 200], [0, 1, 0, 200], [0, -1, 0, 200], [0, 0, 1, 200], [0, 0, -1, 200]]
    return make_cull_view(planes, (50.0, 0.0, 0.0), (60.0, 85.0, 105.0)[:n_lods - 1], 0.0)


def main():
    rounds, iters = int(os.environ.get("AB_ROUNDS", "7")), int(os.environ.get("AB_ITERS", "40"))
    tries = int(os.environ.get("AB_TRIES", "16"))
    nis = [int(x) for x in os.environ.get("AB_NI", "1024,4096,16384,262144").split(",")]
    lib = api.lib()
    rng = np.random.default_rng(2026)

    def timed(dm, run, n):
        for _ in range(5):
            run()
        dm.sync()
        t0 = time.perf_counter()
        for _ in range(n):
            run()
        dm.sync()
        return (time.perf_counter() - t0) / n * 1e3

    # the yardstick: config 3, 256 of 1 024 listed (tools/select_ab.py's row)
    c3 = synth.make_config("config3_crowd")
    NI3, K3 = 1024, 256
    dm = DeformModel(c3)
    d_a, d_b, pl = dm.alloc_outputs(api.OUT_SOA, NI3, tries)
    d_pal = DeviceBuffer.from_numpy(synth.make_palettes(c3, crowd_frames(0, NI3)))
    d_w = DeviceBuffer.from_numpy(synth.morph_weights(c3.nm, 30)[0])
    d_sel = DeviceBuffer.from_numpy(rng.permutation(NI3)[:K3].astype(np.uint32))
    d_selcnt = DeviceBuffer.from_numpy(np.array([K3], np.uint32))
    flags = api.PALETTE_ON_DEVICE | api.WEIGHTS_ON_DEVICE | api.OUT_ON_DEVICE | api.WEIGHTS_SHARED | pl["store_flags"]
    print(f"yardstick: config 3 NV={c3.nv} NI={NI3} k={K3} placement {pl}", flush=True)

    def select():
        dm.deform_batched_raw(NI3, d_w.ptr, d_pal.ptr, d_a.ptr, d_b.ptr, api.OUT_SOA, flags, 1.0, 0, None, select_ptr=d_sel.ptr,
                              select_count_ptr=d_selcnt.ptr, n_select=NI3)

    crowds = {}
    for ni in nis:
        crowds[ni] = dict(bounds=DeviceBuffer.from_numpy(make_scene(ni, rng)), ids=DeviceBuffer(4 * ni * 4), cnt=DeviceBuffer(16),
                          views={k: DeviceBuffer.from_numpy(np.frombuffer(bytes(make_view(k)), np.uint8)) for k in (1, 4)})
    res, shapes, kept = {}, {}, {}
    for r in range(rounds + 1):
        got = {("select", 0, 0, 0): timed(dm, select, iters)}
        for ni in nis:
            c = crowds[ni]
            for form in (1, 2):
                os.environ["MMDX_CULL_FORM"] = str(form)
                lib.mmdx_debug_reload_env()
                for n_lods in (1, 4):
                    run = lambda: dm.cull_bounds(c["bounds"], c["views"][n_lods], ni, c["ids"], c["cnt"])
                    got[("cull", ni, form, n_lods)] = timed(dm, run, iters)
                    s = dm.last_launch_shape()
                    assert s["kernel"] == "cull" and s["select"] == form
                    shapes[(ni, form)] = (s["group"], s["ngroups"])
                    kept[(ni, n_lods)] = c["cnt"].download((4,), np.uint32).tolist()
        os.environ.pop("MMDX_CULL_FORM", None)
        lib.mmdx_debug_reload_env()
        if r >= 1:                                           # round 0 warms every row up
            for key, v in got.items():
                res.setdefault(key, []).append(v)
    med = {k: float(np.median(v)) for k, v in res.items()}
    sel = med[("select", 0, 0, 0)]
    print(f"\nselect 256 of 1024, config 3: {sel:.4f} ms per call (median of {rounds}; min {min(res[('select', 0, 0, 0)]):.4f})")
    print(f"\n{'NI':>7s} {'lods':>4s} {'form 1 ms':>10s} {'(chunk x n)':>12s} {'form 2 ms':>10s} {'(chunk x n)':>12s} {'f2/f1':>7s} {'best/select':>11s}   "
          f"list lengths   (median of {rounds}; f2/f1 min-max over rounds)")
    crossover = None
    for ni in nis:
        faster = True
        for n_lods in (1, 4):
            a, b = med[("cull", ni, 1, n_lods)], med[("cull", ni, 2, n_lods)]
            ratios = np.array(res[("cull", ni, 2, n_lods)]) / np.array(res[("cull", ni, 1, n_lods)])
            faster = faster and b < a
            print(f"{ni:7d} {n_lods:4d} {a:10.4f} {'%d x %d' % shapes[(ni, 1)]:>12s} {b:10.4f} {'%d x %d' % shapes[(ni, 2)]:>12s} {b / a:7.3f} "
                  f"{min(a, b) / sel:11.3f}   {kept[(ni, n_lods)]}   ({ratios.min():.3f}-{ratios.max():.3f})", flush=True)
        if faster and crossover is None:
            crossover = ni
    print(f"\nsmallest swept NI at which form 2 is faster at both list counts: {crossover}")
    for c in crowds.values():
        for x in [c["bounds"], c["ids"], c["cnt"]] + list(c["views"].values()):
            x.free()
    for x in (d_a, d_b, d_pal, d_w, d_sel, d_selcnt):
        x.free()
    dm.close()


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Interleaved A/B of mmdx_deform_batched_select (k listed instances out of 1 024) against the plain mmdx_deform_batched call
with n_instances = k -- the dense call that moves the same bytes -- in ONE process, on the same arrays, median of R rounds.

    python tools/select_ab.py            (AB_ROUNDS=7 AB_ITERS=40 AB_TRIES=16)

Config 3 shape (1 024 x 50 000 vertices, SoA, shared rates), every operand in HBM, arrays from mmdx_crowd_output_alloc with its
store_flags ORed into the call's flags, as bench.py does.  For k in 1 024, 512, 256, 64 and the lists {identity prefix, a seeded
random subset sorted, the same unsorted}: ms per step of the select call with the list and count in device memory, with the list
in host memory (copied per call; that call returns when its work is done), with the list positions blocked over the
workgroups instead of interleaved (MMDX_SELECT_INTERLEAVE=0, device list), and of the dense call on k instances; ratio = device-list
select / dense.  Then one row each for per-instance rates, f16 positions, the 32-byte vertex and tile order (k = 256, unsorted,
device list), and config 3 with bounds (against mmdx_deform_batched_bounds on k instances).
The dense call is timed with THIS library: its plain kernels are, instruction for instruction, the parent commit's
(profiles/select/disassembly_parent_vs_new.txt), so it is the parent's plain call with n_instances = k.
The last lines state the two conditions the call has to meet: 256 of 1 024 faster than the plain call on all 1 024, and the step's
cost falling from k = 1 024 to 64."""
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
KS = (1024, 512, 256, 64)


def make_lists(k, rng):
    sub = rng.permutation(NI)[:k].astype(np.uint32)
    return {"prefix": np.arange(k, dtype=np.uint32), "sorted": np.sort(sub), "unsorted": sub}


def main():
    rounds, iters = int(os.environ.get("AB_ROUNDS", "7")), int(os.environ.get("AB_ITERS", "40"))
    tries = int(os.environ.get("AB_TRIES", "16"))
    lib = api.lib()
    c3 = synth.make_config("config3_crowd")
    dev = api.PALETTE_ON_DEVICE | api.WEIGHTS_ON_DEVICE | api.OUT_ON_DEVICE
    rng = np.random.default_rng(2025)
    # (name, layout, per-instance rates, model flags, bounds, ks, list names)
    cases = [("config 3", api.OUT_SOA, False, {}, False, KS, ("prefix", "sorted", "unsorted")),
             ("config 3 + bounds", api.OUT_SOA, False, {}, True, (256,), ("unsorted",)),
             ("config 3' per-instance", api.OUT_SOA, True, {}, False, (256,), ("unsorted",)),
             ("f16", api.OUT_SOA_POS16, False, {"f16_positions": True}, False, (256,), ("unsorted",)),
             ("32-byte vertex", api.OUT_VERTEX32, False, {}, False, (256,), ("unsorted",)),
             ("tile order", api.OUT_SOA, False, {"tile_order": True}, False, (256,), ("unsorted",))]
    lists = {k: make_lists(k, rng) for k in KS}
    pals = synth.make_palettes(c3, crowd_frames(0, NI))
    setups = []
    for name, layout, per_inst, mflags, bounds, ks, lnames in cases:
        dm = DeformModel(c3, **mflags)
        d_a, d_b, pl = dm.alloc_outputs(layout, NI, tries)
        d_pal = DeviceBuffer.from_numpy(pals)
        w = synth.morph_weights(c3.nm, np.arange(NI) + 30) if per_inst else synth.morph_weights(c3.nm, 30)[0]
        d_w = DeviceBuffer.from_numpy(w)
        d_bnd = DeviceBuffer(NI * 24) if bounds else None
        d_ids, d_cnt = DeviceBuffer(NI * 4), DeviceBuffer(4)
        flags = dev | (0 if per_inst else api.WEIGHTS_SHARED) | pl["store_flags"]
        print(f"{name}: NV={c3.nv} NI={NI} placement {pl}", flush=True)
        setups.append((name, dm, layout, d_a, d_b, d_pal, d_w, d_bnd, d_ids, d_cnt, flags, ks, lnames))

    def timed(dm, run, n):
        for _ in range(5):
            run()
        dm.sync()
        t0 = time.perf_counter()
        for _ in range(n):
            run()
        dm.sync()
        return (time.perf_counter() - t0) / n * 1e3

    res = {}
    for r in range(rounds + 1):
        for name, dm, layout, d_a, d_b, d_pal, d_w, d_bnd, d_ids, d_cnt, flags, ks, lnames in setups:
            scale = 0.1 if layout == api.OUT_VERTEX32 else 1.0
            bptr = d_bnd.ptr if d_bnd else None
            ob = d_b.ptr if d_b else None

            def plain(n):
                dm.deform_batched_raw(n, d_w.ptr, d_pal.ptr, d_a.ptr, ob, layout, flags, scale, 0, bptr)
            got = {("all", "", "plain 1024"): timed(dm, lambda: plain(NI), iters)}
            for k in ks:
                got[(k, "", "dense")] = timed(dm, lambda: plain(k), iters)
                for ln in lnames:
                    ids = lists[k][ln]
                    d_ids.upload(ids)
                    d_cnt.upload(np.array([k], np.uint32))

                    def select_dev():
                        dm.deform_batched_raw(NI, d_w.ptr, d_pal.ptr, d_a.ptr, ob, layout, flags, scale, 0, bptr, select_ptr=d_ids.ptr,
                                              select_count_ptr=d_cnt.ptr, n_select=NI)

                    def select_host():
                        dm.deform_batched_raw(NI, d_w.ptr, d_pal.ptr, d_a.ptr, ob, layout, flags, scale, 0, bptr,
                                              select_ptr=ids.ctypes.data, n_select=k, select_on_device=False)
                    got[(k, ln, "device")] = timed(dm, select_dev, iters)
                    got[(k, ln, "host")] = timed(dm, select_host, iters)
                    os.environ["MMDX_SELECT_INTERLEAVE"] = "0"
                    lib.mmdx_debug_reload_env()
                    got[(k, ln, "blocked")] = timed(dm, select_dev, iters)
                    del os.environ["MMDX_SELECT_INTERLEAVE"]
                    lib.mmdx_debug_reload_env()
            if r >= 1:                                       # round 0 warms every row up
                for key, v in got.items():
                    res.setdefault((name,) + key, []).append(v)
    med = {k: float(np.median(v)) for k, v in res.items()}
    print(f"\n{'row':24s} {'k':>5s} {'list':9s} {'select dev':>11s} {'select host':>12s} {'blocked':>12s} {'dense k':>9s} "
          f"{'dev/dense':>10s}   (ms per step, median of {rounds}; ratio min-max)")
    for name, dm, layout, *_rest, ks, lnames in setups:
        print(f"{name:24s} {'1024':>5s} {'(plain)':9s} {'':11s} {'':12s} {'':12s} {med[(name, 'all', '', 'plain 1024')]:9.4f}")
        for k in ks:
            for ln in lnames:
                d, h, i = (med[(name, k, ln, f)] for f in ("device", "host", "blocked"))
                p = med[(name, k, "", "dense")]
                ratios = np.array(res[(name, k, ln, "device")]) / np.array(res[(name, k, "", "dense")])
                print(f"{name:24s} {k:5d} {ln:9s} {d:11.4f} {h:12.4f} {i:12.4f} {p:9.4f} {d / p:10.3f}   ({ratios.min():.3f}-{ratios.max():.3f})",
                      flush=True)
    name = "config 3"
    full = med[(name, "all", "", "plain 1024")]
    for mapping in ("device", "blocked"):
        s256 = med[(name, 256, "unsorted", mapping)]
        steps = [med[(name, k, "unsorted", mapping)] for k in KS]
        falling = all(a > b for a, b in zip(steps, steps[1:]))
        what = "interleaved (shipped)" if mapping == "device" else "blocked"
        print(f"{what}: select 256 of 1024 = {s256:.4f} ms vs plain 1024 = {full:.4f} ms: {'PASS' if s256 < full else 'FAIL'}; "
              f"k = 1024 -> 64: {' > '.join(f'{x:.4f}' for x in steps)}: {'falling' if falling else 'NOT falling'}")
    for s in setups:
        for x in s[3:10]:
            if x is not None and x.ptr:
                x.free()
        s[1].close()


if __name__ == "__main__":
    main()

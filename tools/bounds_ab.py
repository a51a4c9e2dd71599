#!/usr/bin/env python3
"""Interleaved A/B of mmdx_deform_batched against mmdx_deform_batched_bounds (per-instance bounds) in ONE process, on the same
arrays, median of R rounds.

    python tools/bounds_ab.py            (AB_ROUNDS=7 AB_ITERS=40 AB_TRIES=16)

Rows (1 024 instances unless said otherwise, every operand in HBM, arrays from mmdx_crowd_output_alloc with its store_flags ORed
into the call's flags, as bench.py does): config 3 (50 000 vertices, SoA, shared rates); NV = 50 003 pitched (config 3 with its
first 3 vertices appended once more, pitch = mmdx_model_output_pitch); config 3' (per-instance rates); f16 positions; the 32-byte
vertex (pos_scale 0.1); tile order; NI = 1 (one frame: the plain call takes the one-frame kernel, the bounds call the tile
kernel's bounds flavour plus the reduce launch).  Per row: ms per step without and with bounds, their ratio, and the deform
kernel's share of the step (the profile events around the deform launch -- and, for the bounds call, the reduce launch)."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from pitch_ab import grown  # noqa: E402
from simple_mmd_renderer_amd import _capi as api, synth  # noqa: E402
from simple_mmd_renderer_amd.crowd import crowd_frames  # noqa: E402
from simple_mmd_renderer_amd.engine import DeformModel, DeviceBuffer  # noqa: E402


def main():
    rounds, iters = int(os.environ.get("AB_ROUNDS", "7")), int(os.environ.get("AB_ITERS", "40"))
    tries = int(os.environ.get("AB_TRIES", "16"))
    c3 = synth.make_config("config3_crowd")
    dev = api.PALETTE_ON_DEVICE | api.WEIGHTS_ON_DEVICE | api.OUT_ON_DEVICE
    # (name, model, instances, layout, per-instance rates, pitched, model flags)
    cases = [("config 3", c3, 1024, api.OUT_SOA, False, False, {}),
             ("NV=50003 pitched", grown(c3, 3), 1024, api.OUT_SOA, False, True, {}),
             ("config 3' per-instance", c3, 1024, api.OUT_SOA, True, False, {}),
             ("f16", c3, 1024, api.OUT_SOA_POS16, False, False, {"f16_positions": True}),
             ("32-byte vertex", c3, 1024, api.OUT_VERTEX32, False, False, {}),
             ("tile order", c3, 1024, api.OUT_SOA, False, False, {"tile_order": True}),
             ("NI=1 frame", c3, 1, api.OUT_SOA, False, False, {})]
    setups = []
    for name, m, ni, layout, per_inst, pitched, mflags in cases:
        dm = DeformModel(m, **mflags)
        pitch = dm.output_pitch(layout) if pitched else 0
        d_a, d_b, pl = dm.alloc_outputs(layout, ni, tries, pitch=pitch)
        d_pal = DeviceBuffer.from_numpy(synth.make_palettes(m, crowd_frames(0, ni)))
        w = synth.morph_weights(m.nm, np.arange(ni) + 30) if per_inst else synth.morph_weights(m.nm, 30)[0]
        d_w = DeviceBuffer.from_numpy(w)
        d_bnd = DeviceBuffer(ni * 24)
        flags = dev | (0 if per_inst else api.WEIGHTS_SHARED) | pl["store_flags"]
        print(f"{name}: NV={m.nv} NI={ni} placement {pl}", flush=True)
        setups.append((name, dm, ni, layout, pitch, d_a, d_b, d_pal, d_w, d_bnd, flags))
    res = {}
    for r in range(rounds + 1):
        for name, dm, ni, layout, pitch, d_a, d_b, d_pal, d_w, d_bnd, flags in setups:
            scale = 0.1 if layout == api.OUT_VERTEX32 else 1.0
            n = iters * (25 if ni == 1 else 1)
            for form in ("plain", "bounds"):
                def run():
                    dm.deform_batched_raw(ni, d_w.ptr, d_pal.ptr, d_a.ptr, d_b.ptr if d_b else None, layout, flags, scale, pitch,
                                          d_bnd.ptr if form == "bounds" else None)
                for _ in range(5):
                    run()
                dm.sync()
                t0 = time.perf_counter()
                for _ in range(n):
                    run()
                dm.sync()
                step = (time.perf_counter() - t0) / n * 1e3
                dm.profile_enable(True)
                for _ in range(10):
                    run()
                dm.sync()
                calls, skin_ms, _morph_ms = dm.profile_collect()
                dm.profile_enable(False)
                if r >= 1:                                   # round 0 warms every row up
                    res.setdefault((name, form, "step"), []).append(step)
                    res.setdefault((name, form, "kernel"), []).append(skin_ms / max(calls, 1))
    print(f"\n{'row':26s} {'plain ms':>9s} {'bounds ms':>10s} {'ratio':>7s} {'kernel plain':>13s} {'kernel bounds':>14s} "
          f"{'kernel share':>13s}   (median of {rounds}; ratio min-max)")
    for name, *_ in setups:
        p, b = np.array(res[(name, "plain", "step")]), np.array(res[(name, "bounds", "step")])
        kp, kb = np.median(res[(name, "plain", "kernel")]), np.median(res[(name, "bounds", "kernel")])
        ratios = b / p
        print(f"{name:26s} {np.median(p):9.4f} {np.median(b):10.4f} {np.median(b) / np.median(p):7.3f} {kp:13.4f} {kb:14.4f} "
              f"{kb / np.median(b):13.3f}   ({ratios.min():.3f}-{ratios.max():.3f})", flush=True)
    for s in setups:
        for x in s[5:10]:
            if x is not None and x.ptr:
                x.free()
        s[1].close()


if __name__ == "__main__":
    main()

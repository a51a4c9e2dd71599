#!/usr/bin/env python3
"""What a call of mmdx_morph_motion_eval / _eval_time costs the host, with host pointers and with device pointers: microseconds
per call by the host clock around AB_ITERS back-to-back calls between two synchronisations of the model's stream, median and
min-max of AB_ROUNDS rounds after one warm-up round.  1 024 instances, 52 morphs of 20 keys each.

    timeout -k 10 120 python tools/morph_motion_ab.py            (AB_ROUNDS=9 AB_ITERS=300)

One library per process: run it once with MMDX_LIB=<another build's libmmdx.so> and once without, alternating, to compare two
builds (the rows are tagged "parent" when MMDX_LIB is set).  Nothing here is a pass / fail number."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from simple_mmd_renderer_amd import _capi as api, synth, vmd  # noqa: E402
from simple_mmd_renderer_amd.engine import DeformModel, DeviceBuffer  # noqa: E402

NI, NM = 1024, 52
rounds, iters = int(os.environ.get("AB_ROUNDS", "9")), int(os.environ.get("AB_ITERS", "300"))
lib = api.lib()
names = [f"m{i}" for i in range(NM)]
keys = [(n, f * 30, float((f * 7 + i) % 10) / 10) for i, n in enumerate(names) for f in range(20)]
v = vmd.Vmd(vmd.write_vmd([], keys))
mm = v.bind_morphs(names)
dm = DeformModel(synth.make_model(64, 3, 1, 8, seed=5))
frames = (np.arange(NI, dtype=np.uint32) * 3) % 600
times = frames.astype(np.float64) / 30
out = np.zeros((NI, NM), np.float32)
d_fr, d_t, d_out = (DeviceBuffer.from_numpy(a) for a in (frames, times, out))
FR, OUT = vmd.FRAMES_ON_DEVICE, api.OUT_ON_DEVICE
rows = [("eval       host clock, host out", lib.mmdx_morph_motion_eval, frames.ctypes.data, 0, out.ctypes.data),
        ("eval_time  host clock, host out", lib.mmdx_morph_motion_eval_time, times.ctypes.data, 0, out.ctypes.data),
        ("eval       host clock, dev out ", lib.mmdx_morph_motion_eval, frames.ctypes.data, OUT, d_out.ptr),
        ("eval       device operands     ", lib.mmdx_morph_motion_eval, d_fr.ptr, FR | OUT, d_out.ptr),
        ("eval_time  device operands     ", lib.mmdx_morph_motion_eval_time, d_t.ptr, FR | OUT, d_out.ptr)]
res = {r[0]: [] for r in rows}
for rnd in range(rounds + 1):
    for name, fn, clock, flags, o in rows:
        dm.sync()
        t0 = time.perf_counter()
        for _ in range(iters):
            st = fn(mm.h, dm.h, NI, clock, flags, o)
        dm.sync()
        dt = (time.perf_counter() - t0) / iters * 1e6
        assert st == 0
        if rnd:
            res[name].append(dt)
tag = "parent" if os.environ.get("MMDX_LIB") else "new   "
for name, xs in res.items():
    print(f"{tag} {name}: median {np.median(xs):8.2f} us  min {min(xs):8.2f}  max {max(xs):8.2f}", flush=True)

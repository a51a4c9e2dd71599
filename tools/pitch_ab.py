#!/usr/bin/env python3
"""Interleaved A/B of dense against pitched crowd outputs (MMDX_OUT_PITCHED) in ONE process: config-3-shaped crowds (300 bones,
200 morphs, 2048 morph entries, 1 024 instances, shared rates, every operand in HBM) at vertex counts around 50 000, median of R
rounds.

    python tools/pitch_ab.py            (AB_ROUNDS=7 AB_ITERS=40 AB_TRIES=16)

Rows: NV = 50 000 dense (the reference: BASELINE config 3 itself, every instance starts 16-byte aligned); NV = 50 001 / 50 002 /
50 003 dense (instance i starts at i * NV: the generic copy-out) and pitched (pitch = mmdx_model_output_pitch: the 16-byte
copy-out); an f16-position row and a 32-byte-vertex row at NV = 50 003.  The odd-NV models are config 3 with its first 1-3
vertices appended once more, so that the rows differ in the vertex count alone (synth.make_model draws a different model for
every NV).  Each form runs with the store flavour the placement probe chose (MMDX_OUT_STORES_*) and, as "/other", with the other
one.  The dense and the pitched call of one NV write into the SAME arrays
(allocated once, pitched, through mmdx_crowd_output_alloc_pitched with its placement probe) so that the placement cancels out;
that allocation's placement info is printed with the row.  Per row: ms per step (morph pass + deform kernel, the rates found
unchanged on the device as in bench.py), the deform kernel alone (MMDX_MORPH_UNCHANGED), and the kernel's fraction of 8 TB/s
on algorithmic bytes -- the bytes actually written (NV vertices per instance, never the gap) plus the model's streams read."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from simple_mmd_renderer_amd import _capi as api, synth  # noqa: E402
from simple_mmd_renderer_amd.crowd import crowd_frames  # noqa: E402
from simple_mmd_renderer_amd.engine import DeformModel, DeviceBuffer  # noqa: E402

PEAK_GBS = 8000.0                                         # MI355X HBM3E spec peak, as bench.py
OUT_BPV = {api.OUT_SOA: 24, api.OUT_VERTEX32: 32, api.OUT_SOA_POS16: 18}
LAYOUT_NAME = {api.OUT_SOA: "soa", api.OUT_VERTEX32: "v32", api.OUT_SOA_POS16: "f16"}


def kernel_bytes(dm, layout, ni):
    """bench.py's algorithmic_bytes_config3 (deform kernel part) with the layout's output bytes: static streams + the shared
    morphed positions + per instance its NV written vertices and its palette; the 32-byte vertex also reads the uv stream."""
    i, nv = dm.info, dm.nv
    static = nv * (12 + 12 + 1) + i.n_bdef1 * 2 + i.n_bdef2 * 8 + i.n_bdef4 * 24
    b = static + nv * 12 + ni * (nv * OUT_BPV[layout] + dm.nb * 48)
    return b + (nv * 8 if layout == api.OUT_VERTEX32 else 0)


def grown(m, extra):
    """The model with its first `extra` vertices appended once more (same bones, same morph table)."""
    g = m.copy()
    for k in ("positions", "normals", "uvs", "skin_type", "bone_ids", "bone_weights", "sdef"):
        a = getattr(g, k)
        if a is not None:
            setattr(g, k, np.concatenate([a, a[:extra]]))
    return g


def main():
    rounds, iters = int(os.environ.get("AB_ROUNDS", "7")), int(os.environ.get("AB_ITERS", "40"))
    tries = int(os.environ.get("AB_TRIES", "16"))
    ni = 1024
    cases = [(50000, api.OUT_SOA), (50001, api.OUT_SOA), (50002, api.OUT_SOA), (50003, api.OUT_SOA),
             (50003, api.OUT_SOA_POS16), (50003, api.OUT_VERTEX32)]
    setups = []
    c3 = synth.make_config("config3_crowd")
    # every SoA row writes into ONE pair of arrays (sized for the widest pitch below), so that the placement cancels out across
    # the SoA rows, the NV = 50 000 reference included; the f16 and the 32-byte-vertex rows have arrays of their own
    soa_arrays = None
    for nv, layout in cases:
        m = grown(c3, nv - c3.nv)
        dm = DeformModel(m, f16_positions=layout == api.OUT_SOA_POS16)
        pitch = dm.output_pitch(layout)
        # NV = 50 003, SoA: also pitches that start every instance on a 64-byte (50 032) and a 128-byte (50 048) boundary
        extra = [("pitch64", 50032), ("pitch128", 50048)] if (nv, layout) == (50003, api.OUT_SOA) else []
        if layout == api.OUT_SOA and soa_arrays is not None:
            d_a, d_b, pl = soa_arrays
        else:
            d_a, d_b, pl = dm.alloc_outputs(layout, ni, tries, pitch=50048 if layout == api.OUT_SOA else pitch)
            if layout == api.OUT_SOA:
                soa_arrays = (d_a, d_b, pl)
            print(f"{LAYOUT_NAME[layout]} arrays (NV={nv}): placement {pl}", flush=True)
        d_pal = DeviceBuffer.from_numpy(synth.make_palettes(m, crowd_frames(0, ni)))
        d_w = DeviceBuffer.from_numpy(synth.morph_weights(m.nm, 30)[0])
        base = api.PALETTE_ON_DEVICE | api.WEIGHTS_ON_DEVICE | api.OUT_ON_DEVICE | api.WEIGHTS_SHARED | pl["store_flags"]
        other = (api.OUT_STORES_CACHED if pl["store_flags"] == api.OUT_STORES_WRITE_THROUGH else api.OUT_STORES_WRITE_THROUGH)
        keep = base & ~(api.OUT_STORES_CACHED | api.OUT_STORES_WRITE_THROUGH)
        forms = [(f, p, fl) for f, p in [("dense", 0)] + ([("pitched", pitch)] if pitch != nv else []) + extra
                 for f, fl in ((f, base), (f + "/other", keep | other))]
        setups.append((nv, layout, dm, d_a, d_b, d_pal, d_w, base, forms))
    res = {}
    for r in range(rounds + 1):
        for nv, layout, dm, d_a, d_b, d_pal, d_w, base, forms in setups:
            scale = 0.1 if layout == api.OUT_VERTEX32 else 1.0
            for form, pitch, ff in forms:
                for what, fl in (("step", ff), ("kernel", ff | api.MORPH_UNCHANGED)):
                    def run():
                        dm.deform_batched_raw(ni, d_w.ptr, d_pal.ptr, d_a.ptr, d_b.ptr if d_b else None, layout, fl, scale, pitch)
                    for _ in range(5):
                        run()
                    dm.sync()
                    t0 = time.perf_counter()
                    for _ in range(iters):
                        run()
                    dm.sync()
                    if r >= 1:                                # round 0 warms every row up
                        res.setdefault((nv, layout, form, what), []).append((time.perf_counter() - t0) / iters * 1e3)
                    res[(nv, layout, form, "stores")] = dm.last_store_policy()
    ref = None
    print(f"{'row':34s} {'step ms':>9s} {'kernel ms':>10s} {'kernel frac':>11s} {'vs 50000':>9s}   (median of {rounds}; min-max kernel; stores)")
    for nv, layout, dm, d_a, d_b, d_pal, d_w, base, forms in setups:
        for form, _, _ in forms:
            st, kn = res[(nv, layout, form, "step")], res[(nv, layout, form, "kernel")]
            frac = kernel_bytes(dm, layout, ni) / (np.median(kn) * 1e-3) / 1e9 / PEAK_GBS
            if ref is None:
                ref = frac
            name = f"NV={nv} {LAYOUT_NAME[layout]} {form}"
            print(f"{name:34s} {np.median(st):9.4f} {np.median(kn):10.4f} {frac:11.4f} {frac / ref:9.3f}   "
                  f"({min(kn):.4f}-{max(kn):.4f}; {res[(nv, layout, form, 'stores')]})", flush=True)
    for s in setups:
        for b in s[3:7]:
            if b is not None and b.ptr:
                b.free()
        s[2].close()


if __name__ == "__main__":
    main()

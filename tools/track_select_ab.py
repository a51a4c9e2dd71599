#!/usr/bin/env python3
"""Interleaved A/B of the three *_blend_*_time_select calls against the plain cross-fade calls on the workload of
tools/motion_set_ab.py: 300 bones + 200 morphs, a set of 8 clips (20 keys per bone over 600 frames, 12 keys per morph) assigned at
random, a third of the crowd mid-fade, every operand in HBM.  HIP events around AB_ITERS back-to-back calls, median of AB_ROUNDS
rounds after one warm-up round, min-max over the rounds next to it, at NI = 1 024 and 16 384.

    timeout -k 10 600 python tools/track_select_ab.py [parent/libmmdx.so]      (AB_ROUNDS=7 AB_ITERS=100 AB_ITERS_IK=4 AB_SIZES=1024,16384)

Calls: bones (mmdx_motion_set_blend_bones_time), morphs (_blend_morphs_time), fk (mmdx_skeleton_solve_motion_set_blend_time on the
parallel-FK rig: one launch) and ik (the same on tools/rig_bench.py's IK rig with 8 chains: blend, then the ordered solve).
Rows, per call and size:
  (a) the plain call, this library
  (b) the plain call, the parent commit's library (the argument; left out without it) -- measured by child processes of this tool
      (MMDX_LIB), one per round and library, alternating with children that measure (a) the same way: (a') / (b)
  (c) select of all NI, ascending order
  (d) select of NI/16, scattered (a seeded random subset, unsorted), capacity NI/16
  (e) the plain call on a dense crowd of NI/16: the SAME instances' operands packed into NI/16 rows
  (f) select with n_ids = NI and *count = 64
Printed at the end: (a')/(b) with (b)'s run-to-run spread -- the existing path did not move when the median of (a') lies inside the
min-max of (b)'s rounds; (d)/(e), the price of the indirection, reported, not gated; (d)/(a), which must be below 1; (c)/(a)."""
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from simple_mmd_renderer_amd import synth, vmd  # noqa: E402
from simple_mmd_renderer_amd.engine import DeformModel, DeviceBuffer  # noqa: E402

NB, NM, NCLIPS = 300, 200, 8
CALLS = ("bones", "morphs", "fk", "ik")
NEW = ("mmdx_motion_set_blend_bones_time_select", "mmdx_motion_set_blend_morphs_time_select",
       "mmdx_skeleton_solve_motion_set_blend_time_select")
med = lambda x: float(np.median(x))                    # noqa: E731
span = lambda x: "%.4f-%.4f" % (np.min(x), np.max(x))  # noqa: E731


def sizes():
    return [int(s) for s in os.environ.get("AB_SIZES", "1024,16384").split(",")]


def iters_of(call):
    return int(os.environ.get("AB_ITERS_IK", "4")) if call == "ik" else int(os.environ.get("AB_ITERS", "100"))


def make_clip(seed, names, mnames):
    rng = np.random.RandomState(seed)
    mk = [(n, int(f), float(np.float32(rng.uniform(0, 1)))) for n in mnames for f in sorted(rng.choice(600, 12, replace=False))]
    return vmd.Vmd(vmd.write_vmd(synth.make_bone_keys(names, seed, keys_per=20, span=600), mk))


def operands(ni):
    """8 clips at random on both sides, times with sub-frame offsets, a third of the crowd mid-fade (the others at weight 0)."""
    rng = np.random.default_rng(2026 + ni)
    ca, cb = rng.integers(0, NCLIPS, ni).astype(np.uint32), rng.integers(0, NCLIPS, ni).astype(np.uint32)
    ta = ((np.arange(ni) * 7) % 600) / 30.0 + (np.arange(ni) % 5) / 144.0
    tb = ((np.arange(ni) * 11) % 600) / 30.0 + (np.arange(ni) % 3) / 144.0
    w = np.where(rng.random(ni) < 1 / 3, rng.uniform(0.05, 0.95, ni), 0.0).astype(np.float32)
    return ca, ta, cb, tb, w


def upload(ops):
    return [DeviceBuffer.from_numpy(np.ascontiguousarray(a, t)) for a, t in
            zip(ops, (np.uint32, np.float64, np.uint32, np.float64, np.float32))]


def setup():
    """The stream and the timers (a small model), the set of 8 clips and the two rigs."""
    dm = DeformModel(synth.make_model(120, 4, 2, 10, seed=1))
    names, mnames = [f"b{i}" for i in range(NB)], [f"m{i}" for i in range(NM)]
    vs = [make_clip(303 + c, names, mnames) for c in range(NCLIPS)]
    bms, mms = [v.bind_bones(names) for v in vs], [v.bind_morphs(mnames) for v in vs]
    ms = vmd.MotionSet(bms, mms)
    rig = synth.make_ik_rig(NB, 3003, n_ik=8, n_append=12, post_physics=0.0, levels=1)
    rigs = {"ik": vmd.Skeleton(*rig), "fk": vmd.Skeleton(rig[0], rig[1])}
    assert rigs["fk"].info["solver"] == vmd.SOLVER_PARALLEL_FK and rigs["ik"].info["solver"] == vmd.SOLVER_SERIAL
    return dm, ms, rigs


def timed(dm, run, iters):
    for _ in range(3):
        run()
    dm.sync()
    dm.timer_start()
    for _ in range(iters):
        run()
    return dm.timer_stop() / iters


def plain_rows(dm, ms, rigs, n, ptrs, out):
    """The plain call of every kind over n instances whose operands are at ptrs, the outputs in the buffers of `out`."""
    return {"bones": lambda: ms.blend_bones_time_device(n, *ptrs, out["pose"].ptr, dm),
            "morphs": lambda: ms.blend_morphs_time_device(n, *ptrs, out["rate"].ptr, dm),
            "fk": lambda: rigs["fk"].solve_motion_set_blend_time_device(ms, n, *ptrs, out["pal"].ptr, dm),
            "ik": lambda: rigs["ik"].solve_motion_set_blend_time_device(ms, n, *ptrs, out["pal"].ptr, dm)}


def select_rows(dm, ms, rigs, n, ptrs, out, ids, n_ids, count):
    lst = dict(ids_ptr=ids.ptr, n_ids=n_ids, count_ptr=count.ptr, model=dm)
    return {"bones": lambda: ms.blend_bones_time_select_device(n, *ptrs, out["pose"].ptr, **lst),
            "morphs": lambda: ms.blend_morphs_time_select_device(n, *ptrs, out["rate"].ptr, **lst),
            "fk": lambda: rigs["fk"].solve_motion_set_blend_time_select_device(ms, n, *ptrs, out["pal"].ptr, **lst),
            "ik": lambda: rigs["ik"].solve_motion_set_blend_time_select_device(ms, n, *ptrs, out["pal"].ptr, **lst)}


def outputs(ni):
    return {"pose": DeviceBuffer(ni * NB * 32), "rate": DeviceBuffer(ni * NM * 4), "pal": DeviceBuffer(ni * NB * 64)}


def child():
    """One round of the plain calls at every size with whatever library MMDX_LIB names: one JSON line."""
    if os.environ.get("MMDX_LIB"):                           # the parent's library has no select entry points to bind
        from simple_mmd_renderer_amd import _capi
        for name in NEW:
            _capi.SIGNATURES.pop(name, None)
    dm, ms, rigs = setup()
    res = {}
    for ni in sizes():
        ds, out = upload(operands(ni)), outputs(ni)
        for call, run in plain_rows(dm, ms, rigs, ni, [d.ptr for d in ds], out).items():
            res["%s/%d" % (call, ni)] = timed(dm, run, iters_of(call))
        for d in ds + list(out.values()):
            d.free()
    print("CHILD " + json.dumps(res), flush=True)


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        return child()
    parent_lib = os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else None
    rounds = int(os.environ.get("AB_ROUNDS", "7"))
    dm, ms, rigs = setup()
    res = {}
    for ni in sizes():
        k = ni // 16
        ops = operands(ni)
        sub = np.random.default_rng(ni).permutation(ni)[:k].astype(np.uint32)
        ds, dense = upload(ops), upload([a[sub] for a in ops])
        out = outputs(ni)
        d_all, d_sub = DeviceBuffer.from_numpy(np.arange(ni, dtype=np.uint32)), DeviceBuffer.from_numpy(sub)
        d_n = {n: DeviceBuffer.from_numpy(np.array([n], np.uint32)) for n in (ni, k, 64)}
        ptrs, dptrs = [d.ptr for d in ds], [d.ptr for d in dense]
        rows = {"a": plain_rows(dm, ms, rigs, ni, ptrs, out),
                "c": select_rows(dm, ms, rigs, ni, ptrs, out, d_all, ni, d_n[ni]),
                "d": select_rows(dm, ms, rigs, ni, ptrs, out, d_sub, k, d_n[k]),
                "e": plain_rows(dm, ms, rigs, k, dptrs, out),
                "f": select_rows(dm, ms, rigs, ni, ptrs, out, d_all, ni, d_n[64])}
        for r in range(rounds + 1):
            for call in CALLS:
                for row in rows:                             # a, c, d, e, f back to back inside a round: interleaved
                    ms_per = timed(dm, rows[row][call], iters_of(call))
                    if r >= 1:                               # round 0 warms every row up
                        res.setdefault((call, ni, row), []).append(ms_per)
        for d in ds + dense + list(out.values()) + [d_all, d_sub] + list(d_n.values()):
            d.free()
    # (a') and (b): the plain calls in child processes, this library and the parent's alternating, one process at a time
    if parent_lib:
        for r in range(rounds + 1):
            for key, lib in (("a'", None), ("b", parent_lib)):
                env = dict(os.environ)
                env.pop("MMDX_LIB", None)
                if lib:
                    env["MMDX_LIB"] = lib
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=env, capture_output=True, text=True,
                                   timeout=120)
                line = [l for l in p.stdout.splitlines() if l.startswith("CHILD ")]
                if p.returncode != 0 or not line:
                    sys.stderr.write(p.stdout + p.stderr)
                    raise SystemExit("child run failed (%s)" % key)
                if r >= 1:
                    for name, v in json.loads(line[0][6:]).items():
                        call, ni = name.split("/")
                        res.setdefault((call, int(ni), key), []).append(v)
    what = {"a": "plain NI (this library)", "a'": "plain NI, child process (this library)", "b": "plain NI, child process (parent library)",
            "c": "select NI of NI, ascending", "d": "select NI/16 of NI, scattered", "e": "plain, dense crowd of the same NI/16",
            "f": "select, n_ids NI, *count 64"}
    print(f"{'call':7s} {'NI':>6s} {'row':5s} {'':42s} {'ms per call':>12s}   (median of {rounds}; min-max)")
    for call in CALLS:
        for ni in sizes():
            for row in ("a", "a'", "b", "c", "d", "e", "f"):
                if (call, ni, row) in res:
                    v = res[(call, ni, row)]
                    print(f"{call:7s} {ni:6d} ({row:2s}) {what[row]:42s} {med(v):12.4f}   ({span(v)})", flush=True)
    for call in CALLS:
        for ni in sizes():
            a, c, d, e = (np.array(res[(call, ni, row)]) for row in "acde")
            print(f"{call} {ni}: (d)/(a) = {med(d) / med(a):.3f} {'(below 1)' if med(d) < med(a) else '(NOT below 1: a finding)'}; "
                  f"(d)/(e) = {med(d) / med(e):.3f} (per round {span(d / e)}): the indirection, reported not gated; "
                  f"(c)/(a) = {med(c) / med(a):.3f}")
            if parent_lib:
                a2, b = np.array(res[(call, ni, "a'")]), np.array(res[(call, ni, "b")])
                ok = b.min() <= med(a2) <= b.max()
                print(f"{call} {ni}: (a')/(b) = {med(a2) / med(b):.4f}; median (a') {med(a2):.4f} ms against (b)'s rounds {span(b)} ms "
                      f"(spread {b.min() / med(b):.3f}-{b.max() / med(b):.3f} of its median): "
                      f"{'inside the spread' if ok else 'OUTSIDE the spread'}")


if __name__ == "__main__":
    main()

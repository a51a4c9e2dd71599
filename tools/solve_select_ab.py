#!/usr/bin/env python3
"""Interleaved A/B of mmdx_skeleton_solve_select against the plain mmdx_skeleton_solve on the palette producers' benchmark rigs
(1 024 instances x 300 bones: tools/rig_bench.py's IK rig with 8 chains, and its FK rig), every operand in HBM, the poses those of
the benchmark motion at every instance's own frame.  HIP events around AB_ITERS back-to-back calls, median of AB_ROUNDS rounds
after one warm-up round, min-max over the rounds next to it.

    timeout -k 10 900 python tools/solve_select_ab.py [parent/libmmdx.so]      (AB_ROUNDS=7 AB_ITERS_IK=10 AB_ITERS_FK=200)

Rows, per rig:
  (a) the plain solve of 1 024, this library
  (b) the plain solve of 1 024, the parent commit's library (the argument; left out without it) -- measured by child processes of
      this tool (MMDX_LIB), one per round and library, alternating with children that measure (a) the same way: (a') / (b)
  (c) select of all 1 024, ascending order
  (d) select of 256 of 1 024, scattered (a seeded random subset, unsorted), capacity 256
  (e) the plain solve of a dense crowd of 256: the SAME 256 instances' poses packed into 256 rows
  (f) select with n_ids = 1 024 and *count = 64
Two conditions are printed at the end: (a')/(b) -- the existing path did not move: the median of (a') must lie inside the min-max of
(b)'s rounds -- and (d)/(e), the price of the indirection, which is reported, not gated."""
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from simple_mmd_renderer_amd import synth, vmd  # noqa: E402
from simple_mmd_renderer_amd.engine import DeformModel, DeviceBuffer  # noqa: E402

NI, NB, K = 1024, 300, 256
med = lambda x: float(np.median(x))                    # noqa: E731
span = lambda x: "%.4f-%.4f" % (np.min(x), np.max(x))  # noqa: E731


def setup():
    """The stream and the timers (a small model), the two rigs, and the benchmark motion's poses of 1 024 instances in HBM."""
    dm = DeformModel(synth.make_model(120, 4, 2, 10, seed=1))
    names = [f"b{i}" for i in range(NB)]
    bm = vmd.Vmd(vmd.write_vmd(synth.make_bone_keys(names, 303, keys_per=20, span=600), [])).bind_bones(names)
    rig = synth.make_ik_rig(NB, 3003, n_ik=8, n_append=12, post_physics=0.0, levels=1)
    rigs = {"ik": vmd.Skeleton(*rig), "fk": vmd.Skeleton(rig[0], rig[1])}
    d_fr = DeviceBuffer.from_numpy(((np.arange(NI) * 7) % 600).astype(np.uint32))
    d_pose = DeviceBuffer(NI * NB * 32)
    bm.eval_device(NI, d_fr.ptr, d_pose.ptr, dm)
    dm.sync()
    return dm, rigs, d_pose


def timed(dm, run, iters):
    for _ in range(3):
        run()
    dm.sync()
    dm.timer_start()
    for _ in range(iters):
        run()
    return dm.timer_stop() / iters


def iters_of(name):
    return int(os.environ.get("AB_ITERS_IK", "10")) if name == "ik" else int(os.environ.get("AB_ITERS_FK", "200"))


def child():
    """One round of the plain solve of 1 024 on both rigs with whatever library MMDX_LIB names: one JSON line."""
    if os.environ.get("MMDX_LIB"):                           # the parent's library has no select entry point to bind
        from simple_mmd_renderer_amd import _capi
        _capi.SIGNATURES.pop("mmdx_skeleton_solve_select", None)
    dm, rigs, d_pose = setup()
    d_pal = DeviceBuffer(NI * NB * 64)
    out = {name: timed(dm, lambda: sk.solve_device(NI, d_pose.ptr, d_pal.ptr, dm), iters_of(name)) for name, sk in rigs.items()}
    print("CHILD " + json.dumps(out), flush=True)


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        return child()
    parent_lib = os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else None
    rounds = int(os.environ.get("AB_ROUNDS", "7"))
    dm, rigs, d_pose = setup()
    rng = np.random.default_rng(2026)
    sub = rng.permutation(NI)[:K].astype(np.uint32)
    poses = d_pose.download((NI, NB, 8), np.float32)
    d_dense = DeviceBuffer.from_numpy(poses[sub])
    d_pal = DeviceBuffer(NI * NB * 64)
    d_all, d_sub = DeviceBuffer.from_numpy(np.arange(NI, dtype=np.uint32)), DeviceBuffer.from_numpy(sub)
    d_n = {n: DeviceBuffer.from_numpy(np.array([n], np.uint32)) for n in (NI, K, 64)}
    res = {}
    for r in range(rounds + 1):
        for name, sk in rigs.items():
            it = iters_of(name)
            got = {
                "a": timed(dm, lambda: sk.solve_device(NI, d_pose.ptr, d_pal.ptr, dm), it),
                "c": timed(dm, lambda: sk.solve_select_device(NI, d_pose.ptr, d_pal.ptr, d_all.ptr, NI, d_n[NI].ptr, dm), it),
                "d": timed(dm, lambda: sk.solve_select_device(NI, d_pose.ptr, d_pal.ptr, d_sub.ptr, K, d_n[K].ptr, dm), it),
                "e": timed(dm, lambda: sk.solve_device(K, d_dense.ptr, d_pal.ptr, dm), it),
                "f": timed(dm, lambda: sk.solve_select_device(NI, d_pose.ptr, d_pal.ptr, d_all.ptr, NI, d_n[64].ptr, dm), it),
            }
            if r >= 1:                                       # round 0 warms every row up
                for k, v in got.items():
                    res.setdefault((name, k), []).append(v)
    # (a') and (b): the plain call in child processes, this library and the parent's alternating, one process at a time
    if parent_lib:
        for r in range(rounds + 1):
            for key, lib in (("a'", None), ("b", parent_lib)):
                env = dict(os.environ)
                env.pop("MMDX_LIB", None)
                if lib:
                    env["MMDX_LIB"] = lib
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=env, capture_output=True, text=True,
                                   timeout=300)
                line = [l for l in p.stdout.splitlines() if l.startswith("CHILD ")]
                if p.returncode != 0 or not line:
                    sys.stderr.write(p.stdout + p.stderr)
                    raise SystemExit("child run failed (%s)" % key)
                if r >= 1:
                    for name, v in json.loads(line[0][6:]).items():
                        res.setdefault((name, key), []).append(v)
    what = {"a": "plain 1024 (this library)", "a'": "plain 1024, child process (this library)", "b": "plain 1024, child process (parent library)",
            "c": "select 1024 of 1024, ascending", "d": "select 256 of 1024, scattered", "e": "plain, dense crowd of the same 256",
            "f": "select, n_ids 1024, *count 64"}
    print(f"{'rig':4s} {'row':5s} {'':44s} {'ms per call':>12s}   (median of {rounds}; min-max)")
    for name in rigs:
        for k in ("a", "a'", "b", "c", "d", "e", "f"):
            if (name, k) in res:
                v = res[(name, k)]
                print(f"{name:4s} ({k:2s}) {what[k]:44s} {med(v):12.4f}   ({span(v)})", flush=True)
    for name in rigs:
        d, e, a, c = (np.array(res[(name, k)]) for k in ("d", "e", "a", "c"))
        print(f"{name}: (d)/(e) = {med(d) / med(e):.3f} (per round {span(d / e)}): the indirection, reported not gated; "
              f"(c)/(a) = {med(c) / med(a):.3f}; (d)/(a) = {med(d) / med(a):.3f}")
        if parent_lib:
            a2, b = np.array(res[(name, "a'")]), np.array(res[(name, "b")])
            ok = b.min() <= med(a2) <= b.max()
            print(f"{name}: (a')/(b) = {med(a2) / med(b):.4f}; median (a') {med(a2):.4f} ms against (b)'s rounds {span(b)} ms: "
                  f"{'PASS (inside the spread)' if ok else 'FAIL (outside the spread)'}")


if __name__ == "__main__":
    main()

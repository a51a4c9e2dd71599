#!/usr/bin/env python3
"""Interleaved A/B of mmdx_palette_reach (a set of four reaches: two arms, two legs) against mmdx_palette_aim on the same palettes,
mmdx_palette_place over all rows (the same arithmetic), a device-to-device copy of the bytes the reach moves and the same reach
through a device list, in ONE process, median of R rounds.

    timeout -k 10 600 python tools/reach_ab.py            (AB_ROUNDS=7 AB_ITERS=200 AB_SIZES=1024,16384)

Hypothesis, written before the first run: about the aim's time per subtree row moved; phase A's dependent square roots and divisions
dominate at 1 024 instances (so there the reach costs more per row than the aim, whose phase A is shorter), and at 16 384 the rows do.
What came of it (profiles/reach/reach_ab.txt): not confirmed at either size -- 0.32 of the aim's time per row at 1 024 instances, where
more was expected, and 1.28 at 16 384.

Shapes: 1 024 and 16 384 instances x 300 bones (tools/aim_ab.py's rig), four reaches on the subtrees of bones 3, 4, 5 and 6 (sizes
printed), the aim of tools/aim_ab.py on the subtree of bone 3, every operand in HBM.  Rows, in microseconds per call:
    reach         AB_ITERS back-to-back mmdx_palette_reach calls (device targets every 4 floats, two target arrays taken in turn so
                  that the limbs keep moving) between two synchronisations of the model's stream, host clock, so launch overhead is
                  included; and the same by HIP events (mmdx_timer_*)
    reach list    the same through a device list of every instance, host clock
    aim           mmdx_palette_aim, one 2-link aim, the planner's block, host clock and events
    place         mmdx_palette_place with MMDX_PLACE_MATRIX, in place, over all 300 rows of the same palettes, host clock and events
    copy          mmdx_bench_copy over the bytes the reach moves: per instance the subtrees' rows read and written, per reach the
                  rows of a, b and c read again (64 bytes each) and 16 bytes of target, HIP events
The palettes are uploaded afresh at the start of every round.  The ratios are printed below the table.  Nothing here is a pass /
fail number."""
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from simple_mmd_renderer_amd import _capi as api  # noqa: E402
from simple_mmd_renderer_amd import synth, vmd  # noqa: E402
from simple_mmd_renderer_amd.engine import AimSet, DeformModel, DeviceBuffer, ReachSet  # noqa: E402
from aim_ab import NB, PLACE_DEV, make_rig, subtree_sizes  # noqa: E402


def main():
    rounds, iters = int(os.environ.get("AB_ROUNDS", "7")), int(os.environ.get("AB_ITERS", "200"))
    sizes = [int(v) for v in os.environ.get("AB_SIZES", "1024,16384").split(",")]          # multiples of 1 024
    rng = np.random.default_rng(2033)
    parent, rest, _ = make_rig(rng)
    size = subtree_sizes(parent)
    limbs = [3, 4, 5, 6]                                                    # disjoint subtrees of the binary tree
    reaches = [dict(bones=(a, 2 * a + 1, 2 * (2 * (2 * a + 1) + 1) + 1), max_extension=0.98, pole=(0.0, 0.0, 1.0), keep_end_rotation=a >= 5)
               for a in limbs]                                              # c a grandchild of b: not its direct child; the legs keep the foot
    aim_root = int(np.argmin(np.abs(size[1:] - 100))) + 1
    dm = DeformModel(synth.make_model(64, NB, 0, 0, seed=3))
    sk = vmd.Skeleton(rest, parent)
    rset = ReachSet(sk, reaches)
    aset = AimSet(sk, [dict(links=[aim_root, 2 * (2 * aim_root + 1) + 1], shares=[0.5, 1.0], cos_limits=[0.9, 0.7])])
    n_rows, aim_rows = rset.info()["n_subtree_rows"], aset.info()["n_subtree_rows"]
    poses = np.zeros((64, NB, 8), np.float32)
    q = rng.normal(size=(64, NB, 4)) * 0.15 + np.array([0.0, 0.0, 0.0, 1.0])
    poses[:, :, 4:] = q / np.linalg.norm(q, axis=2, keepdims=True)
    chunk = np.ascontiguousarray(np.tile(sk.solve(poses, dm), (16, 1, 1)))  # 64 different instances, tiled over the crowd 1 024 at a time
    med = lambda x: float(np.median(x))                # noqa: E731
    for ni in sizes:
        d_pal = DeviceBuffer(ni * NB * 64)
        tgts = [np.concatenate([rng.uniform(-2, 2, (ni, 3)) + rest[3], np.ones((ni, 1))], axis=1).astype(np.float32) for _ in range(2)]
        d_tgt = [DeviceBuffer.from_numpy(t) for t in tgts]
        place = np.tile(np.eye(4, dtype=np.float32).reshape(16), (ni, 1))
        place[:, 12:15] = rng.uniform(-1e-3, 1e-3, (ni, 3))                 # next to the identity: the palettes stay where they are
        d_place = DeviceBuffer.from_numpy(place)
        d_ids = DeviceBuffer.from_numpy(np.arange(ni, dtype=np.uint32))
        sel = vmd.instance_select(d_ids.ptr, ni)
        moved = ni * (n_rows * 64 * 2 + len(limbs) * (3 * 64 + 16)) // 2
        d_src, d_dst = DeviceBuffer(moved), DeviceBuffer(moved)
        os.environ.pop("MMDX_AIM_BLOCK", None)
        print(f"\nNI={ni} NB={NB}, four reaches on the subtrees of bones {limbs} ({[int(size[a]) for a in limbs]} = {n_rows} rows), a 2-link aim "
              f"over {aim_rows} rows; the reach moves {2 * moved / 1e6:.1f} MB, the place {ni * NB * 128 / 1e6:.1f} MB", flush=True)
        turn = [0]

        def reach(select=None):
            turn[0] ^= 1
            rset.reach(dm, d_pal, d_tgt[turn[0]], select=select, n_instances=ni)

        def aim():
            turn[0] ^= 1
            aset.aim(dm, d_pal, d_tgt[turn[0]], n_instances=ni)

        def timed(run):
            for _ in range(5):
                run()
            dm.sync()
            t0 = time.perf_counter()
            for _ in range(iters):
                run()
            dm.sync()
            return (time.perf_counter() - t0) / iters * 1e6

        def by_events(run):
            dm.sync()
            dm.timer_start()
            for _ in range(iters):
                run()
            return dm.timer_stop() / iters * 1e3
        place_run = lambda: dm.place_palettes(ni, d_pal.ptr, d_place.ptr, d_pal.ptr, PLACE_DEV)        # noqa: E731
        res = {}
        for r in range(rounds + 1):
            dm.sync()
            for k in range(ni // 1024):
                d_pal.upload(chunk, k * chunk.nbytes)
            row = {}                                                            # every row back to back inside a round: interleaved
            row["reach"], row["reach_ev"] = timed(reach), by_events(reach)
            row["reach_list"] = timed(lambda: reach(select=sel))
            row["aim"], row["aim_ev"] = timed(aim), by_events(aim)
            row["place"], row["place_ev"] = timed(place_run), by_events(place_run)
            ms_avg = C.c_float(0)
            api.check(api.lib().mmdx_bench_copy(d_dst.ptr, d_src.ptr, moved, iters, C.byref(ms_avg)))
            row["copy"] = float(ms_avg.value) * 1e3
            if r >= 1:                                                          # round 0 warms every row up
                for k, us in row.items():
                    res.setdefault(k, []).append(us)
        assert np.isfinite(d_pal.download((1024, NB, 16), np.float32)).all()
        print(f"us per call, median of {rounds} rounds of {iters} calls (min-max of the rounds)")
        for k, text in (("reach", "reach, four reaches, host clock"), ("reach_ev", "reach, four reaches, HIP events"),
                        ("reach_list", "reach through a device list of every instance, host clock"),
                        ("aim", "aim, one 2-link aim, host clock"), ("aim_ev", "aim, one 2-link aim, HIP events"),
                        ("place", "mmdx_palette_place (matrix form, in place, all 300 rows), host clock"),
                        ("place_ev", "mmdx_palette_place, HIP events"),
                        ("copy", "device copy of the bytes the reach moves, HIP events")):
            print(f"{text:<75} {med(res[k]):9.2f} ({min(res[k]):.2f}-{max(res[k]):.2f})")
        per_row = (med(res["reach_ev"]) / n_rows) / (med(res["aim_ev"]) / aim_rows)
        print(f"ratios (events): reach / aim {med(res['reach_ev']) / med(res['aim_ev']):.2f}, per subtree row moved {per_row:.2f}; "
              f"reach / place {med(res['reach_ev']) / med(res['place_ev']):.2f}, / copy {med(res['reach_ev']) / med(res['copy']):.2f}; "
              f"list / plain {med(res['reach_list']) / med(res['reach']):.2f} (host clock)", flush=True)
        for d in [d_pal, d_place, d_ids, d_src, d_dst] + d_tgt:
            d.free()
    for x in (rset, aset, sk, dm):
        x.close()


if __name__ == "__main__":
    main()

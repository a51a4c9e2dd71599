#!/usr/bin/env python3
"""Interleaved A/B of mmdx_palette_aim at both block sizes against mmdx_palette_place on the same palette (the same arithmetic over
ALL rows), a device-to-device copy of the bytes it moves and the spring step that follows it, in ONE process, median of R rounds.

    timeout -k 10 600 python tools/aim_ab.py            (AB_ROUNDS=7 AB_ITERS=200 AB_SIZES=1024,16384)

Shapes: 1 024 and 16 384 instances x 300 bones, one 2-link aim whose subtree is about 100 bones (printed), every operand in HBM.
Rows, in microseconds per call:
    aim 16 / 64   AB_ITERS back-to-back mmdx_palette_aim calls with MMDX_AIM_BLOCK=16 / 64 (device targets every 4 floats, two target
                  arrays taken in turn so that the heads keep turning) between two synchronisations of the model's stream, host
                  clock, so launch overhead is included; and the same by HIP events (mmdx_timer_*)
    aim default   the block the planner chooses by itself (printed), host clock; and through a device list of every instance
    place         mmdx_palette_place with MMDX_PLACE_MATRIX, in place, over all 300 rows of the same palettes, host clock and events
    copy          mmdx_bench_copy over the bytes the aim moves: per instance the subtree's rows read and written, the two link rows
                  and the eye row read again (64 bytes each) and 16 bytes of target, HIP events
    springs       mmdx_spring_step, 12 chains x 8 joints, 4 colliders, on the same palettes, host clock
The palettes are uploaded afresh at the start of every round.  The ratios are printed below the table.  Nothing here is a pass /
fail number; the default block of csrc/aim_table.hpp's planner was chosen from the aim 16 / aim 64 rows."""
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from simple_mmd_renderer_amd import _capi as api  # noqa: E402
from simple_mmd_renderer_amd import synth, vmd  # noqa: E402
from simple_mmd_renderer_amd.engine import AimSet, DeformModel, DeviceBuffer, SpringSet  # noqa: E402

NB, N_CHAINS, N_JOINTS, N_COLLIDERS = 300, 12, 8, 4
BODY = NB - N_CHAINS * N_JOINTS
PLACE_DEV = api.PALETTE_ON_DEVICE | api.OUT_ON_DEVICE | api.PLACE_ON_DEVICE | api.PLACE_MATRIX


def make_rig(rng):
    """300 bones: a body of 204 (a binary tree below bone 0), then 12 chains of 8 hanging off bones 1..12 (tools/springs_ab.py's)."""
    parent = [-1] + [(b - 1) // 2 for b in range(1, BODY)]
    rest = [[0.0, 10.0, 0.0]] + [None] * (BODY - 1)
    for b in range(1, BODY):
        rest[b] = (np.array(rest[parent[b]]) + rng.uniform(-0.5, 0.5, 3)).tolist()
    chains = []
    for c in range(N_CHAINS):
        at, pos, chain = 1 + c, np.array(rest[1 + c]), []
        for _ in range(N_JOINTS):
            pos = pos + np.array([0.0, -0.3, 0.05]) + rng.uniform(-0.05, 0.05, 3)
            parent.append(at)
            rest.append(pos.tolist())
            at = len(parent) - 1
            chain.append(at)
        chains.append(chain)
    return np.array(parent, np.int32), np.array(rest, np.float32), chains


def subtree_sizes(parent):
    size = np.ones(len(parent), np.int64)
    for b in range(len(parent) - 1, 0, -1):          # (parent[b] < b)
        size[parent[b]] += size[b]
    return size


def main():
    rounds, iters = int(os.environ.get("AB_ROUNDS", "7")), int(os.environ.get("AB_ITERS", "200"))
    sizes = [int(v) for v in os.environ.get("AB_SIZES", "1024,16384").split(",")]          # multiples of 1 024
    rng = np.random.default_rng(2033)
    parent, rest, chains = make_rig(rng)
    size = subtree_sizes(parent)
    root = int(np.argmin(np.abs(size[1:] - 100))) + 1                       # the bone whose subtree is nearest to 100 bones
    second = 2 * (2 * root + 1) + 1                                         # a grandchild in the binary tree: not its direct child
    dm = DeformModel(synth.make_model(64, NB, 0, 0, seed=3))
    sk = vmd.Skeleton(rest, parent)
    aset = AimSet(sk, [dict(links=[root, second], shares=[0.5, 1.0], cos_limits=[0.9, 0.7])])
    n_rows = aset.info()["n_subtree_rows"]
    colliders = (np.arange(N_COLLIDERS, dtype=np.uint32), np.concatenate([rest[:N_COLLIDERS], np.full((N_COLLIDERS, 1), 0.4, np.float32)], axis=1))
    poses = np.zeros((64, NB, 8), np.float32)
    q = rng.normal(size=(64, NB, 4)) * 0.15 + np.array([0.0, 0.0, 0.0, 1.0])
    poses[:, :, 4:] = q / np.linalg.norm(q, axis=2, keepdims=True)
    chunk = np.ascontiguousarray(np.tile(sk.solve(poses, dm), (16, 1, 1)))  # 64 different instances, tiled over the crowd 1 024 at a time
    med = lambda x: float(np.median(x))                # noqa: E731
    for ni in sizes:
        sset = SpringSet(sk, chains, [20.0, 0.2, 1.0, 0.05], ni, colliders=colliders)
        d_pal = DeviceBuffer(ni * NB * 64)
        tgts = [np.concatenate([rng.uniform(-8, 8, (ni, 3)) + [0.0, 10.0, 0.0], np.ones((ni, 1))], axis=1).astype(np.float32) for _ in range(2)]
        d_tgt = [DeviceBuffer.from_numpy(t) for t in tgts]
        place = np.tile(np.eye(4, dtype=np.float32).reshape(16), (ni, 1))
        place[:, 12:15] = rng.uniform(-1e-3, 1e-3, (ni, 3))                 # next to the identity: the palettes stay where they are
        d_place = DeviceBuffer.from_numpy(place)
        d_dt = DeviceBuffer.from_numpy(np.array([1 / 60], np.float32))
        d_ids = DeviceBuffer.from_numpy(np.arange(ni, dtype=np.uint32))
        sel = vmd.instance_select(d_ids.ptr, ni)
        moved = ni * (n_rows * 64 * 2 + 3 * 64 + 16) // 2
        d_src, d_dst = DeviceBuffer(moved), DeviceBuffer(moved)
        os.environ.pop("MMDX_AIM_BLOCK", None)
        aset.aim(dm, d_pal, d_tgt[0], n_instances=ni)
        default_block = dm.last_launch_shape()["group"]
        print(f"\nNI={ni} NB={NB}, a 2-link aim (bones {root}, {second}) over a subtree of {n_rows} bones; the aim moves {2 * moved / 1e6:.1f} MB, "
              f"the place {ni * NB * 128 / 1e6:.1f} MB; the planner's block: {default_block}", flush=True)
        turn = [0]

        def aim(block=None, select=None):
            if block is None:
                os.environ.pop("MMDX_AIM_BLOCK", None)
            else:
                os.environ["MMDX_AIM_BLOCK"] = str(block)
            turn[0] ^= 1
            aset.aim(dm, d_pal, d_tgt[turn[0]], select=select, n_instances=ni)

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
        step = lambda: sset.step(d_pal, dt_ptr=d_dt.ptr, n_instances=ni, model=dm)                      # noqa: E731
        res = {}
        for r in range(rounds + 1):
            dm.sync()
            for k in range(ni // 1024):
                d_pal.upload(chunk, k * chunk.nbytes)
            row = {}
            for b in (16, 64):                                                  # every row back to back inside a round: interleaved
                row[f"aim{b}"], row[f"aim{b}_ev"] = timed(lambda: aim(b)), by_events(lambda: aim(b))
            row["aim_default"], row["aim_list"] = timed(aim), timed(lambda: aim(select=sel))
            row["place"], row["place_ev"] = timed(place_run), by_events(place_run)
            ms_avg = C.c_float(0)
            api.check(api.lib().mmdx_bench_copy(d_dst.ptr, d_src.ptr, moved, iters, C.byref(ms_avg)))
            row["copy"] = float(ms_avg.value) * 1e3
            row["springs"] = timed(step)
            if r >= 1:                                                          # round 0 warms every row up
                for k, us in row.items():
                    res.setdefault(k, []).append(us)
        assert np.isfinite(d_pal.download((1024, NB, 16), np.float32)).all()
        print(f"us per call, median of {rounds} rounds of {iters} calls (min-max of the rounds)")
        for k, text in (("aim16", "aim, MMDX_AIM_BLOCK=16, host clock"), ("aim16_ev", "aim, MMDX_AIM_BLOCK=16, HIP events"),
                        ("aim64", "aim, MMDX_AIM_BLOCK=64, host clock"), ("aim64_ev", "aim, MMDX_AIM_BLOCK=64, HIP events"),
                        ("aim_default", "aim, the planner's block, host clock"),
                        ("aim_list", "aim through a device list of every instance, host clock"),
                        ("place", "mmdx_palette_place (matrix form, in place, all 300 rows), host clock"),
                        ("place_ev", "mmdx_palette_place, HIP events"),
                        ("copy", "device copy of the bytes the aim moves, HIP events"),
                        ("springs", "spring step (12 chains x 8 joints, 4 colliders), host clock")):
            print(f"{text:<75} {med(res[k]):9.2f} ({min(res[k]):.2f}-{max(res[k]):.2f})")
        best = min(med(res["aim16_ev"]), med(res["aim64_ev"]))
        print(f"ratios: aim 16 / aim 64 {med(res['aim16']) / med(res['aim64']):.2f} (host clock) {med(res['aim16_ev']) / med(res['aim64_ev']):.2f} (events); "
              f"the faster aim / place {best / med(res['place_ev']):.2f}, / copy {best / med(res['copy']):.2f} (events); "
              f"aim default / springs {med(res['aim_default']) / med(res['springs']):.2f} (host clock)", flush=True)
        for d in [d_pal, d_place, d_dt, d_ids, d_src, d_dst] + d_tgt:
            d.free()
        sset.close()
    os.environ.pop("MMDX_AIM_BLOCK", None)
    for x in (aset, sk, dm):
        x.close()


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Interleaved A/B of mmdx_palette_sockets against the place call on the same crowd, a device-to-device copy of the bytes it moves
and the device-to-host copy of the palette array it replaces, in ONE process, median of R rounds.

    timeout -k 10 600 python tools/sockets_ab.py            (AB_ROUNDS=7 AB_ITERS=200)

Shapes: 1 024 and 16 384 instances x 300 bones (the config-3 model), socket sets of 1, 4 and 16 sockets without and with (pose-form)
offsets, every operand in HBM.  Rows, in microseconds per call:
    sockets     AB_ITERS back-to-back mmdx_palette_sockets calls between two synchronisations of the model's stream, host clock, so
                launch overhead is included; and the same by HIP events (mmdx_timer_*)
    place       mmdx_palette_place (pose form, in place) on the same crowd, host clock
    copy        mmdx_bench_copy over the bytes the sockets call moves (NI * NS * 64 read, the same written), HIP events
    d2h         mmdx_memcpy_d2h of the whole [NI][NB][16] palette array into pageable host memory, host clock: what an adopter pays
                today before computing a single socket on the CPU
Nothing here is a pass / fail number."""
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from simple_mmd_renderer_amd import _capi as api  # noqa: E402
from simple_mmd_renderer_amd import synth  # noqa: E402
from simple_mmd_renderer_amd.engine import DeformModel, DeviceBuffer, SocketSet  # noqa: E402

PLACE_DEV = api.PALETTE_ON_DEVICE | api.PLACE_ON_DEVICE | api.OUT_ON_DEVICE


def main():
    rounds, iters = int(os.environ.get("AB_ROUNDS", "7")), int(os.environ.get("AB_ITERS", "200"))
    m = synth.make_config("config3_crowd")
    nb = m.nb
    dm = DeformModel(m)
    rng = np.random.default_rng(2031)
    med = lambda x: float(np.median(x))                # noqa: E731
    for ni in (1024, 16384):
        nbytes = ni * nb * 64
        pal = np.tile(np.eye(4, dtype=np.float32).reshape(16), (ni, nb, 1))
        pal[..., 12:15] = rng.uniform(-10, 10, (ni, nb, 3))
        poses = np.zeros((ni, 8), np.float32)
        poses[:, 7] = 1.0                              # identity placements: 200 in-place calls keep the values
        d_pal, d_pose = DeviceBuffer.from_numpy(pal), DeviceBuffer.from_numpy(poses)
        host = np.empty_like(pal)
        print(f"\nNI={ni} NB={nb}; palette array {nbytes / 1e6:.1f} MB", flush=True)

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
        cases = []
        for ns in (1, 4, 16):
            bones = rng.integers(0, nb, ns).astype(np.uint32)
            rest = np.asarray(m.bone_pos, np.float32)[bones]
            off = np.zeros((ns, 8), np.float32)
            off[:, :3], off[:, 7] = rng.uniform(-1, 1, (ns, 3)), 1.0
            for offsets in (None, off):
                sset = SocketSet(dm, bones, rest, offsets)
                d_out = DeviceBuffer(ns * ni * 64)
                d_src = DeviceBuffer(ns * ni * 64)
                cases.append((ns, offsets is not None, sset, d_out, d_src))
        res = {}
        for r in range(rounds + 1):
            row = {}
            for ns, with_off, sset, d_out, d_src in cases:      # every row back to back inside a round: interleaved
                key = (ns, with_off)
                run = lambda s=sset, o=d_out: s.sockets(d_pal, o, n_instances=ni)          # noqa: E731
                row[("sockets",) + key] = timed(run)
                row[("sockets_ev",) + key] = by_events(run)
                ms_avg = C.c_float(0)
                api.check(api.lib().mmdx_bench_copy(d_out.ptr, d_src.ptr, ns * ni * 64, iters, C.byref(ms_avg)))
                row[("copy",) + key] = float(ms_avg.value) * 1e3
            row[("place",)] = timed(lambda: dm.place_palettes(ni, d_pal.ptr, d_pose.ptr, d_pal.ptr, PLACE_DEV))
            t0 = time.perf_counter()
            for _ in range(3):
                api.check(api.lib().mmdx_memcpy_d2h(host.ctypes.data, d_pal.ptr, nbytes))
            row[("d2h",)] = (time.perf_counter() - t0) / 3 * 1e6
            if r >= 1:                                          # round 0 warms every row up
                for k, us in row.items():
                    res.setdefault(k, []).append(us)
        print(f"us per call, median of {rounds} rounds of {iters} calls (min-max of the rounds)")
        print(f"{'NS':>3} {'offsets':>7} {'sockets, host clock':>22} {'sockets, HIP events':>22} {'copy of NS*NI*64 B':>22}")
        for ns, with_off, *_ in cases:
            k = (ns, with_off)
            cell = lambda name: "%8.2f (%.2f-%.2f)" % (med(res[(name,) + k]), min(res[(name,) + k]), max(res[(name,) + k]))          # noqa: E731
            print(f"{ns:>3} {'yes' if with_off else 'no':>7} {cell('sockets'):>22} {cell('sockets_ev'):>22} {cell('copy'):>22}")
        print(f"place (pose form, in place, whole palette array), host clock {med(res[('place',)]):9.2f} "
              f"({min(res[('place',)]):.2f}-{max(res[('place',)]):.2f})")
        print(f"device-to-host copy of the palette array (pageable), host clock {med(res[('d2h',)]):9.2f} "
              f"({min(res[('d2h',)]):.2f}-{max(res[('d2h',)]):.2f})", flush=True)
        for _, _, sset, d_out, d_src in cases:
            sset.close()
            d_out.free()
            d_src.free()
        d_pal.free()
        d_pose.free()
    dm.close()


if __name__ == "__main__":
    main()

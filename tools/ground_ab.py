#!/usr/bin/env python3
"""Interleaved A/B of mmdx_ground_place and mmdx_ground_targets (two feet) against a bare launch (mmdx_animator_advance on the same
crowd), mmdx_palette_sockets for the same two bones, and what the two calls replace -- placements and two sockets slabs read back,
the height field sampled on the host, ty and the targets uploaded -- in ONE process, median of R rounds.

    timeout -k 10 600 python tools/ground_ab.py            (AB_ROUNDS=7 AB_ITERS=200 AB_SIZES=1024,16384)

Hypothesis, written before the first run: both calls cost about a launch at both crowd sizes, as advance does (3.4-4.2 us in
profiles/animator/): 16 384 instances are 256 waves, one per CU, and every lane has a handful of loads in flight.  On a 4096 x 4096
field (64 MiB, far above an XCD's 4 MiB L2) with the instances scattered over it the four-corner gathers miss: expected to show at
16 384 instances, not at 1 024.
What came of it (profiles/ground/ground_ab.txt): the first held -- place 0.88 and 0.99 of advance, targets 1.02 and 1.03 --; the
second did not show: the big field costs what the small one does, but every call here samples the same points again, which the
caches keep, so a frame of all-new points is not what this measures.

Rows, in microseconds per call (host clock between two synchronisations of the model's stream, so launch overhead is included, and
HIP events where it says so):
    place            mmdx_ground_place with a drop, 33 x 17 field
    targets          mmdx_ground_targets, two feet from a sockets slab (strides 16 and NI*16), with out_drop, 33 x 17 field
    place / targets (4096^2)   the same on the 4096 x 4096 field, placements and feet scattered over all of it
    targets list     targets through a device list of every instance
    advance          mmdx_animator_advance with a device dt: a bare launch over the same crowd
    sockets          mmdx_palette_sockets for the two foot bones
    host round trip  d2h of [NI][8] placements and of the two slabs, h(x, z) of the numpy restatement's arithmetic vectorised on the
                     host for NI placements and 2 NI feet, h2d of the placements and of [2][NI][4] targets
Nothing here is a pass / fail number."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from simple_mmd_renderer_amd import synth, vmd  # noqa: E402
from simple_mmd_renderer_amd.engine import DeformModel, DeviceBuffer, Ground, SocketSet  # noqa: E402
from tools.motion_set_ab import NCLIPS, NM, make_clip  # noqa: E402

F = np.float32


def host_height(H, origin, cell, x, z):
    """h(x, z) as include/mmdx.h states it, vectorised in binary32: what an adopter's host code does per frame without the calls."""
    nz, nx = H.shape
    u = np.clip((x - F(origin[0])) / F(cell[0]), F(0), F(nx - 1))
    v = np.clip((z - F(origin[1])) / F(cell[1]), F(0), F(nz - 1))
    iu, iv = np.minimum(u.astype(np.int64), nx - 2), np.minimum(v.astype(np.int64), nz - 2)
    fu, fv = u - iu.astype(F), v - iv.astype(F)
    h00, h10, h01, h11 = H[iv, iu], H[iv, iu + 1], H[iv + 1, iu], H[iv + 1, iu + 1]
    lo = (h00 * ((F(1) - fu) - fv) + h10 * fu) + h01 * fv
    up = (h11 * ((fu + fv) - F(1)) + h10 * (F(1) - fv)) + h01 * (F(1) - fu)
    return np.where(fu + fv <= F(1), lo, up)


def main():
    rounds, iters = int(os.environ.get("AB_ROUNDS", "7")), int(os.environ.get("AB_ITERS", "200"))
    sizes = [int(v) for v in os.environ.get("AB_SIZES", "1024,16384").split(",")]
    m = synth.make_config("config3_crowd")
    names = [f"b{i}" for i in range(m.nb)]
    mnames = [f"m{i}" for i in range(NM)]
    dm = DeformModel(m)
    sk = vmd.Skeleton(m.bone_pos, np.asarray(m.bone_parent, np.int32))
    vs = [make_clip(303 + c, names, mnames) for c in range(NCLIPS)]
    bms, mms = [v.bind_bones(names) for v in vs], [v.bind_morphs(mnames) for v in vs]
    ms = vmd.MotionSet(bms, mms)
    feet = [m.nb - 1, m.nb - 2]
    sockets = SocketSet.from_skeleton(dm, sk, feet)
    rng = np.random.default_rng(2034)
    small_h = rng.uniform(-2, 2, (17, 33)).astype(F)
    big_h = rng.uniform(-2, 2, (4096, 4096)).astype(F)
    fields = {"33x17": (small_h, (-16.0, -8.0), (1.0, 1.0)), "4096^2": (big_h, (-2048.0, -2048.0), (1.0, 1.0))}
    grounds = {k: Ground(*v) for k, v in fields.items()}
    med = lambda x: float(np.median(x))                # noqa: E731
    for ni in sizes:
        an = vmd.Animator(ms, ni)
        an.set_state(dm, clips_a=rng.integers(0, NCLIPS, ni), clips_b=np.full(ni, vmd.CLIP_NONE), times_a=rng.uniform(0, 20, ni),
                     times_b=np.zeros(ni), weights=np.zeros(ni), fade_rate=np.zeros(ni), speed=np.ones(ni))
        d_dt = DeviceBuffer.from_numpy(np.array([1 / 60], np.float64))
        place, slabs = {}, {}
        for k, (h, origin, cell) in fields.items():                           # placements and feet scattered over the whole field
            span = np.array([h.shape[1] - 1, h.shape[0] - 1]) * np.array(cell)
            p = np.zeros((ni, 8), F)
            p[:, [0, 2]] = np.array(origin) + rng.uniform(0, 1, (ni, 2)) * span
            p[:, 7] = 1.0
            s = np.zeros((2, ni, 16), F)
            s[:, :, 12] = p[:, 0] + rng.uniform(-0.4, 0.4, (2, ni))
            s[:, :, 14] = p[:, 2] + rng.uniform(-0.4, 0.4, (2, ni))
            s[:, :, 13], s[:, :, 15] = rng.uniform(0, 0.3, (2, ni)), 1.0
            place[k], slabs[k] = DeviceBuffer.from_numpy(p), DeviceBuffer.from_numpy(s)
        d_pal = DeviceBuffer(ni * m.nb * 64)
        d_pal.memset(0)
        d_slab = DeviceBuffer(2 * ni * 64)
        d_tgt, d_drop = DeviceBuffer(2 * ni * 16), DeviceBuffer(ni * 4)
        d_drop.memset(0)
        d_ids = DeviceBuffer.from_numpy(np.arange(ni, dtype=np.uint32))
        sel = vmd.instance_select(d_ids.ptr, ni)
        host_p, host_s, host_t = np.empty((ni, 8), F), np.empty((2, ni, 16), F), np.ones((2, ni, 4), F)

        def do_place(k):
            grounds[k].place(dm, place[k], ni, drop=d_drop, y_offset=0.1)

        def do_targets(k, select=None):
            grounds[k].targets(dm, place[k], slabs[k].ptr + 48, d_tgt, ni, 2, out_drop=d_drop, max_step=0.5, max_drop=0.3, select=select)

        def round_trip():
            h, origin, cell = fields["33x17"]
            dm.sync()
            host_p[:] = place["33x17"].download((ni, 8), F)
            host_s[:] = slabs["33x17"].download((2, ni, 16), F)
            host_p[:, 1] = host_height(h, origin, cell, host_p[:, 0], host_p[:, 2]) + F(0.1)
            hf = host_height(h, origin, cell, host_s[:, :, 12], host_s[:, :, 14])
            host_t[:, :, 0], host_t[:, :, 2] = host_s[:, :, 12], host_s[:, :, 14]
            host_t[:, :, 1] = host_s[:, :, 13] + np.clip(hf - host_p[:, 1], F(-0.5), F(0.5))
            place["33x17"].upload(host_p)
            d_tgt.upload(host_t)
        rows = {"place": lambda: do_place("33x17"), "targets": lambda: do_targets("33x17"),
                "place (4096^2)": lambda: do_place("4096^2"), "targets (4096^2)": lambda: do_targets("4096^2"),
                "targets list": lambda: do_targets("33x17", sel),
                "advance": lambda: an.advance_device_dt(d_dt.ptr, dm),
                "sockets": lambda: sockets.sockets(d_pal, d_slab, n_instances=ni),
                "host round trip": round_trip}

        def timed(run, n):
            for _ in range(5):
                run()
            dm.sync()
            t0 = time.perf_counter()
            for _ in range(n):
                run()
            dm.sync()
            return (time.perf_counter() - t0) / n * 1e6

        def by_events(run):
            dm.sync()
            dm.timer_start()
            for _ in range(iters):
                run()
            return dm.timer_stop() / iters * 1e3
        res = {}
        for r in range(rounds + 1):
            row = {}                                                            # every row back to back inside a round: interleaved
            for name, run in rows.items():
                row[name] = timed(run, iters if name != "host round trip" else max(iters // 10, 5))
                if name != "host round trip":
                    row[name + ", events"] = by_events(run)
            if r >= 1:                                                          # round 0 warms every row up
                for k, us in row.items():
                    res.setdefault(k, []).append(us)
        assert np.isfinite(d_tgt.download((2, ni, 4), F)).all() and np.isfinite(d_drop.download((ni,), F)).all()
        print(f"\nNI={ni}, two feet; us per call, median of {rounds} rounds of {iters} calls (min-max of the rounds)", flush=True)
        for k in res:
            print(f"{k:<34} {med(res[k]):9.2f} ({min(res[k]):.2f}-{max(res[k]):.2f})")
        adv = med(res["advance"])
        print(f"ratios (host clock): place / advance {med(res['place']) / adv:.2f}, targets / advance {med(res['targets']) / adv:.2f}, "
              f"(place + targets) / host round trip {(med(res['place']) + med(res['targets'])) / med(res['host round trip']):.4f}; "
              f"4096^2 / 33x17: place {med(res['place (4096^2)']) / med(res['place']):.2f}, "
              f"targets {med(res['targets (4096^2)']) / med(res['targets']):.2f} (events: "
              f"{med(res['place (4096^2), events']) / med(res['place, events']):.2f}, "
              f"{med(res['targets (4096^2), events']) / med(res['targets, events']):.2f})", flush=True)
        for x in [an, d_dt, d_pal, d_slab, d_tgt, d_drop, d_ids] + list(place.values()) + list(slabs.values()):
            x.free() if isinstance(x, DeviceBuffer) else x.close()
    for x in list(grounds.values()) + [sockets, ms, sk, dm] + bms + mms + vs:
        x.close()


if __name__ == "__main__":
    main()

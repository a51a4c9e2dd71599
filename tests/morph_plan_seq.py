"""The scripted call sequences of tests/golden/morph_plan_sequences.json: what they are (SEQUENCES), how one runs on a GPU (run), and
how it reads to tests/morph_plan_driver.cpp (driver_lines).  Shared by tests/gen_morph_plan_golden.py, which records what a library
does with them, and tests/test_morph_plan.py, which holds the planner and the built library to that record.

A step is a dict: op "call" (a deform call), "record" (the same call into a graph; the step before it is the same call, un-recorded,
so that every scratch buffer has its size) or "replay" (of that graph).  A call has ni, rates (1 = A, 2 = B: one set of rates;
3 = a set of rates per instance), host (the rates are in host memory), shared / unchanged (MMDX_WEIGHTS_SHARED / MMDX_MORPH_UNCHANGED)
and sel (-1: no list, else mmdx_deform_batched_select with a host list of that many ids).  Palettes and outputs are device memory
throughout: the rates alone decide what the morph step does."""
import os

import numpy as np

from simple_mmd_renderer_amd import _capi as api
from simple_mmd_renderer_amd import synth
from simple_mmd_renderer_amd.engine import DeformModel, DeviceBuffer

MODELS = {
    "small": dict(args=[600, 8, 6, 40], seed=406, f16=False),
    "small_f16": dict(args=[600, 8, 6, 40], seed=406, f16=True),
    "big": dict(args=[900, 12, 8300, 2], seed=77, f16=False),            # past kMaxFusedSlots (8192) slots
}
MAX_NI = 12
RATE_FRAMES = {1: 30, 2: 47}


def call(ni, rates, host=False, shared=True, unchanged=False, sel=-1, op="call"):
    return dict(op=op, ni=ni, rates=rates, host=host, shared=shared, unchanged=unchanged, sel=sel)


def record(ni, rates):
    return call(ni, rates, op="record")


REPLAY = dict(op="replay")
A, B, PER = 1, 2, 3
host, dev = (lambda r, ni=12, **k: call(ni, r, host=True, **k)), (lambda r, ni=12, **k: call(ni, r, **k))
frame = lambda r: call(1, r, host=True, shared=False)                    # noqa: E731
per_instance = lambda ni=12, sel=-1: call(ni, PER, shared=False, sel=sel)  # noqa: E731

DEVICE_RATES = [dev(A), dev(A), dev(A), dev(B), dev(B), dev(A), dev(B, 4), dev(A), dev(A, unchanged=True), dev(A)]
HOST_RATES = [host(A), host(A), host(B), host(B), dev(A), host(B), dev(A), record(12, A), host(B), REPLAY, REPLAY, host(B)]
MIXED = [host(A), dev(A), host(A), host(A), host(B, unchanged=True), host(B), host(A, unchanged=True), host(B)]


def _seq(name, model, steps, **env):
    return dict(name=name, model=model, env={k: str(v) for k, v in env.items()}, steps=steps)


SEQUENCES = [
    # the five of tests/test_morph_autoskip.py
    _seq("device rates: unchanged skip the walk, changed rerun it", "small", DEVICE_RATES),
    _seq("host rates: unchanged skip the launch, other writers void the record", "small", HOST_RATES),
    _seq("past the fused flatten limit", "big", [host(A), host(A), host(A), dev(A), dev(A), host(A, 8), host(A, 8), host(B)]),
    _seq("f16 positions", "small_f16", [dev(A), dev(A), dev(A)]),
    _seq("autoskip off", "small", [host(A), host(A), host(A), dev(A), dev(A), dev(A, unchanged=True), dev(B, 4), host(B)],
         MMDX_MORPH_AUTOSKIP=0),
    # the boundary between a small crowd and a crowd
    _seq("8 and 9 instances", "small", [host(A, 8), host(A, 9), host(A, 9), dev(A, 8), dev(A, 9), dev(A, 8, unchanged=True),
                                        dev(A, 9, unchanged=True), host(B, 9), host(B, 8), host(B, 9)]),
    _seq("2 instances", "small", [host(A, 2), host(A, 2), host(A, 2, unchanged=True), dev(B, 2)]),
    # MMDX_SHARED_FUSED
    _seq("shared_fused 0: every crowd takes the pass", "small", [host(A, 2), host(A, 2), dev(A, 8), frame(B), host(A), dev(B, 4)],
         MMDX_SHARED_FUSED=0),
    _seq("shared_fused 2: every crowd gathers", "small", [host(A), dev(A), dev(A, unchanged=True), dev(A, sel=0), dev(A), host(B, 9)],
         MMDX_SHARED_FUSED=2),
    _seq("shared_fused 2 past the fused flatten limit", "big", [host(A), host(A), dev(B), dev(B, 4)], MMDX_SHARED_FUSED=2),
    _seq("device rates, shared_fused 0", "small", DEVICE_RATES, MMDX_SHARED_FUSED=0),
    _seq("device rates, shared_fused 2", "small", DEVICE_RATES, MMDX_SHARED_FUSED=2),
    _seq("device rates, autoskip off", "small", DEVICE_RATES, MMDX_MORPH_AUTOSKIP=0),
    _seq("host rates, shared_fused 0", "small", HOST_RATES, MMDX_SHARED_FUSED=0),
    _seq("host rates, shared_fused 2", "small", HOST_RATES, MMDX_SHARED_FUSED=2),
    _seq("host rates, autoskip off", "small", HOST_RATES, MMDX_MORPH_AUTOSKIP=0),
    _seq("host rates past the fused flatten limit", "big", HOST_RATES),
    # host and device rates in turn, the caller's promise in between
    _seq("host and device rates in turn", "small", MIXED),
    _seq("host and device rates in turn, autoskip off", "small", MIXED, MMDX_MORPH_AUTOSKIP=0),
    _seq("host and device rates in turn past the fused flatten limit", "big", MIXED),
    # select calls
    _seq("select, shared rates", "small", [dev(A, sel=0), dev(A, sel=9), dev(B, sel=9), dev(B, sel=0), dev(B, sel=1), dev(B),
                                           dev(A, sel=9, unchanged=True), dev(B, sel=9)]),
    _seq("select, per-instance rates", "small", [per_instance(sel=9), per_instance(sel=0), per_instance(sel=1), dev(A), per_instance(),
                                                 dev(A), per_instance(sel=9)]),
    _seq("select, small crowd", "small", [dev(A, 4, sel=0), dev(B, 4, sel=1), dev(B, 4, unchanged=True), dev(B), dev(A, 4, sel=4)]),
    _seq("select past the fused flatten limit", "big", [dev(A, sel=0), dev(A, sel=9), per_instance(sel=9), dev(A, sel=9)]),
    # the refusal
    _seq("unchanged without positions", "small", [dev(A, unchanged=True), frame(A), host(A, unchanged=True), per_instance(),
                                                  dev(A, unchanged=True), dev(B, 4), dev(A, unchanged=True), dev(A)]),
    # single frames leave the kept positions alone
    _seq("single frames between crowd calls", "small", [frame(A), host(A), frame(B), host(A), call(1, B, host=True, unchanged=True),
                                                        host(A), call(1, B), dev(A), dev(A)]),
    # replays (a host-rates call first: no scratch buffer may grow once a graph holds its address)
    _seq("replay of a small crowd", "small", [host(A), dev(A, 4), record(4, A), host(B), REPLAY, host(B), host(B), dev(B)]),
    _seq("replay past the fused flatten limit", "big", [host(A), dev(A), record(12, A), host(B), REPLAY, host(B), host(B)]),
    _seq("replay, then device rates", "small", [host(A), dev(B), record(12, B), dev(A), REPLAY, dev(B), REPLAY, dev(A), host(A)]),
]


def make_model(name):
    spec = MODELS[name]
    return synth.make_model(*spec["args"], seed=spec["seed"])


def model_scalars(name):
    """What the driver's launch planner needs of the model (a host-only handle: no GPU)."""
    with DeformModel(make_model(name), host_only=True, f16_positions=MODELS[name]["f16"]) as dm:
        return dict(ns=int(dm.info.n_slots), ntiles=int(dm.info.n_tiles), max_tile_bones=int(dm.info.max_tile_bones))


def select_ids(ni, n):
    """n ids of an ni-instance call: the first and the last instance first"""
    return ([0, ni - 1] + list(range(1, ni - 1)))[:n]


def driver_lines(seq, scalars):
    env = seq["env"]
    out = ["seq %d %d %d %s %s" % (scalars["ns"], scalars["ntiles"], scalars["max_tile_bones"], env.get("MMDX_SHARED_FUSED", "1"),
                                   env.get("MMDX_MORPH_AUTOSKIP", "1"))]
    for s in seq["steps"]:
        out.append("replay" if s["op"] == "replay" else
                   "%s %d %d %d %d %d %d" % (s["op"], s["ni"], s["rates"], s["host"], s["shared"], s["unchanged"], s["sel"]))
    return out


def check_final(oracle, final, what):
    """The first and the last instance of a sequence's last call, bit for bit against the oracle"""
    m, f16, rates, pals, got = final
    q = m
    if f16:                                                     # an f16-position model skins the rounded base positions and offsets
        q = m.copy()
        q.positions = m.positions.astype(np.float16).astype(np.float32)
        q.morph_value = m.morph_value.astype(np.float16).astype(np.float32)
    skin = oracle.normalize(q)
    for i, (a, b) in got.items():
        ep, en = oracle.skin(q, pals[i], oracle.morph(q, rates[i]), skin)
        if f16:
            assert np.array_equal(a.view(np.uint16), ep.astype(np.float16).view(np.uint16)), f"{what}: inst {i} pos"
        else:
            assert np.array_equal(a.view(np.uint32), ep.view(np.uint32)), f"{what}: inst {i} pos"
        assert np.array_equal(b.view(np.uint32), en.view(np.uint32)), f"{what}: inst {i} nrm"


def run(seq):
    """The sequence on the GPU.  Returns (rows, final): rows[i] = "refused" or dict(morph, kernel, stats) after step i; final = what the
    last step wrote: (model, f16, rates [ni][nm], palettes, {instance: (a, b)}) for the first and the last instance."""
    spec = MODELS[seq["model"]]
    m = make_model(seq["model"])
    pals = synth.make_palettes(m, np.arange(MAX_NI) * 3)
    rates = {k: synth.morph_weights(m.nm, f)[0] for k, f in RATE_FRAMES.items()}
    rates[PER] = synth.morph_weights(m.nm, np.arange(MAX_NI) * 9)
    layout = api.OUT_SOA_POS16 if spec["f16"] else api.OUT_SOA
    for k, v in seq["env"].items():
        os.environ[k] = v
    api.lib().mmdx_debug_reload_env()
    rows, graph, bufs = [], None, []
    try:
        with DeformModel(m, f16_positions=spec["f16"]) as dm:
            d_pal = DeviceBuffer.from_numpy(pals)
            d_w = {k: DeviceBuffer.from_numpy(v) for k, v in rates.items()}
            sa, sb = dm.out_sizes(layout, MAX_NI)
            d_a, d_b = DeviceBuffer(sa), DeviceBuffer(sb)
            bufs = [d_pal, d_a, d_b] + list(d_w.values())
            for s in seq["steps"]:
                if s["op"] == "replay":
                    graph.launch()
                    dm.sync()
                else:
                    w = rates[s["rates"]].ctypes.data if s["host"] else d_w[s["rates"]].ptr
                    flags = (api.PALETTE_ON_DEVICE | api.OUT_ON_DEVICE | (0 if s["host"] else api.WEIGHTS_ON_DEVICE) |
                             (api.WEIGHTS_SHARED if s["shared"] else 0) | (api.MORPH_UNCHANGED if s["unchanged"] else 0))
                    if s["op"] == "record":
                        dm.graph_begin()
                    else:
                        d_a.memset(0xFF); d_b.memset(0xFF)
                    try:
                        if s["sel"] >= 0:
                            dm.deform_batched_select(s["ni"], select_ids(s["ni"], s["sel"]), w, d_pal.ptr, d_a.ptr, d_b.ptr, layout, flags)
                        else:
                            dm.deform_batched_raw(s["ni"], w, d_pal.ptr, d_a.ptr, d_b.ptr, layout, flags)
                    except api.MmdxError as e:
                        assert "MMDX_MORPH_UNCHANGED without an earlier" in str(e), e
                        rows.append("refused")
                        continue
                    if s["op"] == "record":
                        graph = dm.graph_end()
                    dm.sync()
                shape = dm.last_launch_shape()
                rows.append(dict(morph=shape["morph"], kernel=shape["kernel"], stats=list(dm.morph_pass_stats())))
            last = seq["steps"][-1]
            assert last["op"] == "call" and not last["unchanged"] and (last["sel"] < 0 or last["sel"] >= 2) and rows[-1] != "refused", \
                "a sequence ends in a call that writes its first and last instance from rates of its own"
            ni = last["ni"]
            r = rates[PER][:ni] if last["rates"] == PER else np.tile(rates[last["rates"]], (ni, 1))
            wa = 6 if spec["f16"] else 12
            got = {i: (d_a.download((m.nv, 3), np.float16 if spec["f16"] else np.float32, offset=i * m.nv * wa),
                       d_b.download((m.nv, 3), np.float32, offset=i * m.nv * 12)) for i in (0, ni - 1)}
            if graph:
                graph.close()
    finally:
        for b in bufs:
            b.free()
        for k in seq["env"]:
            del os.environ[k]
        api.lib().mmdx_debug_reload_env()
    return rows, (m, spec["f16"], r, pals, got)

"""Per-instance bounds of crowd deformation (mmdx_deform_batched_bounds): the call writes exactly what mmdx_deform_batched writes and,
in addition, out_bounds[i] = {min x, min y, min z, max x, max y, max z} of instance i's positions AS WRITTEN (pos_scale applied,
binary16 widened, never the pitch gap), NaN skipped, where the outputs live.
CPU: the ABI (header, export, binding, unchanged struct size and version) and the bounds instantiations' resources.
GPU: every form against mmdx_deform_batched on the same inputs and numpy over the written positions."""
import ctypes as C
import os
import re
import subprocess
import sys
import warnings

import numpy as np
import pytest

from simple_mmd_renderer_amd import _capi as api
from simple_mmd_renderer_amd import synth
from simple_mmd_renderer_amd.engine import DeformModel, DeviceBuffer, PinnedArray, device_count

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mmdx.h")

BPV = {api.OUT_SOA: (12, 12), api.OUT_VERTEX32: (32, 0), api.OUT_SOA_POS16: (6, 12)}   # bytes per vertex of out_a, out_b
TAIL = 64                                                                            # sentinel bytes behind the last instance
DEV = api.PALETTE_ON_DEVICE | api.WEIGHTS_ON_DEVICE | api.OUT_ON_DEVICE


# ---- CPU: the ABI ----------------------------------------------------------------------------------------------------------------
def test_header_declares_bounds_entry_point_and_library_exports_it(hip_lib):
    text = open(HEADER).read()
    assert re.search(r"MMDX_API\s+mmdx_status\s+mmdx_deform_batched_bounds\s*\(\s*mmdx_model_t\s+model\s*,\s*"
                     r"const\s+mmdx_deform_args\s*\*\s*args\s*,\s*float\s*\*\s*out_bounds", text)
    assert hasattr(hip_lib, "mmdx_deform_batched_bounds")
    assert "mmdx_deform_batched_bounds" in api.SIGNATURES


def test_abi_version_and_args_size_unchanged(hip_lib):
    assert "#define MMDX_ABI_VERSION 3u" in open(HEADER).read()
    assert hip_lib.mmdx_abi_version() == 3
    assert C.sizeof(api.DeformArgs) == 56


def test_bounds_instantiations_have_no_spills(hip_lib):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), api.LIB_PATH],
                         capture_output=True, text=True, check=True).stdout.splitlines()
    rows = [l for l in out if re.match(r"deform_kernel<\d+, \d, \d, \w+, \w+, false, true>", l) or l.startswith("bounds_reduce_kernel")]
    # 2 block sizes x 3 layouts x 4 morph modes x 2 vertex orders; plus the reduce
    names = {l.split(">")[0] for l in rows if l.startswith("deform_kernel")}
    assert len(names) == 48, "\n".join(out)
    assert any(l.startswith("bounds_reduce_kernel") for l in rows)
    for l in rows:
        m = re.search(r"spill\s+(\S+)\s+scratch\s+(\S+)", l)
        assert m and m.group(1) == "0" and m.group(2) == "0", l


# ---- GPU helpers ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def _gpu(hip_lib):
    assert device_count() >= 1, "no HIP device visible: the GPU tests must run on the MI355X box"


@pytest.fixture
def set_env(monkeypatch, hip_lib):
    """The teardown removes EVERY variable the test set and only then re-reads the environment (monkeypatch restores it after
    this fixture has finished: a reload before that would keep the overrides for the next test)."""
    was_set = set()

    def _set(**env):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
            was_set.add(k)
        hip_lib.mmdx_debug_reload_env()
    yield _set
    for k in was_set:
        monkeypatch.delenv(k, raising=False)
    hip_lib.mmdx_debug_reload_env()


def positions(a, layout, ni, nv, rows):
    """f32 [ni, nv, 3] positions out of the bytes of out_a ([ni][rows] vertices + tail)."""
    ba = BPV[layout][0]
    body = a[:ni * rows * ba]
    if layout == api.OUT_SOA:
        return body.view(np.float32).reshape(ni, rows, 3)[:, :nv]
    if layout == api.OUT_VERTEX32:
        return body.view(np.float32).reshape(ni, rows, 8)[:, :nv, :3]
    return body.view(np.float16).reshape(ni, rows, 3)[:, :nv].astype(np.float32)


def check_bounds(bnd, pos, what):
    """bnd [ni, 6] against nanmin / nanmax of pos [ni, nv, 3]: numerically equal (+-0 equal, NaN where a component is NaN
    everywhere), and every finite or infinite bound is bitwise one of the written values of its component."""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        want = np.concatenate([np.nanmin(pos, axis=1), np.nanmax(pos, axis=1)], axis=1)
    assert bnd.shape == want.shape
    bad = ~((bnd == want) | (np.isnan(bnd) & np.isnan(want)))
    assert not bad.any(), f"{what}: bounds differ at {np.argwhere(bad)[:4].tolist()}: got {bnd[bad][:4]} want {want[bad][:4]}"
    bits = pos.view(np.uint32)
    for i in range(bnd.shape[0]):
        for c in range(6):
            if not np.isnan(bnd[i, c]):
                assert (bits[i, :, c % 3] == bnd[i:i + 1, c].view(np.uint32)[0]).any(), f"{what}: instance {i} bound {c} not a written value"


def run_device(dm, layout, ni, w, pal, flags, scale, pitch, bounds):
    """One call with every operand in HBM; returns (out_a bytes, out_b bytes or None, bounds [ni, 6] or None).  Outputs start as
    0xFF sentinels, so untouched gaps and tails can be checked."""
    ba, bb = BPV[layout]
    rows = pitch or dm.nv
    na, nb = ni * rows * ba + TAIL, (ni * rows * bb + TAIL if bb else 0)
    d_a, d_b = DeviceBuffer(na), (DeviceBuffer(nb) if nb else None)
    d_pal, d_w = DeviceBuffer.from_numpy(pal), DeviceBuffer.from_numpy(w if w.size else np.zeros(1, np.float32))
    d_bnd = DeviceBuffer(ni * 24) if bounds else None
    for x in (d_a, d_b, d_bnd):
        if x is not None:
            x.memset(0xFF)
    dm.deform_batched_raw(ni, d_w.ptr, d_pal.ptr, d_a.ptr, d_b.ptr if d_b else None, layout, flags | DEV, scale, pitch,
                          d_bnd.ptr if bounds else None)
    dm.sync()
    a = d_a.download((na,), np.uint8)
    b = d_b.download((nb,), np.uint8) if d_b else None
    bnd = d_bnd.download((ni, 6), np.float32) if bounds else None
    for x in (d_a, d_b, d_pal, d_w, d_bnd):
        if x is not None:
            x.free()
    return a, b, bnd


def check_same_and_bounds(dm, layout, ni, w, pal, flags, scale, pitch, what):
    """The bounds call against the plain call on the same inputs: identical bytes (gap and tail included) and exact bounds."""
    a0, b0, _ = run_device(dm, layout, ni, w, pal, flags, scale, pitch, False)
    a1, b1, bnd = run_device(dm, layout, ni, w, pal, flags, scale, pitch, True)
    assert np.array_equal(a0, a1), f"{what}: out_a differs from mmdx_deform_batched"
    assert b0 is None or np.array_equal(b0, b1), f"{what}: out_b differs from mmdx_deform_batched"
    rows = pitch or dm.nv
    ba = BPV[layout][0]
    gap = a1[:ni * rows * ba].reshape(ni, rows * ba)[:, dm.nv * ba:]
    assert (gap == 0xFF).all() and (a1[ni * rows * ba:] == 0xFF).all(), f"{what}: gap or tail written"
    check_bounds(bnd, positions(a1, layout, ni, dm.nv, rows), what)
    return a1, bnd


# ---- GPU: the exactness matrix ----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("tile_order", [False, True], ids=["file-order", "tile-order"])
@pytest.mark.parametrize("nv", [1, 5, 511, 513, 4099])
def test_bounds_exact_every_form(_gpu, nv, tile_order):
    """SoA, 32-byte vertex (pos_scale 0.1), f16 model; shared and per-instance weights; dense and pitched; NI 1, 3, 64 (shared:
    gathered in the kernel at 3, the separate morph pass at 64)."""
    nb = 1 if nv == 1 else 17
    m = synth.make_model(nv, nb, 5, min(nv, 60), seed=7100 + nv)
    with DeformModel(m, tile_order=tile_order) as dm, DeformModel(m, tile_order=tile_order, f16_positions=True) as d16:
        for ni in (1, 3, 64):
            rates = synth.morph_weights(m.nm, np.arange(ni) * 7 + 2)
            pals = synth.make_palettes(m, np.arange(ni) * 3 + 1)
            for layout, model in ((api.OUT_SOA, dm), (api.OUT_VERTEX32, dm), (api.OUT_SOA_POS16, d16)):
                scale = 0.1 if layout == api.OUT_VERTEX32 else 1.0
                for shared in (True, False):
                    w = rates[0] if shared else rates
                    fl = api.WEIGHTS_SHARED if shared else 0
                    for pitch in (0, model.output_pitch(layout) + 3):
                        what = f"nv={nv} ni={ni} layout={layout} shared={shared} pitch={pitch}{' tile' if tile_order else ''}"
                        check_same_and_bounds(model, layout, ni, w, pals, fl, scale, pitch, what)


@pytest.mark.gpu
@pytest.mark.parametrize("nv", [513, 4099])
def test_bounds_exact_on_fast_math_model(_gpu, nv):
    """A MMDX_CREATE_FAST_MATH model: the bounds are exact with respect to that model's own outputs."""
    m = synth.make_model(nv, 17, 5, 60, seed=7300 + nv)
    with DeformModel(m, fast_math=True) as fm:
        for ni, shared in ((9, False), (11, True), (64, True), (1, True)):
            rates = synth.morph_weights(m.nm, np.arange(ni) * 3 + 4)
            pals = synth.make_palettes(m, np.arange(ni) * 5)
            for layout in (api.OUT_SOA, api.OUT_VERTEX32):
                check_same_and_bounds(fm, layout, ni, rates[0] if shared else rates, pals, api.WEIGHTS_SHARED if shared else 0,
                                      0.1 if layout == api.OUT_VERTEX32 else 1.0, 0, f"fast ni={ni} layout={layout}")


# ---- GPU: output paths ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("nv", [63, 4099])
def test_bounds_on_every_output_path(_gpu, nv):
    """Device arrays (device bounds), page-locked host arrays written by the kernel (page-locked host bounds), pageable host
    arrays through the bounce buffer and through the staging buffer (> 4 MB), pitched and dense (pageable host bounds)."""
    m = synth.make_model(nv, 17, 5, min(nv, 60), seed=7500 + nv)
    with DeformModel(m) as dm:
        for path, ni in (("device", 9), ("mapped", 9), ("pageable", 5), ("pageable", 4 * 1024 * 1024 // (24 * nv) + 2)):
            rates = synth.morph_weights(m.nm, np.arange(ni) * 5 + 1)
            pals = synth.make_palettes(m, np.arange(ni) * 2 + 3)
            for pitch in (0, nv + 13):
                rows = pitch or nv
                want_a, want_b, _ = run_device(dm, api.OUT_SOA, ni, rates, pals, 0, 1.0, pitch, False)
                what = f"{path} ni={ni} nv={nv} pitch={pitch}"
                n = ni * rows * 12 + TAIL
                if path == "device":
                    a, b, bnd = run_device(dm, api.OUT_SOA, ni, rates, pals, 0, 1.0, pitch, True)
                elif path == "mapped":
                    pa, pb, pbnd = PinnedArray((n,), np.uint8), PinnedArray((n,), np.uint8), PinnedArray((ni, 6), np.float32)
                    pa.array[:] = 0xFF
                    pb.array[:] = 0xFF
                    dm.deform_batched_raw(ni, rates.ctypes.data, pals.ctypes.data, pa.ptr, pb.ptr, api.OUT_SOA, 0, 1.0, pitch, pbnd.ptr)
                    a, b, bnd = pa.array.copy(), pb.array.copy(), pbnd.array.copy()
                    for x in (pa, pb, pbnd):
                        x.free()
                else:
                    a, b = np.full(n, 0xFF, np.uint8), np.full(n, 0xFF, np.uint8)
                    bnd = np.full((ni, 6), np.nan, np.float32)
                    dm.deform_batched_raw(ni, rates.ctypes.data, pals.ctypes.data, a.ctypes.data, b.ctypes.data, api.OUT_SOA, 0, 1.0,
                                          pitch, bnd.ctypes.data)
                assert np.array_equal(a, want_a) and np.array_equal(b, want_b), what
                check_bounds(bnd, positions(a, api.OUT_SOA, ni, nv, rows), what)


@pytest.mark.gpu
def test_deform_batched_with_bounds_returns_them(_gpu):
    m = synth.make_model(1000, 17, 5, 60, seed=77)
    ni = 7
    rates = synth.morph_weights(m.nm, np.arange(ni))
    pals = synth.make_palettes(m, np.arange(ni) * 2)
    with DeformModel(m) as dm:
        pos, nrm = dm.deform_batched(rates, pals)
        bpos, bnrm, bnd = dm.deform_batched(rates, pals, bounds=True)
        assert np.array_equal(bpos.view(np.uint32), pos.view(np.uint32)) and np.array_equal(bnrm.view(np.uint32), nrm.view(np.uint32))
        check_bounds(bnd, pos, "deform_batched(bounds=True)")
        v32, vb = dm.deform_batched(rates, pals, layout=api.OUT_VERTEX32, pos_scale=0.1, pitch=1001, bounds=True)
        check_bounds(vb, np.ascontiguousarray(v32[:, :, :3]), "vertex32 pitched")


# ---- GPU: non-finite positions ----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("tile_order", [False, True], ids=["file-order", "tile-order"])
def test_bounds_skip_nan_and_keep_inf(_gpu, tile_order):
    """Instance 1: a NaN row in one bone's palette (its vertices NaN); instance 2: +inf / -inf translations on two bones;
    instance 3: x translation NaN on every bone (x NaN everywhere -> NaN bounds for x only)."""
    nv = 4099
    m = synth.make_model(nv, 17, 5, 60, seed=7700)
    ni = 5
    rates = synth.morph_weights(m.nm, np.arange(ni) * 4)
    pals = synth.make_palettes(m, np.arange(ni) * 6).copy()
    pals[1, 3, 0:4] = np.nan
    pals[2, 5, 12] = np.inf
    pals[2, 6, 13] = -np.inf
    pals[3, :, 12] = np.nan
    with DeformModel(m, tile_order=tile_order) as dm:
        for layout in (api.OUT_SOA, api.OUT_VERTEX32):
            for shared in (True, False):
                a, bnd = check_same_and_bounds(dm, layout, ni, rates[0] if shared else rates, pals, api.WEIGHTS_SHARED if shared else 0,
                                               1.0, 0, f"non-finite layout={layout} shared={shared}")
                pos = positions(a, layout, ni, nv, nv)
                assert np.isnan(pos[1]).any() and not np.isnan(bnd[1]).any()
                assert np.isinf(pos[2]).any() and np.isinf(bnd[2]).any()
                assert np.isnan(pos[3, :, 0]).all() and np.isnan(bnd[3, [0, 3]]).all() and not np.isnan(bnd[3, [1, 2, 4, 5]]).any()
                assert not np.isnan(bnd[[0, 4]]).any()


# ---- GPU: graph replay ------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_bounds_call_recorded_in_a_graph_follows_the_palettes(_gpu):
    m = synth.make_model(4099, 40, 6, 200, seed=41)
    ni, pitch = 12, 4099 + 13
    rates = synth.morph_weights(m.nm, 9)[0]
    pals = [synth.make_palettes(m, np.arange(ni) * 3 + k) for k in (0, 50, 90)]
    flags = DEV | api.WEIGHTS_SHARED
    with DeformModel(m) as dm:
        d_pal, d_w = DeviceBuffer.from_numpy(pals[0]), DeviceBuffer.from_numpy(rates)
        n = ni * pitch * 12 + TAIL
        d_a, d_b, d_bnd = DeviceBuffer(n), DeviceBuffer(n), DeviceBuffer(ni * 24)
        dm.deform_batched_raw(ni, d_w.ptr, d_pal.ptr, d_a.ptr, d_b.ptr, api.OUT_SOA, flags, 1.0, pitch, d_bnd.ptr)   # sizes the scratch
        dm.sync()
        dm.graph_begin()
        dm.deform_batched_raw(ni, d_w.ptr, d_pal.ptr, d_a.ptr, d_b.ptr, api.OUT_SOA, flags, 1.0, pitch, d_bnd.ptr)
        g = dm.graph_end()
        prev = None
        for k, p in enumerate(pals):
            d_pal.upload(p)
            for x in (d_a, d_b, d_bnd):
                x.memset(0xFF)
            g.launch()
            dm.sync()
            ra, rbnd = d_a.download((n,), np.uint8), d_bnd.download((ni, 6), np.float32)
            da, _, dbnd = run_device(dm, api.OUT_SOA, ni, rates, p, api.WEIGHTS_SHARED, 1.0, pitch, True)
            assert np.array_equal(ra, da) and np.array_equal(rbnd.view(np.uint32), dbnd.view(np.uint32)), f"replay {k}"
            check_bounds(rbnd, positions(ra, api.OUT_SOA, ni, m.nv, pitch), f"replay {k}")
            assert prev is None or not np.array_equal(prev, rbnd), "the bounds did not follow the palettes"
            prev = rbnd
        g.close()
        for x in (d_pal, d_w, d_a, d_b, d_bnd):
            x.free()


# ---- GPU: the routes that fall back to the crowd kernel's bounds flavour --------------------------------------------------------------
@pytest.mark.gpu
def test_bounds_under_frame_kernel_and_fused_pack(_gpu, set_env):
    m = synth.make_model(4099, 17, 5, 60, seed=7900)
    with DeformModel(m) as dm, DeformModel(m, f16_positions=True) as d16:
        set_env(MMDX_FRAME_KERNEL="2")
        rates = synth.morph_weights(m.nm, np.arange(1) * 3)
        pals = synth.make_palettes(m, np.arange(1) + 2)
        for layout, model in ((api.OUT_SOA, dm), (api.OUT_VERTEX32, dm), (api.OUT_SOA_POS16, d16)):
            check_same_and_bounds(model, layout, 1, rates[0], pals, 0, 0.1 if layout == api.OUT_VERTEX32 else 1.0, 0,
                                  f"MMDX_FRAME_KERNEL=2 layout={layout}")
        set_env(MMDX_FRAME_KERNEL="1", MMDX_FUSED_PACK="1")
        ni = 11
        rates = synth.morph_weights(m.nm, np.arange(ni) * 7)
        pals = synth.make_palettes(m, np.arange(ni) * 3)
        for layout, model in ((api.OUT_SOA, dm), (api.OUT_SOA_POS16, d16)):
            for pitch in (0, model.output_pitch(layout)):
                check_same_and_bounds(model, layout, ni, rates, pals, 0, 1.0, pitch, f"MMDX_FUSED_PACK=1 layout={layout} pitch={pitch}")


# ---- GPU: full size, the benchmark's call form ---------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_full_size_crowd_bounds_bench_call_form(_gpu):
    """Config 3: 1 024 instances x 50 000 vertices, shared rates on the device, arrays from alloc_outputs with the probe's store
    flags.  The bounds call writes what the plain call wrote, and the bounds of all instances match numpy over the positions."""
    from simple_mmd_renderer_amd.crowd import crowd_frames
    m = synth.make_config("config3_crowd")
    ni, nv = 1024, m.nv
    pals = synth.make_palettes(m, crowd_frames(0, ni))
    rates = synth.morph_weights(m.nm, 30)[0]
    d_pal, d_w = DeviceBuffer.from_numpy(pals), DeviceBuffer.from_numpy(rates)
    with DeformModel(m) as dm:
        d_a, d_b, info = dm.alloc_outputs(api.OUT_SOA, ni, 4)
        d_bnd = DeviceBuffer(ni * 24)
        flags = DEV | api.WEIGHTS_SHARED | info["store_flags"]
        chunk = 128
        dm.deform_batched_raw(ni, d_w.ptr, d_pal.ptr, d_a.ptr, d_b.ptr, api.OUT_SOA, flags)
        dm.sync()
        plain = [d_a.download((chunk * nv * 12,), np.uint8, offset=c * nv * 12) for c in range(0, ni, chunk)]
        d_a.memset(0xFF)
        dm.deform_batched_raw(ni, d_w.ptr, d_pal.ptr, d_a.ptr, d_b.ptr, api.OUT_SOA, flags, 1.0, 0, d_bnd.ptr)
        dm.sync()
        bnd = d_bnd.download((ni, 6), np.float32)
        for k, c in enumerate(range(0, ni, chunk)):
            a = d_a.download((chunk * nv * 12,), np.uint8, offset=c * nv * 12)
            assert np.array_equal(a, plain[k]), f"instances {c}..{c + chunk - 1} differ from mmdx_deform_batched"
            check_bounds(bnd[c:c + chunk], a.view(np.float32).reshape(chunk, nv, 3), f"config 3 instances {c}..")
        for x in (d_a, d_b, d_bnd):
            x.free()
    d_pal.free(); d_w.free()


# ---- GPU: argument errors ---------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_bounds_argument_errors(_gpu):
    m = synth.make_model(513, 17, 5, 60, seed=8100)
    ni = 3
    rates = synth.morph_weights(m.nm, np.arange(ni))
    pals = synth.make_palettes(m, np.arange(ni))
    with DeformModel(m) as dm:
        a = api.DeformArgs()
        a.struct_size = C.sizeof(api.DeformArgs)
        pos, nrm, bnd = np.empty((ni, m.nv, 3), np.float32), np.empty((ni, m.nv, 3), np.float32), np.empty((ni, 6), np.float32)
        a.flags, a.n_instances, a.out_layout = 0, ni, api.OUT_SOA
        a.morph_weights, a.palettes, a.out_a, a.out_b, a.pos_scale = rates.ctypes.data, pals.ctypes.data, pos.ctypes.data, nrm.ctypes.data, 1.0
        lib = api.lib()
        assert lib.mmdx_deform_batched_bounds(dm.h, C.byref(a), None) == 1
        assert b"out_bounds" in lib.mmdx_last_error_string()
        a.flags = 1 << 20
        assert lib.mmdx_deform_batched_bounds(dm.h, C.byref(a), bnd.ctypes.data) == 1
        assert b"unknown bits" in lib.mmdx_last_error_string()
        a.flags = 0
        assert lib.mmdx_deform_batched_bounds(dm.h, C.byref(a), bnd.ctypes.data) == 0
        check_bounds(bnd, pos, "after the refusals")

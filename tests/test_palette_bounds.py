"""A conservative box per instance from the palette alone: mmdx_palette_bounds and the bone-box table behind it (include/mmdx.h).

libmmd has no bone boxes, so the contract has the shape of mmdx_cull_bounds':
  * a stated binary32 arithmetic -- tests/palette_bounds_ref.py restates the table and the boxes in numpy from the header's text;
    the library's table, csrc/pbounds_math.hpp on the CPU (tests/pbounds_math_driver.cpp, also under ASan + UBSan) and the kernel
    are held to it bit for bit (a NaN only has to be a NaN);
  * a containment guarantee -- the restatement's box contains what the oracle deforms (the check of the derivation of eps,
    DESIGN.md 6.8), and the kernel's box contains the box mmdx_deform_batched_bounds writes.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from simple_mmd_renderer_amd import _capi as api
from simple_mmd_renderer_amd import synth
from simple_mmd_renderer_amd.engine import DeformModel, DeviceBuffer, device_count
from tests import golden_util as gu
from tests import host_program as hp
from tests import palette_bounds_ref as pb
from tests.test_capi_symbols import declared_symbols

F = np.float32
INVALID, NO_DEVICE, UNSUPPORTED = 1, 3, 6
DEV = api.PALETTE_ON_DEVICE | api.OUT_ON_DEVICE
CONTAIN_MODELS = [(3000, 40, 8, 64), (2000, 7, 3, 200), (4000, 130, 12, 50)]
FRAMES = [0, 13, 47, 200]


@pytest.fixture(autouse=True)
def _lib(hip_lib):
    return hip_lib


def assert_table_equal(got, want, what):
    for k in ("n_boxes", "n_nonconvex", "max_vertex_entries"):
        assert got[k] == want[k], (what, k, got[k], want[k])
    for k in ("eps", "weight_sum_dev"):
        assert gu.bits(F(got[k])) == gu.bits(F(want[k])), (what, k, got[k], want[k])
    assert np.array_equal(got["bones"], want["bones"]), what
    gu.assert_bits_equal(got["boxes"], want["boxes"], what + ": boxes")


def host_table(m, **kw):
    with DeformModel(m, host_only=True, **kw) as dm:
        return dm.bone_boxes(), dm.get_skin()


# ---------------------------------------------------------------------------------------- CPU ----
def test_entry_points_are_declared_exported_and_bound(hip_lib):
    for name in ("mmdx_palette_bounds", "mmdx_model_get_bone_boxes"):
        assert name in declared_symbols() and hasattr(hip_lib, name) and name in api.SIGNATURES, name
    args, info, model_info, abi = hp.c_values(["sizeof(mmdx_palette_bounds_args)", "sizeof(mmdx_bone_box_info)", "sizeof(mmdx_model_info)",
                                               "MMDX_ABI_VERSION"])
    assert C.sizeof(api.PaletteBoundsArgs) == args == 4 * 4 + 2 * 8 + 2 * 4
    assert C.sizeof(api.BoneBoxInfo) == info == 32
    assert model_info == 80 and abi == 3 and hip_lib.mmdx_abi_version() == 3
    assert all(callable(getattr(DeformModel, f)) for f in ("bone_boxes", "palette_bounds_raw", "palette_bounds"))
    assert "mmdx_palette_bounds(" in open(os.path.join(pb.ROOT, "simple_mmd_renderer_amd", "host", "mmdx_poser.hpp")).read()


def _table_variants():
    base = synth.make_model(600, 12, 4, 32, seed=4601)
    yield "plain", base, {}
    # a bone no vertex uses; a BDEF4 weight of exactly 0 and a retagged BDEF2 whose unused id are the only mentions of that bone
    m = base.copy()
    m.bone_ids[m.bone_ids == 5] = 4
    v4 = int(np.nonzero(m.skin_type == synth.BDEF4)[0][0])
    m.bone_ids[v4, 3], m.bone_weights[v4, 3] = 5, 0.0
    v2 = np.nonzero(m.skin_type == synth.BDEF2)[0][:2]
    m.bone_ids[v2[0], 0], m.bone_weights[v2[0], 0] = 5, 0.0            # w == 0: BDEF1 on id1
    m.bone_ids[v2[1], 1], m.bone_weights[v2[1], 0] = 5, 1.0            # w == 1: BDEF1 on id0
    m.meta["absent"], m.meta["retagged"] = 5, v2
    yield "unused bone, zero BDEF4 weight, retagged BDEF2", m, {}
    # a group morph over vertex morphs 0 and 1: their entries count once more each
    g = base.copy()
    e = int(g.morph_off[-1])
    g.morph_type = np.concatenate([g.morph_type, [synth.MORPH_GROUP]]).astype(np.int32)
    g.morph_off = np.concatenate([g.morph_off, [e + 2]]).astype(np.uint32)
    g.morph_index = np.concatenate([g.morph_index, [0, 1]]).astype(np.uint32)
    g.morph_value = np.concatenate([g.morph_value, np.array([[0.5, 0, 0], [0.25, 0, 0]], F)]).astype(F)
    yield "group morph", g, {}
    yield "f16 positions", base, {"f16_positions": True}


@pytest.mark.parametrize("what,m,kw", list(_table_variants()), ids=lambda v: v if isinstance(v, str) else "")
def test_table_equals_the_restatement(what, m, kw):
    got, skin = host_table(m, **kw)
    want = pb.bone_box_table(m, skin, f16=bool(kw.get("f16_positions")))
    assert_table_equal(got, want, what)
    assert got["n_nonconvex"] == 0 and got["n_boxes"] >= 11 and np.isfinite(got["boxes"]).all()
    assert (got["boxes"][:, :3] <= got["boxes"][:, 3:6]).all() and (np.diff(got["bones"].astype(np.int64)) > 0).all()
    plain = host_table(synth.make_model(600, 12, 4, 32, seed=4601))[0]
    if "absent" in m.meta:
        assert m.meta["absent"] not in got["bones"] and got["n_boxes"] == 11
        assert (skin[0][m.meta["retagged"]] == synth.BDEF1).all()
    elif what == "group morph":
        assert got["max_vertex_entries"] > plain["max_vertex_entries"] and (got["boxes"][:, 6:] >= plain["boxes"][:, 6:]).all()
        assert (got["boxes"][:, 6:] > plain["boxes"][:, 6:]).any() and got["eps"] > plain["eps"]
    elif what == "f16 positions":
        assert not np.array_equal(got["boxes"], plain["boxes"])
        assert np.array_equal(got["boxes"][:, :6], got["boxes"][:, :6].astype(np.float16).astype(F))
    # the size query alone
    with DeformModel(m, host_only=True, **kw) as dm:
        info = api.BoneBoxInfo()
        assert api.lib().mmdx_model_get_bone_boxes(dm.h, C.byref(info), None, None) == INVALID          # struct_size 0
        info.struct_size = C.sizeof(api.BoneBoxInfo)
        assert api.lib().mmdx_model_get_bone_boxes(dm.h, C.byref(info), None, None) == api.OK and info.n_boxes == got["n_boxes"]
        assert api.lib().mmdx_model_get_bone_boxes(dm.h, None, None, None) == INVALID


def _arithmetic_cases():
    """(what, boxes [n, 9], mats [NI, n, 16], eps, morph_scale, pos_scale)"""
    rng = np.random.RandomState(4602)
    n, ni = 9, 6
    lo = rng.uniform(-10, 10, (n, 3))
    boxes = np.concatenate([lo, lo + rng.uniform(0, 5, (n, 3)), rng.uniform(0, 1.5, (n, 3))], axis=1).astype(F)
    m = synth.make_model(64, n, 0, 0, seed=4603)
    rigid = synth.make_palettes(m, np.arange(ni) * 11 + 3)
    eps = F(34 * pb.U) + F(3e-8)
    yield "rigid", boxes, rigid, eps, 1.0, 0.1
    yield "rigid, no morphs, pos_scale 1", boxes, rigid, eps, 0.0, 1.0
    scaled = rigid.copy().reshape(ni, n, 4, 4)
    scaled[:, :, :3, :3] *= rng.uniform(0.2, 3.0, (ni, n, 3, 1)).astype(F)
    yield "scaled", boxes, scaled.reshape(ni, n, 16), eps, 0.5, 0.1
    sheared = scaled.copy()
    sheared[:, :, 0, 1] += F(0.75)
    sheared[:, :, 2, 0] -= F(1.25)
    yield "sheared", boxes, sheared.reshape(ni, n, 16), eps, 1.0, 2.5
    special = rigid.copy()
    special[0, :, 0:3] = F(-0.0)                       # a -0 row of the matrix
    special[1, 2, 12:15] = F(-0.0)
    special[2] *= F(1e-40)                             # denormal matrix elements
    tiny = boxes.copy()
    tiny[0, :6] = [-0.0, 0.0, -0.0, 0.0, -0.0, 0.0]
    tiny[1, :6] = np.array([-3, -2, -1, 1, 2, 3], F) * F(1e-41)
    yield "-0 and denormals", tiny, special, eps, 0.0, 1.0
    inf = rigid.copy()
    inf[1, 3, 13] = np.inf                             # an infinite translation: inf - inf in that instance
    inf[4, 0, 12] = -np.inf
    yield "infinite translation", boxes, inf, eps, 1.0, 0.1
    nan = rigid.copy()
    nan[3, 5, 6] = np.nan
    yield "a NaN element", boxes, nan, eps, 1.0, 0.1
    yield "empty table", np.zeros((0, 9), F), np.zeros((3, 0, 16), F), eps, 1.0, 0.1


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan-ubsan"])
def test_arithmetic_header_equals_the_restatement_on_the_cpu(sanitize):
    """csrc/pbounds_math.hpp, the code the kernel compiles, as a stand-alone host program (-ffp-contract=off; the second build with
    -fsanitize=address,undefined, run directly)."""
    exe = pb.build_math_driver(sanitize)
    seen = {}
    for what, boxes, mats, eps, ms, ps in _arithmetic_cases():
        blo, bhi, _ = pb.row_boxes(boxes, mats, eps, ms)
        want = pb.fold(blo, bhi, ps)
        pb.assert_rows_equal(pb.run_driver(exe, boxes, mats, eps, ms, ps), want, what)
        seen[what] = want
    assert all(np.isfinite(seen[k]).all() for k in ("rigid", "scaled", "sheared", "-0 and denormals"))
    nan_rows = lambda a: np.isnan(a).all(axis=1)       # noqa: E731
    assert np.isnan(seen["a NaN element"]).any(axis=1).tolist() == nan_rows(seen["a NaN element"]).tolist() == [False] * 3 + [True] + [False] * 2
    assert nan_rows(seen["infinite translation"]).tolist() == [False, True, False, False, True, False]
    assert nan_rows(seen["empty table"]).all() and seen["empty table"].shape == (3, 6)
    assert (seen["rigid"][:, :3] < seen["rigid"][:, 3:]).all()


@pytest.fixture(scope="module")
def contain_cases(oracle):
    """(shape, morph_scale, frame index, restatement's row, oracle min, oracle max): deformed once, shared."""
    out = []
    for shape in CONTAIN_MODELS:
        m = synth.make_model(*shape, seed=4604)
        table, skin = host_table(m)
        assert_table_equal(table, pb.bone_box_table(m, skin), "containment model")
        pals = synth.make_palettes(m, FRAMES)
        for ms, rates in ((1.0, synth.morph_weights(m.nm, FRAMES)), (0.0, np.zeros((len(FRAMES), m.nm), F))):
            rows = pb.palette_bounds(table, pals, 0.1, ms)
            for i in range(len(FRAMES)):
                pos = oracle.deform(m, rates[i], pals[i])[0] * F(0.1)
                out.append((shape, ms, i, rows[i], pos.min(axis=0), pos.max(axis=0)))
    return out


def test_restatement_box_contains_the_oracle_on_the_cpu(contain_cases):
    """The check of the derivation of eps: all 24 cases, every axis, nothing left out."""
    assert len(contain_cases) == 24
    ratios = []
    for shape, ms, i, row, lo, hi in contain_cases:
        assert np.isfinite(row).all()
        assert (row[:3] <= lo).all() and (row[3:] >= hi).all(), (shape, ms, FRAMES[i], row, lo, hi)
        ratios.append((row[3:] - row[:3]) / (hi - lo))
    print("palette box extent / true extent: %.3f .. %.3f" % (np.min(ratios), np.max(ratios)))


def test_box_is_tight_where_it_can_be(oracle):
    """One vertex per bone, BDEF1 only, no morphs: every bone box is a point, so the row may differ from the true box by the padding
    and the rounding it covers only: |row - true| <= 2 * pad per component."""
    nb = 40
    m = synth.make_model(nb, nb, 0, 0, seed=4605, mix=(1.0, 0.0, 0.0, 0.0))
    m.bone_ids[:, 0] = np.arange(nb)
    table, skin = host_table(m)
    assert_table_equal(table, pb.bone_box_table(m, skin), "tightness model")
    assert table["n_boxes"] == nb and table["max_vertex_entries"] == 0 and np.array_equal(table["boxes"][:, :3], table["boxes"][:, 3:6])
    pals = synth.make_palettes(m, FRAMES)
    for ps in (1.0, 0.1):
        rows, pad = pb.palette_bounds(table, pals, ps, 0.0), pb.max_pad(table, pals, ps, 0.0)
        for i in range(len(FRAMES)):
            pos = oracle.deform(m, np.zeros(0, F), pals[i])[0] * F(ps)
            true = np.concatenate([pos.min(axis=0), pos.max(axis=0)])
            assert (rows[i, :3] <= true[:3]).all() and (rows[i, 3:] >= true[3:]).all()
            assert (np.abs(rows[i].astype(np.float64) - true) <= 2.0 * np.tile(pad[i], 2).astype(np.float64)).all(), (ps, i, rows[i], true, pad[i])
            assert (pad[i] < 1e-3 * (true[3:] - true[:3])).all()


def test_palette_bounds_refuses_bad_arguments():
    """Everything is decided before the first HIP call, so a host-only handle shows it without a GPU: every mistake is
    MMDX_ERR_INVALID_ARGUMENT first, then a model with a negative weight is MMDX_ERR_UNSUPPORTED, and only a valid call gets as far
    as MMDX_ERR_NO_DEVICE."""
    lib = api.lib()
    err = lambda: lib.mmdx_last_error_string().decode()          # noqa: E731
    ni, nb = 3, 5
    m = synth.make_model(64, nb, 2, 8, seed=4606)
    pal = np.zeros((ni + 1, nb, 16), F)
    out = np.zeros((ni, 6), F)

    def args(n=ni, flags=0, struct_size=None, reserved0=0, palettes=pal.ctypes.data, out_bounds=out.ctypes.data, pos_scale=0.1,
             morph_scale=1.0):
        a = api.PaletteBoundsArgs()
        a.struct_size = C.sizeof(api.PaletteBoundsArgs) if struct_size is None else struct_size
        a.flags, a.n_instances, a.reserved0 = flags, n, reserved0
        a.palettes, a.out_bounds, a.pos_scale, a.morph_scale = palettes, out_bounds, pos_scale, morph_scale
        return a
    with DeformModel(m, host_only=True) as dm:
        call = lambda a, h=dm.h: lib.mmdx_palette_bounds(h, C.byref(a) if a is not None else None)          # noqa: E731
        assert call(args(), None) == INVALID and "NULL" in err()
        assert call(None) == INVALID and "NULL" in err()
        for k in ("palettes", "out_bounds"):
            assert call(args(**{k: None})) == INVALID and "NULL" in err(), k
        for size in (0, C.sizeof(api.PaletteBoundsArgs) - 8, C.sizeof(api.PaletteBoundsArgs) + 8):
            assert call(args(struct_size=size)) == INVALID and "struct_size" in err(), size
        for bad in (1 << 1, 1 << 3, 1 << 7, 1 << 8, 1 << 9, 1 << 31):
            assert call(args(flags=bad)) == INVALID and "unknown flag" in err(), bad
        assert call(args(reserved0=1)) == INVALID and "reserved0" in err()
        for bad in (0.0, -1.0, np.inf, np.nan):
            assert call(args(pos_scale=bad)) == INVALID and "pos_scale" in err(), bad
        for bad in (-1e-9, -1.0, np.inf, np.nan):
            assert call(args(morph_scale=bad)) == INVALID and "morph_scale" in err(), bad
        base = pal.ctypes.data
        for at in (base, base + 64, base + ni * nb * 64 - 4, base - ni * 24 + 4):
            assert call(args(out_bounds=at)) == INVALID and "overlaps" in err(), at - base
        assert call(args(out_bounds=base + ni * nb * 64)) == NO_DEVICE                        # directly behind: valid
        assert call(args(flags=api.PALETTE_ON_DEVICE, palettes=base + 8)) == INVALID and "16-byte" in err()
        assert call(args(flags=api.OUT_ON_DEVICE, out_bounds=out.ctypes.data + 2)) == INVALID and "4-byte" in err()
        assert call(args(n=0)) == api.OK and call(args(n=0, palettes=None, out_bounds=None)) == api.OK
        for flags, ms in ((0, 1.0), (DEV, 0.0), (api.OUT_ON_DEVICE, 2.0)):
            assert call(args(flags=flags, morph_scale=ms)) == NO_DEVICE, flags
        with pytest.raises(api.MmdxError) as e:
            dm.palette_bounds(pal[:ni], 0.1, 1.0)
        assert e.value.status == NO_DEVICE
    # one negative BDEF4 weight: counted, and refused after validation but before the device question
    neg = m.copy()
    v4 = int(np.nonzero(neg.skin_type == synth.BDEF4)[0][0])
    neg.bone_weights[v4, 2] = -0.125
    with DeformModel(neg, host_only=True) as dm:
        assert dm.bone_boxes()["n_nonconvex"] == 1 == pb.bone_box_table(neg, dm.get_skin())["n_nonconvex"]
        call = lambda a, h=dm.h: lib.mmdx_palette_bounds(h, C.byref(a))          # noqa: E731
        assert call(args()) == UNSUPPORTED and "1 vertices" in err() and "negative" in err()
        assert call(args(reserved0=1)) == INVALID and call(args(pos_scale=0.0)) == INVALID
        assert call(args(n=0)) == api.OK
    # BDEF2 weights outside [0, 1] count too
    neg2 = m.copy()
    v2 = np.nonzero(neg2.skin_type == synth.BDEF2)[0][:2]
    neg2.bone_weights[v2, 0] = [-0.25, 1.5]
    with DeformModel(neg2, host_only=True) as dm:
        assert dm.bone_boxes()["n_nonconvex"] == 2 == pb.bone_box_table(neg2, dm.get_skin())["n_nonconvex"]


def test_palette_bounds_kernels_have_no_spills_and_no_scratch(hip_lib):
    out = subprocess.run([sys.executable, os.path.join(pb.ROOT, "tools", "kernel_resources.py"), api.LIB_PATH, "palette_bounds"],
                         capture_output=True, text=True, check=True).stdout.splitlines()
    assert {l.split()[0] for l in out} == {"palette_bounds_kernel<1>", "palette_bounds_kernel<4>"}
    for l in out:
        f = l.split()
        res = dict(zip(f[1::2], (int(v) for v in f[2::2])))
        assert res["spill"] == 0 and res["scratch"] == 0 and res["vgpr"] <= 64, l
        assert res["lds"] == (0 if "<1>" in l else 128), l


# ---------------------------------------------------------------------------------------- GPU ----
def _rows_both_forms(dm, pals, ps, ms):
    """The call with device operands (the output between sentinel rows) and with host operands -> (device rows, host rows)."""
    ni = pals.shape[0]
    d_pal = DeviceBuffer.from_numpy(pals)
    d_out = DeviceBuffer((ni + 2) * 24)
    d_out.memset(0xEE)
    dm.palette_bounds_raw(ni, d_pal.ptr, d_out.ptr + 24, DEV, ps, ms)
    dm.sync()
    raw = d_out.download((ni + 2, 6), F)
    assert (raw[[0, -1]].view(np.uint32) == 0xEEEEEEEE).all(), "the call wrote outside its rows"
    gu.assert_bits_equal(d_pal.download(pals.shape, F), pals, "the call changed its input")
    d_pal.free()
    d_out.free()
    return raw[1:-1], dm.palette_bounds(pals, ps, ms)


@pytest.mark.gpu
@pytest.mark.parametrize("nb", [1, 63, 64, 65, 257, 600])
def test_gpu_kernel_equals_the_restatement(nb):
    """Table lengths at the wave edge (63, 64, 65: one wave per instance up to 64 rows, a workgroup per instance above), at the
    workgroup edge (257: the register fold runs a second, partial trip) and 600 (three trips); 1, 3 and 70 instances (a partial
    workgroup of the four-instances form, 18 workgroups of it); both scales; device and host operands; a fast-math model."""
    assert device_count() >= 1, "no HIP device visible: the GPU tests must run on the MI355X box"
    m = synth.make_model(8 * nb, nb, 2, 16, seed=900 + nb)
    all_pals = synth.make_palettes(m, np.arange(70) * 0.83 + 1)          # the synthetic poses repeat every 60 frames: 70 distinct ones
    with DeformModel(m) as dm, DeformModel(m, fast_math=True) as fm:
        table = dm.bone_boxes()
        assert table["n_boxes"] == nb
        assert_table_equal(table, pb.bone_box_table(m, dm.get_skin()), "device model")
        for ni in (1, 3, 70):
            pals = np.ascontiguousarray(all_pals[:ni])
            for ps in (1.0, 0.1):
                for ms in (0.0, 1.0):
                    want = pb.palette_bounds(table, pals, ps, ms)
                    assert np.isfinite(want).all() and len({r.tobytes() for r in want}) == ni
                    what = "nb %d ni %d pos_scale %g morph_scale %g" % (nb, ni, ps, ms)
                    dev, host = _rows_both_forms(dm, pals, ps, ms)
                    gu.assert_bits_equal(dev, want, what + ": device operands")
                    gu.assert_bits_equal(host, want, what + ": host operands")
            gu.assert_bits_equal(fm.palette_bounds(pals, 0.1, 1.0), pb.palette_bounds(table, pals, 0.1, 1.0), "fast-math model, ni %d" % ni)
        # a NaN in one instance's palette: that row is NaN, the others are untouched by it
        bad = all_pals[:7].copy()
        bad[4, int(table["bones"][nb // 2]), 9] = np.nan
        want = pb.palette_bounds(table, bad, 0.1, 1.0)
        assert np.isnan(want).all(axis=1).tolist() == [i == 4 for i in range(7)]
        dev, host = _rows_both_forms(dm, bad, 0.1, 1.0)
        pb.assert_rows_equal(dev, want, "NaN palette: device operands")
        pb.assert_rows_equal(host, want, "NaN palette: host operands")
        assert np.isnan(dev[4]).all() and np.isfinite(np.delete(dev, 4, axis=0)).all()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["plain", "fast_math", "tile_order"])
def test_gpu_box_contains_the_deform_bounds(kind):
    """For every instance the row contains the row mmdx_deform_batched_bounds writes from the same palette and pos_scale: both
    float32 layouts, shared and per-instance rates."""
    assert device_count() >= 1, "no HIP device visible: the GPU tests must run on the MI355X box"
    ni = 16
    m = synth.make_model(3000, 40, 8, 64, seed=4607)
    pals = synth.make_palettes(m, np.arange(ni) * 9 + 2)
    rates = synth.morph_weights(m.nm, np.arange(ni) * 4)
    with DeformModel(m, **({} if kind == "plain" else {kind: True})) as dm:
        table = dm.bone_boxes()
        row = dm.palette_bounds(pals, 0.1, 1.0)
        gu.assert_bits_equal(row, pb.palette_bounds(table, pals, 0.1, 1.0), kind)
        for layout in (api.OUT_SOA, api.OUT_VERTEX32):
            for shared in (True, False):
                bnd = dm.deform_batched(rates[3] if shared else rates, pals, layout, shared_weights=shared, pos_scale=0.1, bounds=True)[-1]
                assert np.isfinite(bnd).all()
                what = (kind, layout, shared)
                assert (row[:, :3] <= bnd[:, :3]).all() and (row[:, 3:] >= bnd[:, 3:]).all(), what
                ratio = (row[:, 3:] - row[:, :3]) / (bnd[:, 3:] - bnd[:, :3])
                print(what, "extent ratio %.3f .. %.3f" % (ratio.min(), ratio.max()))

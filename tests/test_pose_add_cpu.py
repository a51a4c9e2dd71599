"""Additive layers without a GPU: mmdx_pose_add / mmdx_rate_add (include/mmdx.h).

  * tests/golden/pose_add_expect.npz comes from the real libmmd (tests/pose_add_driver.cpp over libmmd's own operators;
    tests/gen_pose_add_golden.py); tests/pose_add_ref.py -- the numpy restatement written from the header -- reproduces it bit for
    bit, and so does a fresh run of libmmd where its headers are present;
  * the bone-morph property: the oracle's morphed solve of poses P equals its plain solve of the restatement's P + (T, Q) rows;
  * everything the two calls refuse before the first HIP call, on a MMDX_CREATE_HOST_ONLY model, each with its status, and
    MMDX_ERR_NO_DEVICE for a valid call.
"""
import ctypes as C
import os

import numpy as np
import pytest

from simple_mmd_renderer_amd import _capi as api
from simple_mmd_renderer_amd import synth, vmd
from simple_mmd_renderer_amd.engine import DeformModel
from tests import golden_util as gu
from tests import motion_time_ref as mt
from tests import pose_add_ref as pa
from tests import row_blend_ref as rb
from tests.test_capi_symbols import declared_symbols

ROOT = os.path.dirname(mt.HERE)
INVALID, BAD_INDEX, NO_DEVICE, UNSUPPORTED = 1, 2, 3, 6
A, B, PARAMS, OUT = api.BLEND_A_ON_DEVICE, api.BLEND_B_ON_DEVICE, api.BLEND_PARAMS_ON_DEVICE, api.OUT_ON_DEVICE
needs_driver = pytest.mark.skipif(not mt.driver_available(), reason="the reference's libmmd headers are not present")


@pytest.fixture(autouse=True)
def _lib(hip_lib):
    return hip_lib


def test_entry_points_are_declared_exported_and_bound(hip_lib):
    syms = declared_symbols()
    for name in ("mmdx_pose_add", "mmdx_rate_add"):
        assert name in syms and hasattr(hip_lib, name) and name in api.SIGNATURES, name
    hdr = open(os.path.join(ROOT, "include", "mmdx.h")).read()
    assert "typedef struct mmdx_row_add_args {" in hdr and "#define MMDX_ABI_VERSION 3u" in hdr
    assert "#define MMDX_REF_NONE 0xFFFFFFFFu" in hdr and api.REF_NONE == vmd.REF_NONE == pa.REF_NONE == 0xFFFFFFFF
    assert hip_lib.mmdx_abi_version() == 3
    # the blend's structure (four u32, five pointers, two u32, one pointer) and then two pointers and two u32
    assert C.sizeof(api.RowAddArgs) == C.sizeof(api.RowBlendArgs) + 2 * 8 + 2 * 4 == 96
    for f in api.RowBlendArgs._fields_:
        assert getattr(api.RowAddArgs, f[0]).offset == getattr(api.RowBlendArgs, f[0]).offset, f[0]
    assert [f[0] for f in api.RowAddArgs._fields_[-4:]] == ["ref_ids", "refs", "n_refs", "reserved1"]
    for name in ("add_poses", "add_rates", "add_poses_device", "add_rates_device"):
        assert callable(getattr(vmd, name))
    poser = open(os.path.join(ROOT, "simple_mmd_renderer_amd", "host", "mmdx_poser.hpp")).read()
    assert "mmdx_pose_add(" in poser and "mmdx_rate_add(" in poser and "void AddPoses(" in poser and "void AddRates(" in poser


# ---- the fixture ------------------------------------------------------------------------------------------------------------------
def test_numpy_restatement_reproduces_the_libmmd_fixture():
    z = pa.fixture()
    n = z["weights"].size
    assert n == len(pa.WEIGHTS) * (rb.N_MASKS + 1) * 2 * pa.TIMES_PER_CASE + 2 * len(pa.WEIGHTS)
    assert os.path.getsize(pa.FIXTURE) <= os.path.getsize(rb.FIXTURE)
    gu.assert_bits_equal(z["bone_masks"], rb.fixture()["bone_masks"], "the mask rows are row_blend_ref's")
    gu.assert_bits_equal(z["morph_masks"], rb.fixture()["morph_masks"], "the mask rows are row_blend_ref's")
    got_p, got_r = pa.add_poses(*pa.operands(z, "poses")), pa.add_rates(*pa.operands(z, "rates"))
    gu.assert_bits_equal(got_p, z["expect_poses"], "poses")
    gu.assert_bits_equal(got_r, z["expect_rates"], "rates")
    # items that stay A are A's items, every bit; mixed items have a fourth translation float of +0
    for what, got in (("poses", got_p), ("rates", got_r)):
        a, b, w, masks, ids, refs, rids = pa.operands(z, what)
        _, mix = pa.mixing(w, a.shape[1], masks, ids, refs, rids)
        gu.assert_bits_equal(z["expect_" + what][~mix], a[~mix], "A items of " + what)
        assert mix.any() and (~mix).any()
        if what == "poses":
            assert (got[mix][:, 3].view(np.uint32) == 0).all()
    # reference row 0 is clip b at time 0: the B row of a fixture row whose time b is 0
    at0 = np.flatnonzero(~z["synthetic"] & (z["times_b"] == 0))
    assert at0.size
    gu.assert_bits_equal(z["b_poses"][at0[0]], z["pose_refs"][0], "reference poses")
    gu.assert_bits_equal(z["b_rates"][at0[0]], z["rate_refs"][0], "reference rates")


def test_fixture_covers_what_it_claims():
    pa.check_coverage(pa.fixture())


def test_restatement_reference_id_cases():
    """MMDX_REF_NONE: B is the difference; a valid id: B against that row; any other id: the row is A (the device rule)."""
    a = np.array([[[1, 2, 3, 5, 0, 0, 0, 1]]] * 3, np.float32)
    b = np.array([[[1, 1, 1, 0, 0, 0, 0, 1]]] * 3, np.float32)
    refs = np.array([[[0.5, 0.5, 0.5, 0, 0, 0, 0, 1]]], np.float32)
    got = pa.add_poses(a, b, [1, 1, 1], refs=refs, ref_ids=[pa.REF_NONE, 0, 7])
    assert got[0, 0].tolist() == [2, 3, 4, 0, 0, 0, 0, 1] and got[1, 0].tolist() == [1.5, 2.5, 3.5, 0, 0, 0, 0, 1]
    gu.assert_bits_equal(got[2], a[2], "row A, the fourth float included")
    assert pa.add_poses(a, b, [2, 0.5, 0])[..., 0].reshape(-1).tolist() == [3, 1.5, 1]             # exaggerated, partial, A
    r = pa.add_rates([[0.5], [0.5], [0.5]], [[1.0], [1.0], [1.0]], [1.5, 1.5, 1.5], refs=[[0.25]], ref_ids=[pa.REF_NONE, 0, 1])
    assert r.reshape(-1).tolist() == [2.0, 1.625, 0.5]
    # a quarter turn about x added at half weight to the identity: an eighth turn, as SLerp gives it
    q = pa.add_poses(np.array([[[0, 0, 0, 0, 0, 0, 0, 1]]], np.float32),
                     np.array([[[0, 0, 0, 0, np.sin(np.pi / 4), 0, 0, np.cos(np.pi / 4)]]], np.float32), [0.5])[0, 0, 4:]
    assert np.allclose(q, [np.sin(np.pi / 8), 0, 0, np.cos(np.pi / 8)], atol=1e-6)


@needs_driver
def test_fixture_equals_a_fresh_run_of_libmmd():
    from tests import gen_pose_add_golden as gen
    z, fresh = pa.fixture(), gen.build()
    assert set(z) == set(fresh)
    for k in sorted(z):
        assert fresh[k].dtype == z[k].dtype and fresh[k].shape == z[k].shape, k
        if z[k].dtype == np.float32:
            gu.assert_bits_equal(fresh[k], z[k], k)
        else:
            np.testing.assert_array_equal(fresh[k], z[k], k)          # (the times of the synthetic rows are NaN)


# ---- the bone-morph property ----------------------------------------------------------------------------------------------------------
def test_added_morph_rows_solve_to_the_morphed_palettes_on_the_cpu(oracle):
    """Every bone the target of at most one application (T, Q): the oracle's morphed solve of P at the morphs' rates equals, value
    for value, its plain solve of the restatement's P + (T, Q) rows at those rates.  == on floats, not bit patterns: the plain
    solve multiplies by the identity once more, which can turn -0 into +0 and changes nothing else."""
    g = pa.morph_rig()
    added = pa.add_poses(g["poses"], g["b"], g["weights"], g["masks"], g["mask_ids"])
    e, mix = pa.mixing(g["weights"], g["poses"].shape[1], g["masks"], g["mask_ids"])
    assert mix.any(1).all() and (~mix).any(1).all() and not np.isnan(added).any() and np.isnan(g["b"][:, 0]).all()
    touched = 0
    for i in range(g["poses"].shape[0]):
        morphed = oracle.bone_solve_full(g["rest"], g["parent"], g["poses"][i], g["level"], g["flags"], morphs=g["morphs"], rates=g["rates"][i])
        plain = oracle.bone_solve_full(g["rest"], g["parent"], added[i], g["level"], g["flags"])
        assert np.isfinite(morphed).all() and np.array_equal(morphed, plain), i
        touched += int(not np.array_equal(morphed, oracle.bone_solve_full(g["rest"], g["parent"], g["poses"][i], g["level"], g["flags"])))
    assert touched == g["poses"].shape[0]                              # the morphs moved every instance


# ---- refusals ahead of the first HIP call -------------------------------------------------------------------------------------------
NI, ITEMS, NM, NR = 3, 5, 2, 2
ALL = A | B | PARAMS | OUT


def said(status, want_status, want_text, what):
    msg = api.lib().mmdx_last_error_string().decode()
    assert status == want_status and want_text in msg, (what, status, msg, want_text)


class Host:
    """Valid host operands of both calls, by name."""

    def __init__(self, item_floats):
        tail = (item_floats,) if item_floats > 1 else ()
        shape = (NI, ITEMS) + tail
        self.a = dict(a=np.zeros(shape, np.float32), b=np.ones(shape, np.float32), out=np.zeros(shape, np.float32),
                      weights=np.array([0.0, 0.5, 1.5], np.float32), mask_ids=np.array([0, 1, rb.MASK_NONE], np.uint32),
                      masks=np.array([[0, 0.5, 1, 2, -1]] * NM, np.float32), ref_ids=np.array([1, pa.REF_NONE, 0], np.uint32),
                      refs=np.ones((NR, ITEMS) + tail, np.float32), ids=np.array([2, 0], np.uint32), count=np.array([2], np.uint32))

    def args(self, flags=0, n=NI, items=ITEMS, size=None, reserved0=0, reserved1=0, n_masks=NM, n_refs=NR, **replace):
        p = {k: v.ctypes.data for k, v in self.a.items()}
        p.update(replace)
        return api.RowAddArgs(C.sizeof(api.RowAddArgs) if size is None else size, flags, n, items, p["a"], p["b"], p["weights"],
                              p["mask_ids"], p["masks"], n_masks, reserved0, p["out"], p["ref_ids"], p["refs"], n_refs, reserved1)


def _select(ids, n_ids, count=None, on_device=False, size=None, flags=None, reserved0=0):
    s = vmd.instance_select(ids, n_ids, count, on_device=on_device)
    if size is not None:
        s.struct_size = size
    if flags is not None:
        s.flags = flags
    s.reserved0 = reserved0
    return s


@pytest.mark.parametrize("which", ["pose", "rate"])
def test_add_calls_refuse_before_the_device_on_a_host_only_model(which):
    lib = api.lib()
    fn = lib.mmdx_pose_add if which == "pose" else lib.mmdx_rate_add
    name = "mmdx_pose_add" if which == "pose" else "mmdx_rate_add"
    item_floats = 8 if which == "pose" else 1
    h = Host(item_floats)
    row_bytes = NI * ITEMS * item_floats * 4
    with DeformModel(synth.make_model(64, 3, 1, 8, seed=5), host_only=True) as dm:
        def call(args, sel=None, m=dm.h):
            return fn(m, C.byref(args) if args is not None else None, C.byref(sel) if sel is not None else None)
        said(call(h.args(), m=None), INVALID, "model / args is NULL", "NULL model")
        said(call(None), INVALID, "model / args is NULL", "NULL args")
        for size in (0, C.sizeof(api.RowBlendArgs), C.sizeof(api.RowAddArgs) - 8, C.sizeof(api.RowAddArgs) + 8):
            said(call(h.args(size=size)), INVALID, "mmdx_row_add_args.struct_size mismatch", size)
        for bad in (1 << 0, 1 << 1, 1 << 4, 1 << 8, 1 << 10, 1 << 14, 1 << 31):
            said(call(h.args(flags=bad)), INVALID, "unknown flag bits in mmdx_row_add_args.flags", bad)
        said(call(h.args(reserved0=1)), INVALID, "mmdx_row_add_args.reserved0 must be 0", "reserved0")
        said(call(h.args(reserved1=1)), INVALID, "mmdx_row_add_args.reserved1 must be 0", "reserved1")
        # the list's header, ahead of the empty call
        ids, count = h.a["ids"].ctypes.data, h.a["count"].ctypes.data
        said(call(h.args(n=0), _select(ids, 2, size=8)), INVALID, "mmdx_instance_select.struct_size mismatch", "list size")
        said(call(h.args(), _select(ids, 2, flags=2)), INVALID, "unknown bits in mmdx_instance_select.flags", "list bits")
        said(call(h.args(), _select(ids, 2, reserved0=3)), INVALID, "mmdx_instance_select.reserved0 must be 0", "list reserved0")
        said(call(h.args(), _select(None, 2)), INVALID, "mmdx_instance_select.ids is NULL", "list ids")
        # nothing to do: MMDX_OK, on a host-only model too, whatever the pointers
        assert call(h.args(n=0, a=None, b=None, out=None, weights=None, refs=None)) == 0
        assert call(h.args(items=0, a=None, b=None, out=None, weights=None, refs=None)) == 0
        for k in ("a", "b", "weights", "out"):
            said(call(h.args(**{k: None})), INVALID, "a / b / weights / out is NULL", k)
        said(call(h.args(masks=None)), INVALID, "n_masks > 0 but masks is NULL", "masks")
        said(call(h.args(refs=None)), INVALID, "n_refs > 0 but refs is NULL", "refs")
        assert call(h.args(refs=None, ref_ids=None)) == NO_DEVICE                       # without ref ids refs is not looked at
        # overlaps: only out == a and out == b are in place
        a, b, out = (h.a[k].ctypes.data for k in ("a", "b", "out"))
        said(call(h.args(out=a + 32)), INVALID, "a / b and out overlap without being the same array", "a, out")
        said(call(h.args(out=b + row_bytes - 4)), INVALID, "a / b and out overlap without being the same array", "b, out")
        said(call(h.args(b=a)), INVALID, "a and b overlap", "a == b")
        said(call(h.args(b=a + row_bytes - 4)), INVALID, "a and b overlap", "a, b")
        for k in ("weights", "mask_ids", "masks"):
            said(call(h.args(**{k: out + 4})), INVALID, "weights / mask_ids / masks overlaps out", k)
        for k in ("ref_ids", "refs"):
            said(call(h.args(**{k: out + 4})), INVALID, "ref_ids / refs overlaps out", k)
            said(call(h.args(**{k: out + row_bytes - 4})), INVALID, "ref_ids / refs overlaps out", k)
        said(call(h.args(refs=out)), INVALID, "ref_ids / refs overlaps out", "refs == out")
        assert call(h.args(refs=a)) == NO_DEVICE and call(h.args(refs=b)) == NO_DEVICE  # the reference may be A's or B's array
        assert call(h.args(mask_ids=None, masks=out, n_masks=0)) == NO_DEVICE          # masks that are not read may be anything
        assert call(h.args(ref_ids=None, refs=out)) == NO_DEVICE                       # and so may refs
        assert call(h.args(refs=out, n_refs=0, ref_ids=np.full(NI, pa.REF_NONE, np.uint32).ctypes.data)) == NO_DEVICE
        # alignment of device operands (never dereferenced here: the model has no device)
        far = [0x7000_0000_0000 + k * 0x10_0000_0000 for k in range(9)]
        dev = dict(a=far[0], b=far[1], out=far[2], weights=far[3], mask_ids=far[4], masks=far[5], ref_ids=far[7], refs=far[8])
        step = 4 if which == "pose" else 2
        want = "must be 16-byte aligned" if which == "pose" else "must be 4-byte aligned"
        for k, flag in (("a", A), ("b", B), ("out", OUT)):
            said(call(h.args(flags=flag, **{k: dev[k] + step})), INVALID, "device a / b / out of " + name + " " + want, k)
            said(call(h.args(flags=ALL, **dict(dev, **{k: dev[k] + step}))), INVALID, "device a / b / out of " + name + " " + want, k)
        for k in ("weights", "mask_ids", "masks"):
            said(call(h.args(flags=ALL, **dict(dev, **{k: dev[k] + 2}))), INVALID, "device weights / mask_ids / masks must be 4-byte aligned", k)
        said(call(h.args(flags=ALL, **dict(dev, ref_ids=dev["ref_ids"] + 2))), INVALID, "device ref_ids must be 4-byte aligned", "ref_ids")
        said(call(h.args(flags=ALL, **dict(dev, refs=dev["refs"] + step))), INVALID, "device refs of " + name + " " + want, "refs")
        assert call(h.args(flags=A | B | OUT, a=dev["a"], b=dev["b"], out=dev["out"], refs=h.a["refs"].ctypes.data + 0)) == NO_DEVICE
        assert call(h.args(flags=ALL, **dict(dev, out=dev["a"]))) == NO_DEVICE            # in place, both ways
        assert call(h.args(flags=ALL, **dict(dev, out=dev["b"]))) == NO_DEVICE
        # sizes one launch cannot hold
        said(call(h.args(flags=ALL, n=(1 << 23) + 1, items=1, **dev)), UNSUPPORTED, "more than 2^23 instances", "instances")
        said(call(h.args(flags=ALL, n=1, items=65535 * 256 + 1, **dev)), UNSUPPORTED, "2^24 items in a row", "items")
        said(call(h.args(flags=ALL, **dev), _select(far[6], (1 << 23) + 1, on_device=True)), UNSUPPORTED, "list positions", "list")
        # the list
        said(call(h.args(flags=ALL, **dev), _select(far[6] + 2, 2, on_device=True)), INVALID,
             "device ids / count of mmdx_instance_select must be 4-byte aligned", "list alignment")
        for flags in (0, A | B, A | OUT, B | OUT | PARAMS):
            said(call(h.args(flags=flags), _select(ids, 2, count)), INVALID,
                 name + " with a select list takes a, b and out in device memory only", flags)
        rows = dict(a=dev["a"], b=dev["b"], out=dev["out"])
        past, one = np.array([0, NI], np.uint32), np.array([1], np.uint32)
        said(call(h.args(flags=A | B | OUT, **rows), _select(past.ctypes.data, 2)), INVALID,
             "mmdx_instance_select.ids[1] = 3 is not below n_instances", "host id")
        assert call(h.args(flags=A | B | OUT, **rows), _select(past.ctypes.data, 2, one.ctypes.data)) == NO_DEVICE   # behind *count
        # host operands are read before the first HIP call
        nan_w = np.array([0.5, np.nan, 0.0], np.float32)
        said(call(h.args(weights=nan_w.ctypes.data)), INVALID, "weights[1] is NaN", "NaN weight")
        said(call(h.args(flags=A | B | OUT, weights=nan_w.ctypes.data, **rows)), INVALID, "weights[1] is NaN", "NaN weight, device rows")
        big_w = np.array([7.0, 1e30, np.inf], np.float32)
        assert call(h.args(weights=big_w.ctypes.data)) == NO_DEVICE                    # weights above 1 are legal
        bad_ids = np.array([0, NM, rb.MASK_NONE], np.uint32)
        said(call(h.args(mask_ids=bad_ids.ctypes.data)), BAD_INDEX, "mask_ids[1] = 2 is neither below n_masks nor MMDX_MASK_NONE", "mask id")
        nan_m = np.array([[0, 1, 0, 1, 0], [0, 0, np.nan, 0, 0]], np.float32)
        said(call(h.args(masks=nan_m.ctypes.data)), INVALID, "masks holds a NaN (value 7)", "NaN mask value")
        bad_refs = np.array([0, pa.REF_NONE, NR], np.uint32)
        said(call(h.args(ref_ids=bad_refs.ctypes.data)), BAD_INDEX, "ref_ids[2] = 2 is neither below n_refs nor MMDX_REF_NONE", "ref id")
        said(call(h.args(flags=A | B | OUT, ref_ids=bad_refs.ctypes.data, **rows)), BAD_INDEX, "ref_ids[2] = 2", "ref id, device rows")
        said(call(h.args(n_refs=0, refs=None)), BAD_INDEX, "ref_ids[0] = 1", "no reference rows at all")
        nan_r = np.full_like(h.a["refs"], np.nan)
        assert call(h.args(refs=nan_r.ctypes.data)) == NO_DEVICE                       # host refs are not inspected
        # a valid call, every placement of the operands: the model has nothing to run on
        host_only = "model was created with MMDX_CREATE_HOST_ONLY"
        said(call(h.args()), NO_DEVICE, host_only, "host operands")
        said(call(h.args(out=a)), NO_DEVICE, host_only, "host operands, out == a")
        said(call(h.args(out=b)), NO_DEVICE, host_only, "host operands, out == b")
        said(call(h.args(flags=ALL, **dev)), NO_DEVICE, host_only, "device operands")
        said(call(h.args(flags=A | B | OUT, **rows), _select(ids, 2, count)), NO_DEVICE, host_only, "host list")
        said(call(h.args(flags=ALL, **dev), _select(far[6], 2, far[6] + 64, on_device=True)), NO_DEVICE, host_only, "device list")
    # the Python face
    with pytest.raises(ValueError):
        vmd.add_poses(np.zeros((2, 3, 8)), np.zeros((2, 4, 8)), [0, 0])
    with pytest.raises(ValueError):
        vmd.add_rates(np.zeros((2, 3)), np.zeros((2, 3)), [0, 0, 0])
    with pytest.raises(ValueError):
        vmd.add_rates(np.zeros((2, 3)), np.zeros((2, 3)), [0, 0], refs=np.zeros((1, 4)), ref_ids=[0, 0])
    with pytest.raises(api.MmdxError) as e:
        vmd.add_rates(np.zeros((2, 3)), np.zeros((2, 3)), [0, 0])               # no model
    assert e.value.status == INVALID

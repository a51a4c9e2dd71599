"""Layers without a GPU: mmdx_pose_blend / mmdx_rate_blend / mmdx_skeleton_subtree_mask (include/mmdx.h).

  * tests/golden/row_blend_expect.npz comes from the real libmmd (tests/motion_blend_driver.cpp as it is, one call per bone or morph
    with that item's effective weights; tests/gen_row_blend_golden.py); tests/row_blend_ref.py -- motion_blend_ref's restatement
    applied per (row, item) -- reproduces it bit for bit, and so does a fresh run of libmmd where its headers are present;
  * mmdx_skeleton_subtree_mask on hand-written hierarchies, through the library and through csrc/bone_mask.hpp as a stand-alone
    program built with -fsanitize=address,undefined;
  * everything the two blend calls refuse before the first HIP call, on a MMDX_CREATE_HOST_ONLY model, each with its status, and
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
from tests import host_program as hp
from tests import motion_blend_ref as mb
from tests import motion_time_ref as mt
from tests import row_blend_ref as rb
from tests.test_capi_symbols import declared_symbols

ROOT = hp.ROOT
INVALID, BAD_INDEX, NO_DEVICE, UNSUPPORTED = 1, 2, 3, 6
A, B, PARAMS, OUT = api.BLEND_A_ON_DEVICE, api.BLEND_B_ON_DEVICE, api.BLEND_PARAMS_ON_DEVICE, api.OUT_ON_DEVICE
needs_driver = pytest.mark.skipif(not mt.driver_available(), reason="the reference's libmmd headers are not present")


@pytest.fixture(autouse=True)
def _lib(hip_lib):
    return hip_lib


def test_entry_points_are_declared_exported_and_bound(hip_lib):
    syms = declared_symbols()
    for name in ("mmdx_pose_blend", "mmdx_rate_blend", "mmdx_skeleton_subtree_mask"):
        assert name in syms and hasattr(hip_lib, name) and name in api.SIGNATURES, name
    hdr = open(os.path.join(ROOT, "include", "mmdx.h")).read()
    assert "typedef struct mmdx_row_blend_args {" in hdr and "#define MMDX_ABI_VERSION 3u" in hdr
    assert "#define MMDX_MASK_NONE 0xFFFFFFFFu" in hdr and api.MASK_NONE == vmd.MASK_NONE == rb.MASK_NONE == 0xFFFFFFFF
    assert hip_lib.mmdx_abi_version() == 3
    assert C.sizeof(api.RowBlendArgs) == 4 * 4 + 5 * 8 + 2 * 4 + 8           # four u32, five pointers, two u32, one pointer
    # three flag bits of their own: no other *_ON_DEVICE flag or mode bit of the header has them
    assert (A, B, PARAMS) == (1 << 11, 1 << 12, 1 << 13)
    for name in ("blend_poses", "blend_rates", "blend_poses_device", "blend_rates_device"):
        assert callable(getattr(vmd, name))
    assert callable(vmd.Skeleton.subtree_mask)
    poser = open(os.path.join(ROOT, "simple_mmd_renderer_amd", "host", "mmdx_poser.hpp")).read()
    assert "mmdx_pose_blend(" in poser and "mmdx_rate_blend(" in poser and "mmdx_skeleton_subtree_mask(" in poser


# ---- the fixture ------------------------------------------------------------------------------------------------------------------
def test_numpy_restatement_reproduces_the_libmmd_fixture():
    z = rb.fixture()
    n = z["weights"].size
    assert n == len(mb.WEIGHTS) * len(mb.PAIRS) * (rb.N_MASKS + 1) and os.path.getsize(rb.FIXTURE) < 512 * 1024
    assert z["bone_masks"].shape == (rb.N_MASKS, len(z["bone_names"])) and z["morph_masks"].shape == (rb.N_MASKS, len(z["morph_names"]))
    assert set(np.unique(z["bone_masks"])) == set(np.unique(z["morph_masks"])) == set(rb.MASK_VALUES)
    gu.assert_bits_equal(rb.blend_poses(z["a_poses"], z["b_poses"], z["weights"], z["bone_masks"], z["mask_ids"]), z["expect_poses"],
                         "poses")
    gu.assert_bits_equal(rb.blend_rates(z["a_rates"], z["b_rates"], z["weights"], z["morph_masks"], z["mask_ids"]), z["expect_rates"],
                         "rates")
    # end-point items are the unblended items, every bit
    side = mb.side_of(rb.effective_weights(z["weights"], len(z["bone_names"]), z["bone_masks"], z["mask_ids"]))
    gu.assert_bits_equal(z["expect_poses"][side == 0], z["a_poses"][side == 0], "A items")
    gu.assert_bits_equal(z["expect_poses"][side == 1], z["b_poses"][side == 1], "B items")
    # without a mask the per-item restatement is the row-level one of the cross-fade
    none = z["mask_ids"] == rb.MASK_NONE
    gu.assert_bits_equal(mb.blend_poses(z["a_poses"][none], z["b_poses"][none], z["weights"][none]), z["expect_poses"][none], "no mask")
    gu.assert_bits_equal(mb.blend_rates(z["a_rates"][none], z["b_rates"][none], z["weights"][none]), z["expect_rates"][none], "no mask")


def test_fixture_covers_what_it_claims():
    rb.check_coverage(rb.fixture())


def test_restatement_mask_id_cases():
    """MMDX_MASK_NONE: the weight itself; a valid id: its row; any other id: 0, the row is A."""
    m = np.array([[0.5, 2.0, -1.0]], np.float32)
    e = rb.effective_weights([0.5, 0.5, 0.5, np.nan], 3, m, [rb.MASK_NONE, 0, 1, 0])
    assert e[0].tolist() == [0.5, 0.5, 0.5] and e[1].tolist() == [0.25, 1.0, -0.5] and e[2].tolist() == [0.0, 0.0, 0.0]
    assert np.isnan(e[3]).all()
    assert rb.effective_weights([0.25], 2).tolist() == [[0.25, 0.25]]


@needs_driver
def test_fixture_equals_a_fresh_run_of_libmmd():
    z = rb.fixture()
    nb, nm = len(z["bone_names"]), len(z["morph_names"])
    ops = (z["bone_names"], z["morph_names"], z["clips_a"], z["times_a"], z["clips_b"], z["times_b"])
    poses, rates = rb.driver_expect(*ops, rb.effective_weights(z["weights"], nb, z["bone_masks"], z["mask_ids"]),
                                    rb.effective_weights(z["weights"], nm, z["morph_masks"], z["mask_ids"]))
    gu.assert_bits_equal(poses, z["expect_poses"], "poses")
    gu.assert_bits_equal(rates, z["expect_rates"], "rates")
    n = z["weights"].size
    a_poses, a_rates = rb.driver_expect(*ops, np.zeros((n, nb), np.float32), np.zeros((n, nm), np.float32))
    b_poses, b_rates = rb.driver_expect(*ops, np.ones((n, nb), np.float32), np.ones((n, nm), np.float32))
    for got, key in ((a_poses, "a_poses"), (b_poses, "b_poses"), (a_rates, "a_rates"), (b_rates, "b_rates")):
        gu.assert_bits_equal(got, z[key], key)


# ---- mmdx_skeleton_subtree_mask -----------------------------------------------------------------------------------------------------
TREE = [-1, 0, 0, 1, 1, 2, 2]          # 0 -> (1 -> 3, 4), (2 -> 5, 6)
MASK_CASES = [   # name, parent, roots, inside, outside, expected mask as inside (1) / outside (0), or the position of the bad root
    ("a chain", [-1, 0, 1, 2, 3], [2], 1.0, 0.0, [0, 0, 1, 1, 1]),
    ("a fork", TREE, [1], 1.0, 0.0, [0, 1, 0, 1, 1, 0, 0]),
    ("two roots, one inside the other's subtree", TREE, [1, 3], 1.0, 0.0, [0, 1, 0, 1, 1, 0, 0]),
    ("the inner root first, a root listed twice", TREE, [3, 1, 3], 1.0, 0.0, [0, 1, 0, 1, 1, 0, 0]),
    ("a root that is a leaf", TREE, [5], 1.0, 0.0, [0, 0, 0, 0, 0, 1, 0]),
    ("the root of everything", TREE, [0], 0.75, -0.5, [1] * 7),
    ("n_roots == 0", TREE, [], 1.0, 0.25, [0] * 7),
    ("several parentless bones, parents outside [0, NB)", [-1, 0, -7, 2, 9, 4], [2, 4], 1.0, 0.0, [0, 0, 1, 1, 1, 1]),
    ("children ahead of their parents", [1, 2, -1, 0], [1], 0.5, 0.0, [1, 1, 0, 1]),
    ("a cycle is left after NB steps", [1, 0, 1], [2], 1.0, 0.0, [0, 0, 1]),
    ("a bad root", [-1, 0, 1, 2, 3], [1, 9], 1.0, 0.0, 1),
    ("a bad root that equals NB", [-1, 0], [2], 1.0, 0.0, 0),
]


def _mask_bits(expected, inside, outside):
    return np.where(np.array(expected, bool), np.float32(inside), np.float32(outside)).astype(np.float32).view(np.uint32)


@pytest.mark.parametrize("case", MASK_CASES, ids=[c[0] for c in MASK_CASES])
def test_subtree_mask_through_the_library(case):
    _, parent, roots, inside, outside, expected = case
    sk = vmd.Skeleton(np.zeros((len(parent), 3), np.float32), parent)
    if isinstance(expected, int):
        with pytest.raises(api.MmdxError) as e:
            sk.subtree_mask(roots, inside, outside)
        assert e.value.status == BAD_INDEX and "roots[%d] = %d" % (expected, roots[expected]) in str(e.value)
        out = np.full(len(parent), np.float32(7))
        r = np.array(roots, np.uint32)
        assert api.lib().mmdx_skeleton_subtree_mask(sk.h, r.size, r.ctypes.data, 1.0, 0.0, out.ctypes.data) == BAD_INDEX
        assert (out == 7).all()                                      # nothing written
    else:
        got = sk.subtree_mask(roots, inside, outside)
        assert got.dtype == np.float32 and got.view(np.uint32).tolist() == _mask_bits(expected, inside, outside).tolist()
    sk.close()


def test_subtree_mask_refuses_nulls_and_needs_no_device():
    lib = api.lib()
    sk = vmd.Skeleton(np.zeros((3, 3), np.float32), [-1, 0, 1], physics_seam=True)      # the ordered solver's plan keeps parents too
    out, roots = np.zeros(3, np.float32), np.array([1], np.uint32)
    assert lib.mmdx_skeleton_subtree_mask(None, 1, roots.ctypes.data, 1.0, 0.0, out.ctypes.data) == INVALID
    assert lib.mmdx_skeleton_subtree_mask(sk.h, 1, roots.ctypes.data, 1.0, 0.0, None) == INVALID
    assert lib.mmdx_skeleton_subtree_mask(sk.h, 1, None, 1.0, 0.0, out.ctypes.data) == INVALID
    assert lib.mmdx_skeleton_subtree_mask(sk.h, 0, None, 1.0, 0.5, out.ctypes.data) == 0 and out.tolist() == [0.5] * 3
    assert sk.subtree_mask([1]).tolist() == [0.0, 1.0, 1.0]
    sk.close()


def mask_driver():
    """tests/bone_mask_driver.cpp (csrc/bone_mask.hpp with its own main) under the sanitizers of tests/host_program.py."""
    return hp.build("bone_mask_driver", [os.path.join(hp.TESTS, "bone_mask_driver.cpp")], opt="-O1", sanitize=True)


@pytest.mark.parametrize("case", MASK_CASES, ids=[c[0] for c in MASK_CASES])
def test_subtree_mask_header_under_asan_ubsan(case):
    """The same cases through the stand-alone program: the walk stays inside its arrays and computes the same masks."""
    _, parent, roots, inside, outside, expected = case
    argv = [str(len(parent))] + [str(p) for p in parent] + [str(len(roots))] + [str(r) for r in roots] + \
        [repr(float(inside)), repr(float(outside))]
    r = hp.run(mask_driver(), argv, timeout=60)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stdout, r.stderr)
    if isinstance(expected, int):
        assert r.stdout.split() == ["BAD", str(expected)]
    else:
        assert [int(x, 16) for x in r.stdout.split()] == _mask_bits(expected, inside, outside).tolist()


# ---- refusals ahead of the first HIP call -------------------------------------------------------------------------------------------
NI, ITEMS, NM = 3, 5, 2
ALL = A | B | PARAMS | OUT


def said(status, want_status, want_text, what):
    msg = api.lib().mmdx_last_error_string().decode()
    assert status == want_status and want_text in msg, (what, status, msg, want_text)


class Host:
    """Valid host operands of both calls, by name."""

    def __init__(self, item_floats):
        shape = (NI, ITEMS) + ((item_floats,) if item_floats > 1 else ())
        self.a = dict(a=np.zeros(shape, np.float32), b=np.ones(shape, np.float32), out=np.zeros(shape, np.float32),
                      weights=np.array([0.0, 0.5, 1.0], np.float32), mask_ids=np.array([0, 1, rb.MASK_NONE], np.uint32),
                      masks=np.array([[0, 0.5, 1, 2, -1]] * NM, np.float32), ids=np.array([2, 0], np.uint32),
                      count=np.array([2], np.uint32))

    def args(self, flags=0, n=NI, items=ITEMS, size=None, reserved0=0, n_masks=NM, **replace):
        p = {k: v.ctypes.data for k, v in self.a.items()}
        p.update(replace)
        return api.RowBlendArgs(C.sizeof(api.RowBlendArgs) if size is None else size, flags, n, items, p["a"], p["b"], p["weights"],
                                p["mask_ids"], p["masks"], n_masks, reserved0, p["out"])


def _select(ids, n_ids, count=None, on_device=False, size=None, flags=None, reserved0=0):
    s = vmd.instance_select(ids, n_ids, count, on_device=on_device)
    if size is not None:
        s.struct_size = size
    if flags is not None:
        s.flags = flags
    s.reserved0 = reserved0
    return s


@pytest.mark.parametrize("which", ["pose", "rate"])
def test_blend_calls_refuse_before_the_device_on_a_host_only_model(which):
    lib = api.lib()
    fn = lib.mmdx_pose_blend if which == "pose" else lib.mmdx_rate_blend
    item_floats = 8 if which == "pose" else 1
    h = Host(item_floats)
    row_bytes = NI * ITEMS * item_floats * 4
    with DeformModel(synth.make_model(64, 3, 1, 8, seed=5), host_only=True) as dm:
        def call(args, sel=None, m=dm.h):
            return fn(m, C.byref(args) if args is not None else None, C.byref(sel) if sel is not None else None)
        said(call(h.args(), m=None), INVALID, "model / args is NULL", "NULL model")
        said(call(None), INVALID, "model / args is NULL", "NULL args")
        for size in (0, C.sizeof(api.RowBlendArgs) - 8, C.sizeof(api.RowBlendArgs) + 8):
            said(call(h.args(size=size)), INVALID, "mmdx_row_blend_args.struct_size mismatch", size)
        for bad in (1 << 0, 1 << 1, 1 << 4, 1 << 8, 1 << 10, 1 << 14, 1 << 31):
            said(call(h.args(flags=bad)), INVALID, "unknown flag bits in mmdx_row_blend_args.flags", bad)
        said(call(h.args(reserved0=1)), INVALID, "mmdx_row_blend_args.reserved0 must be 0", "reserved0")
        # the list's header, ahead of the empty call
        ids, count = h.a["ids"].ctypes.data, h.a["count"].ctypes.data
        said(call(h.args(n=0), _select(ids, 2, size=8)), INVALID, "mmdx_instance_select.struct_size mismatch", "list size")
        said(call(h.args(), _select(ids, 2, flags=2)), INVALID, "unknown bits in mmdx_instance_select.flags", "list bits")
        said(call(h.args(), _select(ids, 2, reserved0=3)), INVALID, "mmdx_instance_select.reserved0 must be 0", "list reserved0")
        said(call(h.args(), _select(None, 2)), INVALID, "mmdx_instance_select.ids is NULL", "list ids")
        # nothing to do: MMDX_OK, on a host-only model too, whatever the pointers
        assert call(h.args(n=0, a=None, b=None, out=None, weights=None)) == 0
        assert call(h.args(items=0, a=None, b=None, out=None, weights=None)) == 0
        for k in ("a", "b", "weights", "out"):
            said(call(h.args(**{k: None})), INVALID, "a / b / weights / out is NULL", k)
        said(call(h.args(masks=None)), INVALID, "n_masks > 0 but masks is NULL", "masks")
        # overlaps: only out == a and out == b are in place
        a, b, out = (h.a[k].ctypes.data for k in ("a", "b", "out"))
        said(call(h.args(out=a + 32)), INVALID, "a / b and out overlap without being the same array", "a, out")
        said(call(h.args(out=b + row_bytes - 4)), INVALID, "a / b and out overlap without being the same array", "b, out")
        said(call(h.args(b=a)), INVALID, "a and b overlap", "a == b")
        said(call(h.args(b=a + row_bytes - 4)), INVALID, "a and b overlap", "a, b")
        for k in ("weights", "mask_ids", "masks"):
            said(call(h.args(**{k: out + 4})), INVALID, "weights / mask_ids / masks overlaps out", k)
        assert call(h.args(mask_ids=None, masks=out, n_masks=0)) == NO_DEVICE          # masks that are not read may be anything
        # alignment of device operands (never dereferenced here: the model has no device)
        far = [0x7000_0000_0000 + k * 0x10_0000_0000 for k in range(7)]
        dev = dict(a=far[0], b=far[1], out=far[2], weights=far[3], mask_ids=far[4], masks=far[5])
        step = 4 if which == "pose" else 2
        want = "must be 16-byte aligned" if which == "pose" else "must be 4-byte aligned"
        for k, flag in (("a", A), ("b", B), ("out", OUT)):
            said(call(h.args(flags=flag, **{k: dev[k] + step})), INVALID, want, k)
            said(call(h.args(flags=ALL, **dict(dev, **{k: dev[k] + step}))), INVALID, want, k)
        for k in ("weights", "mask_ids", "masks"):
            said(call(h.args(flags=ALL, **dict(dev, **{k: dev[k] + 2}))), INVALID, "device weights / mask_ids / masks must be 4-byte aligned", k)
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
            said(call(h.args(flags=flags), _select(ids, 2, count)), INVALID, "with a select list takes a, b and out in device memory only", flags)
        rows = dict(a=dev["a"], b=dev["b"], out=dev["out"])
        past, one = np.array([0, NI], np.uint32), np.array([1], np.uint32)
        said(call(h.args(flags=A | B | OUT, **rows), _select(past.ctypes.data, 2)), INVALID,
             "mmdx_instance_select.ids[1] = 3 is not below n_instances", "host id")
        assert call(h.args(flags=A | B | OUT, **rows), _select(past.ctypes.data, 2, one.ctypes.data)) == NO_DEVICE   # behind *count
        # host operands are read before the first HIP call
        nan_w = np.array([0.5, np.nan, 0.0], np.float32)
        said(call(h.args(weights=nan_w.ctypes.data)), INVALID, "weights[1] is NaN", "NaN weight")
        said(call(h.args(flags=A | B | OUT, weights=nan_w.ctypes.data, **rows)), INVALID, "weights[1] is NaN", "NaN weight, device rows")
        bad_ids = np.array([0, NM, rb.MASK_NONE], np.uint32)
        said(call(h.args(mask_ids=bad_ids.ctypes.data)), BAD_INDEX, "mask_ids[1] = 2 is neither below n_masks nor MMDX_MASK_NONE", "mask id")
        said(call(h.args(mask_ids=h.a["mask_ids"].ctypes.data, n_masks=0, masks=None)), BAD_INDEX, "mask_ids[0] = 0", "no masks at all")
        nan_m = np.array([[0, 1, 0, 1, 0], [0, 0, np.nan, 0, 0]], np.float32)
        said(call(h.args(masks=nan_m.ctypes.data)), INVALID, "masks holds a NaN (value 7)", "NaN mask value")
        assert call(h.args(mask_ids=None, masks=nan_m.ctypes.data)) == NO_DEVICE       # without mask ids no mask is read
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
        vmd.blend_poses(np.zeros((2, 3, 8)), np.zeros((2, 4, 8)), [0, 0])
    with pytest.raises(ValueError):
        vmd.blend_rates(np.zeros((2, 3)), np.zeros((2, 3)), [0, 0, 0])
    with pytest.raises(api.MmdxError) as e:
        vmd.blend_rates(np.zeros((2, 3)), np.zeros((2, 3)), [0, 0])               # no model
    assert e.value.status == INVALID

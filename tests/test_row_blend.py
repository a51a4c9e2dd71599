"""Layers on the GPU: mmdx_pose_blend / mmdx_rate_blend (include/mmdx.h), the masked blend of two evaluated pose or rate arrays.

Everything is compared as bit patterns.  The expectation is tests/golden/row_blend_expect.npz (the real libmmd) or
tests/row_blend_ref.py (motion_blend_ref's restatement at the effective weight of every (row, item)); only in a MIXED item that
holds a NaN is the comparison by position (the sign and payload of such a NaN are outside the contract).  Shapes: row lengths on
either side of a wave and of a 256-lane chunk, 1 / 3 / 65 instances.
"""
import ctypes as C
import os

import numpy as np
import pytest

from simple_mmd_renderer_amd import _capi as api
from simple_mmd_renderer_amd import synth, vmd
from simple_mmd_renderer_amd.engine import DeformModel, DeviceBuffer
from tests import golden_util as gu
from tests import motion_blend_ref as mb
from tests import row_blend_ref as rb

pytestmark = pytest.mark.gpu
NONE = rb.MASK_NONE
SENT = 0xC5                                   # byte pattern of an output before the call
ALL = api.BLEND_A_ON_DEVICE | api.BLEND_B_ON_DEVICE | api.BLEND_PARAMS_ON_DEVICE | api.OUT_ON_DEVICE
POISON = np.array([0x7FC0BAD1], np.uint32).view(np.float32)[0]      # a NaN no arithmetic here produces


@pytest.fixture(autouse=True)
def _lib(hip_lib):
    return hip_lib


@pytest.fixture(scope="module")
def dm():
    with DeformModel(synth.make_model(64, 3, 1, 8, seed=5)) as m:
        yield m


def _close(*xs):
    for x in xs:
        for y in (x if isinstance(x, (list, tuple)) else [x]):
            y.free() if isinstance(y, DeviceBuffer) else y.close()


def _fn(a):
    return api.lib().mmdx_pose_blend if a.ndim == 3 else api.lib().mmdx_rate_blend


def run_device(dm, a, b, w, masks=None, mask_ids=None, out="separate", select=None):
    """One call with every operand in device memory -> the WHOLE output array.  out: "separate" (prefilled with SENT), "a" or "b"
    (in place).  select: (ids, count or None, on_device) -- ids u32 array, the list's capacity is its size."""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    ni, items = a.shape[:2]
    d_a, d_b, d_w = DeviceBuffer.from_numpy(a), DeviceBuffer.from_numpy(b), DeviceBuffer.from_numpy(np.ascontiguousarray(w, np.float32))
    bufs = [d_a, d_b, d_w]
    d_out = d_a if out == "a" else d_b if out == "b" else DeviceBuffer(a.nbytes)
    if out == "separate":
        d_out.memset(SENT)
        bufs.append(d_out)
    args = api.RowBlendArgs(C.sizeof(api.RowBlendArgs), ALL, ni, items, d_a.ptr, d_b.ptr, d_w.ptr, None, None, 0, 0, d_out.ptr)
    if mask_ids is not None:
        m = np.ascontiguousarray(masks, np.float32).reshape(-1, items)
        d_ids, d_m = DeviceBuffer.from_numpy(np.ascontiguousarray(mask_ids, np.uint32)), DeviceBuffer.from_numpy(m) if m.size else None
        bufs += [d_ids] + ([d_m] if d_m else [])
        args.mask_ids, args.masks, args.n_masks = d_ids.ptr, d_m.ptr if d_m else None, m.shape[0]
    sel = None
    if select is not None:
        ids, count, on_device = select
        ids = np.ascontiguousarray(ids, np.uint32)
        cnt = None if count is None else np.array([count], np.uint32)
        if on_device:
            d_l = DeviceBuffer(max(ids.nbytes, 4))
            if ids.size:
                d_l.upload(ids)
            d_c = DeviceBuffer.from_numpy(cnt) if cnt is not None else None
            bufs += [d_l] + ([d_c] if d_c else [])
            sel = vmd.instance_select(d_l.ptr, ids.size, d_c.ptr if d_c else None)
        else:
            sel = vmd.instance_select(ids.ctypes.data, ids.size, cnt.ctypes.data if cnt is not None else None, on_device=False)
    api.check(_fn(a)(dm.h, C.byref(args), C.byref(sel) if sel is not None else None))
    dm.sync()
    got = d_out.download(a.shape, np.float32)
    _close(bufs)
    return got


def _sentinel(like):
    return np.full(like.nbytes, SENT, np.uint8).view(np.float32).reshape(like.shape)


def run_host(dm, a, b, w, masks=None, mask_ids=None, out="separate"):
    """The same with every operand in host memory."""
    a, b = np.array(a, np.float32), np.array(b, np.float32)          # copies: in place writes into them
    ni, items = a.shape[:2]
    w = np.ascontiguousarray(w, np.float32)
    o = a if out == "a" else b if out == "b" else _sentinel(a)
    args = api.RowBlendArgs(C.sizeof(api.RowBlendArgs), 0, ni, items, a.ctypes.data, b.ctypes.data, w.ctypes.data, None, None, 0, 0,
                            o.ctypes.data)
    if mask_ids is not None:
        ids, m = np.ascontiguousarray(mask_ids, np.uint32), np.ascontiguousarray(masks, np.float32).reshape(-1, items)
        args.mask_ids, args.masks, args.n_masks = ids.ctypes.data, m.ctypes.data if m.size else None, m.shape[0]
    api.check(_fn(a)(dm.h, C.byref(args), None))
    return o.copy()


def assert_blend_equal(got, want, e, what):
    """Bit for bit; a mixed item in which the expectation holds a NaN: NaN at the same positions, the other floats bit for bit."""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    assert got.shape == want.shape, what
    mixed = np.broadcast_to((mb.side_of(e) == 2).reshape(e.shape + (1,) * (got.ndim - 2)), got.shape)
    loose = mixed & np.isnan(want)
    assert np.isnan(got[loose]).all(), what + ": NaN positions"
    gu.assert_bits_equal(np.where(loose, np.float32(0), got), np.where(loose, np.float32(0), want), what)


# ---- the libmmd fixture ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("out", ["separate", "a", "b"])
@pytest.mark.parametrize("where", ["device", "host"])
def test_gpu_fixture_rows_equal_libmmd(dm, where, out):
    z = rb.fixture()
    run = run_device if where == "device" else run_host
    gu.assert_bits_equal(run(dm, z["a_poses"], z["b_poses"], z["weights"], z["bone_masks"], z["mask_ids"], out), z["expect_poses"],
                         f"poses ({where} operands, out {out})")
    gu.assert_bits_equal(run(dm, z["a_rates"], z["b_rates"], z["weights"], z["morph_masks"], z["mask_ids"], out), z["expect_rates"],
                         f"rates ({where} operands, out {out})")


def test_gpu_python_face_equals_the_fixture(dm):
    z = rb.fixture()
    gu.assert_bits_equal(vmd.blend_poses(z["a_poses"], z["b_poses"], z["weights"], z["bone_masks"], z["mask_ids"], model=dm),
                         z["expect_poses"], "vmd.blend_poses")
    gu.assert_bits_equal(vmd.blend_rates(z["a_rates"], z["b_rates"], z["weights"], z["morph_masks"], z["mask_ids"], model=dm),
                         z["expect_rates"], "vmd.blend_rates")
    none = z["mask_ids"] == NONE
    gu.assert_bits_equal(vmd.blend_poses(z["a_poses"][none], z["b_poses"][none], z["weights"][none], model=dm), z["expect_poses"][none],
                         "vmd.blend_poses without masks")


# ---- seeded random rows at the shapes where the kernels can go wrong ----------------------------------------------------------------
def _random_case(ni, items, seed):
    """Poses and rates with non-unit quaternions, a few NaN / infinite entries and -0.0; three mask rows with values outside [0, 1];
    mask ids of every kind; weights of every class."""
    rng = np.random.RandomState(seed)
    poses = []
    for _ in range(2):
        p = rng.uniform(-2, 2, (ni, items, 8)).astype(np.float32)
        p[..., 3] = 0
        p[..., 4:] *= rng.uniform(0.2, 3.0, (ni, items, 1)).astype(np.float32)          # not unit length
        flat = p.reshape(-1)
        k = max(1, flat.size // 97)
        flat[rng.choice(flat.size, k, replace=False)] = np.float32(-0.0)
        flat[rng.choice(flat.size, max(1, k // 3), replace=False)] = np.float32(np.nan)
        flat[rng.choice(flat.size, max(1, k // 3), replace=False)] = np.float32(np.inf) * rng.choice([-1, 1])
        poses.append(p)
    poses[0][0, 0, 3] = np.float32(5.0)            # a fourth translation float that is not 0: copied on sides A and B, 0 when mixed
    rates = [rng.uniform(-0.5, 1.5, (ni, items)).astype(np.float32) for _ in range(2)]
    rates[0].reshape(-1)[::53] = np.float32(-0.0)
    rates[1].reshape(-1)[::71] = np.float32(np.nan)
    masks = rng.choice(np.array([0, 0.25, 0.5, 1, 1, -0.5, 2.0, 1e-7, 4e6], np.float32), (3, items)).astype(np.float32)
    masks[2] = np.float32(1)                       # a row that changes nothing
    ids = rng.choice(np.array([NONE, 0, 1, 2, 3, 77, 0xFFFFFFFE], np.uint32), ni).astype(np.uint32)      # 3, 77, ...: out of range
    w = np.r_[mb.WEIGHTS, np.float32(np.nan), rng.uniform(0, 1, 64).astype(np.float32)].astype(np.float32)[rng.permutation(75)[:ni]]
    return poses, rates, masks, ids, w


@pytest.mark.parametrize("ni", [1, 3, 65])
@pytest.mark.parametrize("items", [1, 63, 64, 65, 257])
def test_gpu_random_rows_equal_the_restatement(dm, items, ni):
    poses, rates, masks, ids, w = _random_case(ni, items, 1000 * items + ni)
    e = rb.effective_weights(w, items, masks, ids)
    want_p, want_r = rb.blend_poses(*poses, w, masks, ids), rb.blend_rates(*rates, w, masks, ids)
    for out in ("separate", "a", "b"):
        got = run_device(dm, *poses, w, masks, ids, out)
        assert_blend_equal(got, want_p, e, f"poses, out {out}")
        assert_blend_equal(run_device(dm, *rates, w, masks, ids, out), want_r, e, f"rates, out {out}")
    # without mask ids the masks are not looked at
    e = rb.effective_weights(w, items)
    assert_blend_equal(run_device(dm, *poses, w), rb.blend_poses(*poses, w), e, "poses, no masks")
    assert_blend_equal(run_device(dm, *rates, w), rb.blend_rates(*rates, w), e, "rates, no masks")


def test_gpu_every_side_and_mask_id_case_occurs_in_the_random_rows():
    sides, kinds = set(), set()
    for items in (63, 257):
        _, _, masks, ids, w = _random_case(65, items, 1000 * items + 65)
        e = rb.effective_weights(w, items, masks, ids)
        sides |= set(np.unique(mb.side_of(e)))
        kinds |= {"none" if i == NONE else "valid" if i < 3 else "out of range" for i in ids}
        assert np.isnan(w).any() and (masks < 0).any() and (masks > 1).any()
    assert sides == {0, 1, 2} and kinds == {"none", "valid", "out of range"}


# ---- B is not read where it is not needed -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("out", ["separate", "a"])
def test_gpu_b_is_not_read_where_it_is_not_needed(dm, out):
    """B rows of instances with weight 0 or NaN and B items under mask value 0 hold a NaN pattern; so do the B items of instances
    with an out-of-range mask id.  The output is what clean B rows give, and A's bits at those items."""
    ni, items = 65, 65
    rng = np.random.RandomState(7)
    a = rng.uniform(-1, 1, (ni, items, 8)).astype(np.float32)
    b = rng.uniform(-1, 1, (ni, items, 8)).astype(np.float32)
    ra, rbb = rng.uniform(0, 1, (ni, items)).astype(np.float32), rng.uniform(0, 1, (ni, items)).astype(np.float32)
    masks = rng.choice(np.array([0, 0, 0.5, 1], np.float32), (2, items)).astype(np.float32)
    ids = rng.choice(np.array([0, 1, NONE, 9], np.uint32), ni).astype(np.uint32)
    w = rng.choice(np.array([0, -0.0, np.nan, 0.3, 1.0, 1.0], np.float32), ni).astype(np.float32)
    e = rb.effective_weights(w, items, masks, ids)
    unneeded = mb.side_of(e) == 0
    assert unneeded[(w == 0) | np.isnan(w)].all() and unneeded[ids == 9].all() and 0.3 < unneeded.mean() < 0.9
    b_poison, r_poison = b.copy(), rbb.copy()
    b_poison[unneeded] = POISON
    r_poison[unneeded] = POISON
    got_p, got_r = run_device(dm, a, b_poison, w, masks, ids, out), run_device(dm, ra, r_poison, w, masks, ids, out)
    gu.assert_bits_equal(got_p, rb.blend_poses(a, b, w, masks, ids), "poses")
    gu.assert_bits_equal(got_r, rb.blend_rates(ra, rbb, w, masks, ids), "rates")
    gu.assert_bits_equal(got_p[unneeded], a[unneeded], "A's items")
    gu.assert_bits_equal(got_r[unneeded], ra[unneeded], "A's rates")


def test_gpu_in_place_with_every_weight_zero_or_nan_leaves_the_array_as_it_is(dm):
    """out == a, every weight 0, -0 or NaN: the kernel may return before it loads anything, and the array must come back byte for
    byte, NaN payloads and non-zero fourth floats included."""
    ni, items = 65, 257
    rng = np.random.RandomState(9)
    a = rng.uniform(-1, 1, (ni, items, 8)).astype(np.float32)
    a.reshape(-1)[::31] = POISON
    b = np.full_like(a, POISON)
    w = np.array([0.0, -0.0, np.nan], np.float32)[np.arange(ni) % 3]
    masks = np.array([[2.0] * items, [np.inf] * items], np.float32)          # 0 * inf = NaN: still A
    ids = np.array([0, 1, NONE, 5], np.uint32)[np.arange(ni) % 4]
    gu.assert_bits_equal(run_device(dm, a, b, w, masks, ids, "a"), a, "poses in place")
    gu.assert_bits_equal(run_device(dm, a, b, w, masks, ids, "separate"), a, "poses copied")
    ra = a[..., 0].copy()
    gu.assert_bits_equal(run_device(dm, ra, b[..., 0].copy(), w, masks, ids, "a"), ra, "rates in place")
    gu.assert_bits_equal(run_device(dm, ra, b[..., 0].copy(), w, masks, ids, "separate"), ra, "rates copied")


# ---- the no-mask call is the set's blend --------------------------------------------------------------------------------------------
def _fixture_set(z):
    bvs, mvs = [vmd.Vmd(p) for p in mb.BONE_VMDS], [vmd.Vmd(p) for p in mb.MORPH_VMDS]
    bms, mms = [v.bind_bones(z["bone_names"]) for v in bvs], [v.bind_morphs(z["morph_names"]) for v in mvs]
    ms = vmd.MotionSet(bms, mms)
    _close(bms, mms, bvs, mvs)
    return ms


def test_gpu_no_mask_call_is_the_blend_of_the_motion_set(dm):
    """On the fixture's set and clocks: mmdx_pose_blend(eval(a), eval(b), w) without masks is byte for byte
    mmdx_motion_set_blend_bones_time, mmdx_rate_blend the same against _blend_morphs_time; separate output and in place."""
    z = rb.fixture()
    n, nb, nm = z["weights"].size, len(z["bone_names"]), len(z["morph_names"])
    ms = _fixture_set(z)
    ds = [DeviceBuffer.from_numpy(np.ascontiguousarray(z[k], t)) for k, t in
          (("clips_a", np.uint32), ("times_a", np.float64), ("clips_b", np.uint32), ("times_b", np.float64), ("weights", np.float32))]
    d_ca, d_ta, d_cb, d_tb, d_w = ds
    for bones in (True, False):
        items, floats = (nb, 8) if bones else (nm, 1)
        shape = (n, items, 8) if bones else (n, items)
        d_a, d_b, d_want, d_got = (DeviceBuffer(n * items * floats * 4) for _ in range(4))
        ev = ms.eval_bones_time_device if bones else ms.eval_morphs_time_device
        ev(n, d_ca.ptr, d_ta.ptr, d_a.ptr, dm)
        ev(n, d_cb.ptr, d_tb.ptr, d_b.ptr, dm)
        (ms.blend_bones_time_device if bones else ms.blend_morphs_time_device)(n, *[d.ptr for d in ds], d_want.ptr, dm)
        blend = vmd.blend_poses_device if bones else vmd.blend_rates_device
        d_got.memset(SENT)
        blend(n, items, d_a.ptr, d_b.ptr, d_w.ptr, d_got.ptr, model=dm)
        dm.sync()
        want = d_want.download(shape, np.float32)
        gu.assert_bits_equal(d_got.download(shape, np.float32), want, "separate output")
        blend(n, items, d_a.ptr, d_b.ptr, d_w.ptr, d_a.ptr, model=dm)
        dm.sync()
        gu.assert_bits_equal(d_a.download(shape, np.float32), want, "in place")
        _close(d_a, d_b, d_want, d_got)
    _close(ds, ms)


# ---- the select form ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("out", ["separate", "a"])
def test_gpu_select_writes_the_listed_rows_and_nothing_else(dm, out):
    ni, items = 65, 65
    poses, rates, masks, ids, w = _random_case(ni, items, 4242)
    rng = np.random.RandomState(5)
    lst = np.r_[rng.permutation(ni)[:20], [3, 3, ni, ni + 7, 0xFFFFFFFF], rng.permutation(ni)[:6]].astype(np.uint32)
    lst = lst[rng.permutation(lst.size)]
    assert (lst >= ni).sum() == 3 and np.unique(lst).size < lst.size
    if out == "a":          # in place an id is listed once: a second blend of the row would start from the first one's result
        lst = lst[np.sort(np.unique(lst, return_index=True)[1])]
    for a, b, what in ((poses[0], poses[1], "poses"), (rates[0], rates[1], "rates")):
        plain = run_device(dm, a, b, w, masks, ids, out)
        before = a if out == "a" else _sentinel(a)
        for count in (0, 1, 17, lst.size, None, lst.size + 9):
            used = lst[:lst.size if count is None else min(count, lst.size)]
            listed = np.zeros(ni, bool)
            listed[used[used < ni]] = True
            got = run_device(dm, a, b, w, masks, ids, out, select=(lst, count, True))
            gu.assert_bits_equal(got[listed], plain[listed], f"{what}, count {count}: listed rows")
            gu.assert_bits_equal(got[~listed], before[~listed], f"{what}, count {count}: every other byte")
            valid = used[used < ni]                                   # a host list may not hold an id >= NI
            host = run_device(dm, a, b, w, masks, ids, out, select=(valid, None, False))
            gu.assert_bits_equal(host, got, f"{what}, count {count}: host list")
        host = run_device(dm, a, b, w, masks, ids, out, select=(lst[lst < ni], 5, False))        # a host count below n_ids
        gu.assert_bits_equal(host, run_device(dm, a, b, w, masks, ids, out, select=(lst[lst < ni], 5, True)), what + ": host count")


def test_gpu_select_refuses_host_rows_and_bad_host_ids(dm):
    a = np.zeros((3, 5, 8), np.float32)
    d = DeviceBuffer.from_numpy(a)
    w, ids = np.zeros(3, np.float32), np.array([0, 3], np.uint32)
    args = api.RowBlendArgs(C.sizeof(api.RowBlendArgs), api.BLEND_A_ON_DEVICE | api.OUT_ON_DEVICE, 3, 5, d.ptr, a.ctypes.data,
                            w.ctypes.data, None, None, 0, 0, d.ptr)
    sel = vmd.instance_select(ids.ctypes.data, 1, None, on_device=False)
    assert api.lib().mmdx_pose_blend(dm.h, C.byref(args), C.byref(sel)) == 1
    assert b"a, b and out in device memory only" in api.lib().mmdx_last_error_string()
    d_b = DeviceBuffer.from_numpy(a)
    args.flags, args.b = api.BLEND_A_ON_DEVICE | api.BLEND_B_ON_DEVICE | api.OUT_ON_DEVICE, d_b.ptr
    sel = vmd.instance_select(ids.ctypes.data, 2, None, on_device=False)
    assert api.lib().mmdx_pose_blend(dm.h, C.byref(args), C.byref(sel)) == 1
    assert b"ids[1] = 3 is not below n_instances" in api.lib().mmdx_last_error_string()
    _close(d, d_b)


# ---- a recorded frame -----------------------------------------------------------------------------------------------------------------
def _layer_scene(ni, seed):
    rng = np.random.RandomState(seed)
    ops = lambda: (rng.randint(0, 2, ni).astype(np.uint32), rng.uniform(0, 5, ni), rng.randint(0, 2, ni).astype(np.uint32),      # noqa: E731
                   rng.uniform(0, 5, ni), rng.choice(np.array([0, 0.4, 1], np.float32), ni).astype(np.float32))
    return ops(), ops()


def test_gpu_tracks_layer_and_solve_record_into_one_graph(dm):
    """blend tracks (base) -> blend tracks (layer) -> mmdx_pose_blend in place -> mmdx_skeleton_solve, recorded once and replayed
    after the layer weights and the mask ids were rewritten in device memory: the palettes are the eager sequence's.  A host
    operand while recording is refused."""
    z = rb.fixture()
    zr = np.load(os.path.join(gu.GOLDEN_DIR, "rig_small_expect.npz"))
    nb, ni = len(z["bone_names"]), 65
    ms = _fixture_set(z)
    sk = vmd.Skeleton(zr["rest"], zr["parent"], zr["level"], zr["flags"])
    masks = np.stack([sk.subtree_mask([5]), sk.subtree_mask([2], 0.5, 0.0)])
    base, layer = _layer_scene(ni, 77)
    d_base = [DeviceBuffer.from_numpy(np.ascontiguousarray(x)) for x in base]
    d_layer = [DeviceBuffer.from_numpy(np.ascontiguousarray(x)) for x in layer]
    d_pose, d_lpose, d_pal = DeviceBuffer(ni * nb * 32), DeviceBuffer(ni * nb * 32), DeviceBuffer(ni * nb * 64)
    d_lw, d_ids, d_masks = DeviceBuffer(ni * 4), DeviceBuffer(ni * 4), DeviceBuffer.from_numpy(masks)

    def frame():
        ms.blend_bones_time_device(ni, *[d.ptr for d in d_base], d_pose.ptr, dm)
        ms.blend_bones_time_device(ni, *[d.ptr for d in d_layer], d_lpose.ptr, dm)
        vmd.blend_poses_device(ni, nb, d_pose.ptr, d_lpose.ptr, d_lw.ptr, d_pose.ptr, d_masks.ptr, 2, d_ids.ptr, model=dm)
        sk.solve_device(ni, d_pose.ptr, d_pal.ptr, dm)

    rng = np.random.RandomState(3)
    settings = [(rng.choice(np.array([0, 0.3, 1, np.nan], np.float32), ni).astype(np.float32),
                 rng.choice(np.array([0, 1, NONE, 6], np.uint32), ni).astype(np.uint32)) for _ in range(3)]
    eager = []
    for lw, ids in settings:
        d_lw.upload(lw); d_ids.upload(ids)
        frame()
        dm.sync()
        eager.append(d_pal.download((ni, nb, 16), np.float32))
    assert not np.array_equal(eager[0], eager[1])
    dm.graph_begin()
    frame()
    host_w = np.full(ni, 0.5, np.float32)
    args = api.RowBlendArgs(C.sizeof(api.RowBlendArgs), ALL & ~api.BLEND_PARAMS_ON_DEVICE, ni, nb, d_pose.ptr, d_lpose.ptr,
                            host_w.ctypes.data, None, None, 0, 0, d_pose.ptr)
    assert api.lib().mmdx_pose_blend(dm.h, C.byref(args), None) == 1
    assert b"while a graph is being recorded a, b, weights, mask_ids, masks and out must all be in device memory" in \
        api.lib().mmdx_last_error_string()
    args.flags, args.weights = ALL, d_lw.ptr
    hl = np.array([0], np.uint32)
    sel = vmd.instance_select(hl.ctypes.data, 1, None, on_device=False)
    assert api.lib().mmdx_pose_blend(dm.h, C.byref(args), C.byref(sel)) == 1
    assert b"the instance list must be in device memory" in api.lib().mmdx_last_error_string()
    g = dm.graph_end()
    for k in (2, 0, 1):
        lw, ids = settings[k]
        d_lw.upload(lw); d_ids.upload(ids)
        d_pal.memset(SENT)
        g.launch()
        dm.sync()
        gu.assert_bits_equal(d_pal.download((ni, nb, 16), np.float32), eager[k], f"replay with setting {k}")
    g.close()
    _close(d_base, d_layer, d_pose, d_lpose, d_pal, d_lw, d_ids, d_masks, ms, sk)


# ---- end to end on rig_small ----------------------------------------------------------------------------------------------------------
def test_gpu_layered_palettes_equal_the_oracle_solve_of_the_numpy_blend(dm, oracle):
    """Fixture rows as base and layer, an upper-body mask from the hierarchy: the palettes mmdx_skeleton_solve makes of the layered
    poses are the oracle's bone solve of the numpy-blended poses."""
    z = rb.fixture()
    zr = np.load(os.path.join(gu.GOLDEN_DIR, "rig_small_expect.npz"))
    sk = vmd.Skeleton(zr["rest"], zr["parent"], zr["level"], zr["flags"])
    children = [int(b) for b in np.flatnonzero(zr["parent"] >= 0)]
    root = children[len(children) // 3]
    masks = np.stack([sk.subtree_mask([root]), sk.subtree_mask([root, children[-1]], 0.5, 0.25)])
    assert 0 < masks[0].sum() < masks[0].size
    rows = np.arange(0, z["weights"].size, 11)
    a, b = z["a_poses"][rows], z["b_poses"][rows]
    w = np.array([0.0, 0.3, 1.0, 0.75], np.float32)[np.arange(rows.size) % 4]
    ids = np.array([0, 1, NONE], np.uint32)[np.arange(rows.size) % 3]
    layered = vmd.blend_poses(a, b, w, masks, ids, model=dm)
    want = rb.blend_poses(a, b, w, masks, ids)
    gu.assert_bits_equal(layered, want, "layered poses")
    pal = sk.solve(layered, dm)
    for i in range(rows.size):
        gu.assert_bits_equal(pal[i], oracle.bone_solve(zr["rest"], zr["parent"], want[i], zr["level"], zr["flags"]), f"palette of row {i}")
    sk.close()

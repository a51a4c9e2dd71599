"""mmdx_skeleton_solve_select: the bone solve for a listed subset of a crowd (include/mmdx.h, rules 1-10).

The expected value everywhere is the PLAIN call on the same operands -- Skeleton.solve / mmdx_skeleton_solve_morphed, which
tests/test_rig.py pins bit for bit against libmmd -- compared with golden_util.assert_bits_equal, no tolerance: listed rows carry
the plain call's bytes, every other byte of the palette array keeps the pattern it held before the call (0xA5), and the pose and
rate rows of unlisted instances hold NaN.  Shapes: 70 instances, lists that straddle 16 (instances per workgroup of the ordered
kernel, solves per block of ik_coop_kernel); 4 300 instances once, for the two-workgroups-per-CU variant.
CPU tests: the symbol, and every argument error before the device is touched."""
import ctypes as C

import numpy as np
import pytest

from simple_mmd_renderer_amd import _capi as api
from simple_mmd_renderer_amd import synth, vmd
from simple_mmd_renderer_amd.engine import DeformModel, DeviceBuffer, device_count, planes_from_matrix
from tests import golden_util as gu
from tests import palette_place_ref as pp
from tests.test_cull_bounds import F, SENT, View, look_at, mat_mul, perspective
from tests.test_rig import NESTED_CASES, random_poses

NI = 70
PATTERN = 0xA5
DEV = vmd.POSES_ON_DEVICE | api.OUT_ON_DEVICE


@pytest.fixture(autouse=True)
def _lib(hip_lib):
    return hip_lib


def pattern(ni, nb):
    return np.full((ni, nb, 16), PATTERN * 0x01010101, np.uint32).view(np.float32)


def listed_rows(ids, count, ni):
    """The rows a call with this list writes: the first min(count, len) ids that are rows of the arrays."""
    ids = np.asarray(ids, np.uint32)
    live = ids[:ids.size if count is None else min(int(count), ids.size)]
    rows = np.zeros(ni, bool)
    rows[live[live < ni]] = True
    return rows


def nan_unlisted(a, rows):
    a = np.array(a, np.float32)
    a[~rows] = np.nan
    return a


def check(got, want, rows, what):
    """Listed rows: the plain call's bits.  Everything else: the pattern, byte for byte."""
    gu.assert_bits_equal(got[rows], want[rows], what + ": listed rows differ from the plain call")
    assert (got[~rows].view(np.uint8) == PATTERN).all(), what + ": a row that is not listed was written"


# ---------------------------------------------------------------------------------------- CPU ----
def test_library_exports_solve_select_and_binding_declares_it():
    assert hasattr(api.lib(), "mmdx_skeleton_solve_select")
    assert "mmdx_skeleton_solve_select" in api.SIGNATURES
    assert len(api.SIGNATURES["mmdx_skeleton_solve_select"][1]) == 8


def test_argument_errors_precede_any_device_call():
    """Every refusal of rules 5 and 6, NULL arguments and n_instances == 0 are MMDX_ERR_INVALID_ARGUMENT -- on a machine without a
    GPU too, where the first call that reaches the device would say MMDX_ERR_NO_DEVICE instead.  Pointers are never followed."""
    lib = api.lib()
    rest, parent, level, flags = synth.make_skeleton(3, 1)
    sk = vmd.Skeleton(rest, parent, level, flags)
    poses, pal, w = 0x1000, 0x2000, 0x3000                       # "device" addresses: validation must not look behind them
    ids = np.array([0, 1], np.uint32)

    def sel(flags=api.SELECT_ON_DEVICE, size=C.sizeof(api.InstanceSelect), ids_ptr=0x4000, count=None, n_ids=2, reserved0=0):
        s = api.InstanceSelect()
        s.struct_size, s.flags, s.ids, s.count, s.n_ids, s.reserved0 = size, flags, ids_ptr, count, n_ids, reserved0
        return s

    def call(s=None, sk_h=sk.h, ni=2, poses=poses, w=None, flags=DEV, pal=pal, select="default"):
        s = sel() if s is None else s
        st = lib.mmdx_skeleton_solve_select(sk_h, None, ni, poses, w, flags, None if select is None else C.byref(s), pal)
        return st, lib.mmdx_last_error_string().decode()

    assert call(sk_h=None)[0] == 1 and call(poses=None)[0] == 1 and call(pal=None)[0] == 1
    st, msg = call(ni=0)
    assert st == 1 and "n_instances" in msg
    for fl in (0, vmd.POSES_ON_DEVICE, api.OUT_ON_DEVICE):                           # missing *_ON_DEVICE bits
        st, msg = call(flags=fl)
        assert st == 1 and "device operands only" in msg, (fl, msg)
    st, msg = call(w=w)                                                              # rates without MMDX_WEIGHTS_ON_DEVICE
    assert st == 1 and "MMDX_WEIGHTS_ON_DEVICE" in msg
    st, msg = call(w=w, flags=DEV | api.WEIGHTS_SHARED)
    assert st == 1 and "MMDX_WEIGHTS_ON_DEVICE" in msg
    for bit in (vmd.FRAMES_ON_DEVICE, 32, api.OUT_PITCHED, 1 << 9, 1 << 31):         # bits of other calls, unknown bits
        st, msg = call(flags=DEV | bit)
        assert st == 1 and "unknown flag bits" in msg, (bit, msg)
    st, msg = call(select=None)
    assert st == 1 and "select is NULL" in msg
    st, msg = call(sel(size=C.sizeof(api.InstanceSelect) - 4))
    assert st == 1 and "struct_size" in msg
    st, msg = call(sel(flags=api.SELECT_ON_DEVICE | 2))
    assert st == 1 and "mmdx_instance_select.flags" in msg
    st, msg = call(sel(reserved0=1))
    assert st == 1 and "reserved0" in msg
    st, msg = call(sel(ids_ptr=None))
    assert st == 1 and "ids is NULL" in msg
    st, msg = call(sel(ids_ptr=0x4002))
    assert st == 1 and "aligned" in msg
    # a host list is read on the host: an id that is no row fails there, inside the count only
    bad = np.array([1, 2, 0], np.uint32)
    st, msg = call(sel(flags=0, ids_ptr=bad.ctypes.data, n_ids=3))
    assert st == 1 and "ids[1] = 2" in msg
    two = np.array([2], np.uint32)
    st, msg = call(sel(flags=0, ids_ptr=bad.ctypes.data, count=two.ctypes.data, n_ids=3))
    assert st == 1 and "ids[1] = 2" in msg
    n = C.c_int32()
    if lib.mmdx_device_count(C.byref(n)) != 0 or n.value < 1:      # this machine has no GPU: valid arguments must say so, not compute
        one = np.array([1], np.uint32)                             # (an id behind the count is not looked at)
        st, msg = call(sel(flags=0, ids_ptr=bad.ctypes.data, count=one.ctypes.data, n_ids=3))
        assert st == 3 and "no HIP device" in msg
        st, msg = call(sel(flags=0, ids_ptr=ids.ctypes.data, n_ids=2))
        assert st == 3 and "no HIP device" in msg
        st, msg = call()
        assert st == 3 and "no HIP device" in msg


# ---------------------------------------------------------------------------------------- GPU ----
RIGS = {
    "fk": lambda: synth.make_ik_rig(30, 0, n_ik=0, n_append=0),
    "ik44": lambda: synth.make_ik_rig(44, 1, n_ik=3, n_append=4),
    "nested": lambda: synth.make_nested_ik_rig(*NESTED_CASES[1]),
    "ik300": lambda: synth.make_ik_rig(300, 7, n_ik=8, n_append=12),
}
_cases = {}


def case(name, coop=None):
    """(rig, skeleton, poses [NI], the plain call's palettes): computed once per rig and IK kernel, shared, never written."""
    key = (name, coop)
    if key not in _cases:
        rig = RIGS[name]()
        nb = rig[0].shape[0]
        sk = vmd.Skeleton(*rig)
        poses = random_poses(NI, nb, 1300 + nb)
        want = sk.solve(poses)
        for a in (poses, want):
            a.setflags(write=False)
        _cases[key] = (rig, sk, poses, want)
    return _cases[key]


def run(sk, poses, ids, count, out_before=None, model=None, rates=None, host_list=False, n_ids=None):
    """One select call through the raw entry point: poses / rates as given, the palette array holding the pattern before the call;
    returns the WHOLE palette array.  count None = no count word."""
    p = np.ascontiguousarray(poses, np.float32)
    ni, nb = p.shape[0], p.shape[1]
    ids = np.ascontiguousarray(ids, np.uint32)
    n_ids = ids.size if n_ids is None else n_ids
    d_pose = DeviceBuffer.from_numpy(p)
    d_out = DeviceBuffer.from_numpy(pattern(ni, nb) if out_before is None else out_before)
    bufs = [d_pose, d_out]
    w_ptr, shared = None, False
    if rates is not None:
        bufs.append(DeviceBuffer.from_numpy(np.ascontiguousarray(rates, np.float32)))
        w_ptr, shared = bufs[-1].ptr, np.ndim(rates) == 1
    cnt = None if count is None else np.array([count], np.uint32)
    if host_list:
        sk.solve_select_device(ni, d_pose.ptr, d_out.ptr, ids.ctypes.data, n_ids, cnt.ctypes.data if cnt is not None else None, model,
                               w_ptr, shared, select_on_device=False)
    else:
        bufs.append(DeviceBuffer.from_numpy(ids if ids.size else np.zeros(1, np.uint32)))
        ids_ptr = bufs[-1].ptr
        cnt_ptr = None
        if cnt is not None:
            bufs.append(DeviceBuffer.from_numpy(cnt))
            cnt_ptr = bufs[-1].ptr
        sk.solve_select_device(ni, d_pose.ptr, d_out.ptr, ids_ptr, n_ids, cnt_ptr, model, w_ptr, shared)
        api.check(api.lib().mmdx_sync(model.h) if model is not None else api.lib().mmdx_device_synchronize())
    got = d_out.download((ni, nb, 16), np.float32)               # (a host-list call has completed when it returns)
    for b in bufs:
        b.free()
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("name,coop", [("fk", None), ("ik44", "0"), ("ik44", "1"), ("nested", "0"), ("nested", "1"), ("ik300", None)])
def test_gpu_every_solver_listed_rows_and_untouched_rows(monkeypatch, oracle, name, coop):
    """Device lists in random order, counts 0, 1, 16, 17, 37 and 70 of a capacity of 70, and no count word with a capacity of 17."""
    assert device_count() >= 1, "no HIP device visible: the GPU tests must run on the MI355X box"
    if coop is not None:
        monkeypatch.setenv("MMDX_IK_COOP", coop)                  # (read per call; the plain reference runs under it too)
    rig, sk, poses, want = case(name, coop)
    assert sk.info["solver"] == (vmd.SOLVER_PARALLEL_FK if name == "fk" else vmd.SOLVER_SERIAL)
    ids = np.random.RandomState(len(name)).permutation(NI).astype(np.uint32)
    for count in (0, 1, 16, 17, 37, 70):
        rows = listed_rows(ids, count, NI)
        assert rows.sum() == count
        check(run(sk, nan_unlisted(poses, rows), ids, count), want, rows, f"{name}: count {count}")
    rows = listed_rows(ids[:17], None, NI)
    got = run(sk, nan_unlisted(poses, rows), ids[:17], None)
    check(got, want, rows, f"{name}: 17 ids, no count word")
    if name == "ik44" and coop == "1":                            # and a few listed rows against the checker itself
        for i in ids[[0, 8, 16]]:
            gu.assert_bits_equal_or_both_nan(got[i], oracle.bone_solve_full(rig[0], rig[1], poses[i], *rig[2:]), f"oracle, row {i}")


@pytest.mark.gpu
def test_gpu_convenience_call_equals_raw_call():
    """Skeleton.solve_select (uploads, calls, downloads the whole array) on the 37-of-70 list."""
    rig, sk, poses, want = case("ik44")
    ids = np.random.RandomState(4).permutation(NI).astype(np.uint32)
    rows = listed_rows(ids, 37, NI)
    check(sk.solve_select(nan_unlisted(poses, rows), ids, 37, out=pattern(NI, sk.nb)), want, rows, "convenience call")
    zero = sk.solve_select(poses, ids, 0)
    assert not zero.any()                                         # out=None: zeros before the call, and an empty list writes nothing


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["ik44", "fk"])
def test_gpu_bone_morphs_per_instance_and_shared(name):
    """make_bone_morphs on both solvers, rates as in test_gpu_bone_morphs_vs_oracle (the 5e-8 skip among them), 23 of 70 listed."""
    rig = RIGS[name]()
    nb = rig[0].shape[0]
    morphs = synth.make_bone_morphs(nb, 90 + (1 if name == "ik44" else 0))
    nm = morphs["type"].size
    sk = vmd.Skeleton(*rig, morphs)
    assert sk.info["n_bone_morph_entries"] > 0
    poses = random_poses(NI, nb, 500 + nb)
    rates = np.random.RandomState(nb).choice([0, 5e-8, 0.3, 1.0, 1.7, -0.5], (NI, nm)).astype(np.float32)
    ids = np.random.RandomState(23).permutation(NI)[:23].astype(np.uint32)
    rows = listed_rows(ids, None, NI)
    per, shared, plain = sk.solve(poses, morph_weights=rates), sk.solve(poses, morph_weights=rates[3]), sk.solve(poses)
    assert not np.array_equal(gu.bits(per), gu.bits(plain))       # the morphs really move bones
    check(run(sk, nan_unlisted(poses, rows), ids, 23, rates=nan_unlisted(rates, rows)), per, rows, name + ": per-instance rates")
    check(run(sk, nan_unlisted(poses, rows), ids, 23, rates=rates[3]), shared, rows, name + ": shared rates")
    check(run(sk, nan_unlisted(poses, rows), ids, 23), plain, rows, name + ": no rates")


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["ik44", "fk"])
def test_gpu_duplicates_and_out_of_range_device_ids(name):
    """[5, 5, 69, 70, 0xFFFFFFFF, 12, 5]: rows 5, 12 and 69 are the plain call's, nothing else is written, and the stream is
    healthy afterwards (run() synchronises and checks the status)."""
    rig, sk, poses, want = case(name)
    ids = np.array([5, 5, 69, 70, 0xFFFFFFFF, 12, 5], np.uint32)
    rows = listed_rows(ids, None, NI)
    assert np.flatnonzero(rows).tolist() == [5, 12, 69]
    with DeformModel(synth.make_model(120, 4, 2, 10, seed=1)) as dm:
        check(run(sk, nan_unlisted(poses, rows), ids, 7, model=dm), want, rows, name + ": count word")
        check(run(sk, nan_unlisted(poses, rows), ids, None, model=dm), want, rows, name + ": no count word")
        dm.sync()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["ik44", "fk"])
def test_gpu_host_list_equals_device_list(name):
    """The 23-of-70 list with ids and count in host memory: identical output, readable as soon as the call returns; a capacity
    above the count, ids behind the count that are no rows."""
    rig, sk, poses, want = case(name)
    ids = np.random.RandomState(23).permutation(NI)[:23].astype(np.uint32)
    rows = listed_rows(ids, None, NI)
    p = nan_unlisted(poses, rows)
    dev = run(sk, p, ids, 23)
    check(dev, want, rows, name + ": device list")
    gu.assert_bits_equal(run(sk, p, ids, 23, host_list=True), dev, name + ": host list")
    gu.assert_bits_equal(run(sk, p, ids, None, host_list=True), dev, name + ": host list, no count word")
    padded = np.r_[ids, np.full(9, 1000, np.uint32)].astype(np.uint32)
    gu.assert_bits_equal(run(sk, p, padded, 23, host_list=True), dev, name + ": host list, capacity above the count")
    assert (run(sk, p, ids, 0, host_list=True).view(np.uint8) == PATTERN).all()


@pytest.mark.gpu
def test_gpu_recorded_select_solve_reads_list_and_count_at_replay():
    """One eager run, then the select solve recorded with a device list; every replay is correct for the ids and the count device
    memory holds at that moment.  A host list is refused while recording; once the graph exists, a call whose capacity would grow
    the skeleton's pinned scratch is refused (the pin rule of every recorded solve)."""
    rig = RIGS["ik44"]()
    sk = vmd.Skeleton(*rig)                                       # its own skeleton: the graph pins its scratch
    nb = sk.nb
    poses = random_poses(NI, nb, 1300 + nb)
    want = sk.solve(poses)
    cap = 40
    rs = np.random.RandomState(9)
    with DeformModel(synth.make_model(120, 4, 2, 10, seed=1)) as dm:
        d_pose, d_out = DeviceBuffer(poses.nbytes), DeviceBuffer(want.nbytes)
        d_ids, d_cnt = DeviceBuffer(cap * 4), DeviceBuffer(4)
        lists = [(rs.permutation(NI)[:cap].astype(np.uint32), n) for n in (17, 40, 0, 33)]

        def stage(ids, n):
            rows = listed_rows(ids, n, NI)
            d_pose.upload(nan_unlisted(poses, rows))
            d_out.upload(pattern(NI, nb))
            d_ids.upload(ids)
            d_cnt.upload(np.array([n], np.uint32))
            return rows

        rows = stage(*lists[0])
        sk.solve_select_device(NI, d_pose.ptr, d_out.ptr, d_ids.ptr, cap, d_cnt.ptr, dm)
        dm.sync()
        check(d_out.download((NI, nb, 16), F), want, rows, "eager run")
        dm.graph_begin()
        sk.solve_select_device(NI, d_pose.ptr, d_out.ptr, d_ids.ptr, cap, d_cnt.ptr, dm)
        with pytest.raises(api.MmdxError, match="MMDX_SELECT_ON_DEVICE") as e:
            sk.solve_select_device(NI, d_pose.ptr, d_out.ptr, lists[0][0].ctypes.data, cap, None, dm, select_on_device=False)
        assert e.value.status == 1
        graph = dm.graph_end()
        for k, (ids, n) in enumerate(lists[1:]):
            rows = stage(ids, n)
            graph.launch()
            dm.sync()
            check(d_out.download((NI, nb, 16), F), want, rows, f"replay {k}: {n} of {cap}")
        big = DeviceBuffer.from_numpy((np.arange(3 * NI) % NI).astype(np.uint32))   # more cells than any call before sized
        with pytest.raises(api.MmdxError, match="recorded") as e:
            sk.solve_select_device(NI, d_pose.ptr, d_out.ptr, big.ptr, 3 * NI, None, dm)
        assert e.value.status == 1
        graph.close()
        for b in (d_pose, d_out, d_ids, d_cnt, big):
            b.free()


@pytest.mark.gpu
def test_gpu_select_beyond_one_workgroup_per_cu():
    """4 200 distinct ids of 4 300 instances in random order: more workgroups than CUs, so the select form of the ordered solver's
    two-workgroups-per-CU variant runs (the shape of test_gpu_ik_skeleton_crowd_beyond_one_workgroup_per_cu).  Every listed row
    against the plain call on all 4 300, the 100 others for the pattern."""
    nb, ni, k = 44, 4300, 4200
    rig = RIGS["ik44"]()
    sk = vmd.Skeleton(*rig)
    poses = np.tile(random_poses(300, nb, 977), (ni // 300 + 1, 1, 1))[:ni]
    poses[..., 0:3] += np.random.RandomState(5).uniform(-0.2, 0.2, (ni, nb, 3)).astype(np.float32)
    want = sk.solve(poses)
    ids = np.random.RandomState(6).permutation(ni)[:k].astype(np.uint32)
    rows = listed_rows(ids, None, ni)
    assert rows.sum() == k
    check(run(sk, nan_unlisted(poses, rows), ids, k), want, rows, "4 200 of 4 300")
    shape = sk.last_solve_shape()                                 # by crowd size alone: MMDX_SOLVE_DENSE is not set here
    assert shape["solver"] == "ordered" and shape["select"] == 1 and shape["dense"] == 1 and shape["workgroups"] == (k + 15) // 16, shape
    small = np.arange(NI, dtype=np.uint32)
    check(run(sk, poses[:NI], small, NI), want[:NI], np.ones(NI, bool), "the first 70 alone")
    shape = sk.last_solve_shape()
    assert shape["solver"] == "ordered" and shape["select"] == 1 and shape["dense"] == 0 and shape["workgroups"] == 5, shape


@pytest.mark.gpu
def test_gpu_recorded_cull_solve_select_place_bounds_cull_deform_select_loop():
    """The loop for IK rigs, small, as one graph: mmdx_cull_bounds on last frame's boxes -> mmdx_skeleton_solve_select with list 0
    -> mmdx_palette_place -> mmdx_palette_bounds -> mmdx_cull_bounds -> mmdx_deform_batched_select, replayed with the view rewritten.
    Last frame's boxes are those of the unselected sequence (plain solve, same place), so what the second cull lists was solved; an
    instance that was not solved keeps the model-space palette it had (here the pattern: a matrix of ~-3e-16, which places its box
    at the origin, outside both views).  For the instances of the final list the vertices equal the unselected sequence's."""
    nb, nv, spacing = 44, 600, 12.0
    rig = RIGS["ik44"]()
    m = synth.make_model(nv, nb, 8, 64, seed=7500)
    rates = synth.morph_weights(m.nm, np.arange(NI) * 3)
    sk = vmd.Skeleton(*rig)
    poses = random_poses(NI, nb, 1300 + nb)
    model_space = sk.solve(poses)
    place = np.zeros((NI, 8), F)
    place[:, 0] = (np.arange(NI) - NI / 2) * spacing
    yaw = 0.05 + 0.03 * np.arange(NI)
    place[:, 5], place[:, 7] = np.sin(yaw / 2), np.cos(yaw / 2)

    def camera(x, fov):
        eye = (x, 10.0, 80.0)
        cam = mat_mul(perspective(fov, 1.0, 0.1, 1000.0), look_at(eye, (x, 10.0, 0.0)))
        return View(planes_from_matrix(cam, True), 6, 1, eye, 0.0, (0.0, 0.0, 0.0))

    views = [camera(-150.0, 50.0), camera(200.0, 35.0), camera(-300.0, 40.0)]
    dev = api.PALETTE_ON_DEVICE | api.OUT_ON_DEVICE
    with DeformModel(m) as dm:
        na, nbytes_b = dm.out_sizes(api.OUT_SOA, NI)
        d_pose, d_model = DeviceBuffer.from_numpy(poses), DeviceBuffer(model_space.nbytes)
        d_place, d_pal = DeviceBuffer.from_numpy(place), DeviceBuffer(model_space.nbytes)
        d_last, d_bnd = DeviceBuffer(NI * 24), DeviceBuffer(NI * 24)
        d_ids0, d_cnt0, d_ids, d_cnt = DeviceBuffer(NI * 4), DeviceBuffer(16), DeviceBuffer(NI * 4), DeviceBuffer(16)
        d_view = DeviceBuffer.from_numpy(np.frombuffer(bytes(views[0].struct()), np.uint8))
        d_a, d_b, d_w = DeviceBuffer(na), DeviceBuffer(nbytes_b), DeviceBuffer.from_numpy(rates)
        dflags = dev | api.WEIGHTS_ON_DEVICE
        # the unselected sequence: plain solve, place, palette bounds (= "last frame's boxes"), plain deform
        d_model.upload(model_space)
        dm.place_palettes(NI, d_model.ptr, d_place.ptr, d_pal.ptr, dev | api.PLACE_ON_DEVICE)
        dm.palette_bounds_raw(NI, d_pal.ptr, d_last.ptr, dev, 1.0, 1.0)
        dm.deform_batched_raw(NI, d_w.ptr, d_pal.ptr, d_a.ptr, d_b.ptr, api.OUT_SOA, dflags)
        dm.sync()
        gu.assert_bits_equal(d_pal.download(model_space.shape, F), pp.place_crowd(model_space, place, False), "placed palettes")
        want = [d_a.download((NI, nv * 12), np.uint8), d_b.download((NI, nv * 12), np.uint8)]
        boxes = d_last.download((NI, 6), F)

        def frame():
            dm.cull_bounds(d_last, d_view, NI, d_ids0, d_cnt0)
            sk.solve_select_device(NI, d_pose.ptr, d_model.ptr, d_ids0.ptr, NI, d_cnt0.ptr, dm)
            dm.place_palettes(NI, d_model.ptr, d_place.ptr, d_pal.ptr, dev | api.PLACE_ON_DEVICE)
            dm.palette_bounds_raw(NI, d_pal.ptr, d_bnd.ptr, dev, 1.0, 1.0)
            dm.cull_bounds(d_bnd, d_view, NI, d_ids, d_cnt)
            dm.deform_batched_raw(NI, d_w.ptr, d_pal.ptr, d_a.ptr, d_b.ptr, api.OUT_SOA, dflags, select_ptr=d_ids.ptr,
                                  select_count_ptr=d_cnt.ptr, n_select=NI)

        d_model.memset(PATTERN)
        frame()                                                   # once un-recorded: sizes every scratch
        dm.sync()
        dm.graph_begin()
        frame()
        graph = dm.graph_end()
        seen = []
        for k, view in enumerate(views):
            what = "replay %d" % k
            first = view.ref(boxes, True)[0][0]
            assert 0 < first.size < NI, what
            rows = listed_rows(first, None, NI)
            d_view.upload(np.frombuffer(bytes(view.struct()), np.uint8))
            d_pose.upload(nan_unlisted(poses, rows))              # a pose that is not listed is never read
            for buf in (d_model, d_a, d_b):
                buf.memset(PATTERN)
            for buf in (d_ids0, d_ids):
                buf.upload(np.full(NI, SENT, np.uint32))
            graph.launch()
            dm.sync()
            assert d_cnt0.download((4,), np.uint32)[0] == first.size, what
            assert np.array_equal(d_ids0.download((NI,), np.uint32)[:first.size], first), what
            check(d_model.download(model_space.shape, F), model_space, rows, what + ": model-space palettes")
            n = int(d_cnt.download((4,), np.uint32)[0])
            final = d_ids.download((NI,), np.uint32)[:n]
            assert n > 0 and rows[final].all(), what + ": the final list holds an instance that was not solved"
            assert np.array_equal(final, first), what + ": this frame's boxes of the solved instances are last frame's"
            shown = listed_rows(final, None, NI)
            for got, w in ((d_a.download((NI, nv * 12), np.uint8), want[0]), (d_b.download((NI, nv * 12), np.uint8), want[1])):
                assert np.array_equal(got[shown], w[shown]), what + ": vertices differ from the unselected sequence"
                assert (got[~shown] == PATTERN).all(), what + ": an instance outside the final list was deformed"
            seen.append(sorted(final.tolist()))
        assert len({tuple(s) for s in seen}) == len(views), seen    # every view listed other instances
        graph.close()
        for b in (d_pose, d_model, d_place, d_pal, d_last, d_bnd, d_ids0, d_cnt0, d_ids, d_cnt, d_view, d_a, d_b, d_w):
            b.free()

"""The cross-fade calls for a listed subset of a crowd: mmdx_motion_set_blend_bones_time_select, _blend_morphs_time_select and
mmdx_skeleton_solve_motion_set_blend_time_select (include/mmdx.h, rules 1-10).

The expected value everywhere is the EXISTING plain call on clean operands -- tests/test_motion_blend.py holds it to the libmmd
fixture -- compared as bit patterns, no tolerance: listed rows carry the plain call's bytes, every other byte of the output keeps
the pattern it held before the call (0xA5), and the operand rows of unlisted instances hold clip ids out of range, NaN times and
NaN weights.  Shapes: the 67 x 41 x 7 crowd of test_motion_blend.py and a list of capacity 150 whose counts straddle the first
workgroup boundary of either track kernel; 9 instances for the palette call on three rigs.
CPU tests: the symbols, and every argument error before the device is touched."""
import ctypes as C
import os

import numpy as np
import pytest

from simple_mmd_renderer_amd import _capi as api
from simple_mmd_renderer_amd import synth, vmd
from simple_mmd_renderer_amd.engine import DeformModel, DeviceBuffer, device_count, planes_from_matrix
from tests import golden_util as gu
from tests import motion_blend_ref as mb
from tests import palette_place_ref as pp
from tests.test_capi_symbols import declared_symbols
from tests.test_cull_bounds import F, SENT, View, look_at, mat_mul, perspective
from tests.test_motion_blend import NB, NCLIPS, NI, NM, NONE, _close, _crowd, _crowd_set, _device_operands, _ptrs, _run_blend, _solve_cases
from tests.test_solve_select import RIGS, listed_rows

SELECT_ENTRY_POINTS = ("mmdx_motion_set_blend_bones_time_select", "mmdx_motion_set_blend_morphs_time_select",
                       "mmdx_skeleton_solve_motion_set_blend_time_select")
PATTERN = 0xA5
THREADS = 256                                        # threads per workgroup of both track kernels (kRigThreads, kThreads)
CAPACITY = 150
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(autouse=True)
def _lib(hip_lib):
    return hip_lib


def check(got, want, rows, what):
    """Listed rows: the plain call's bits.  Everything else: the pattern, byte for byte."""
    gu.assert_bits_equal(got[rows], want[rows], what + ": listed rows differ from the plain call")
    assert (got[~rows].view(np.uint8) == PATTERN).all(), what + ": a row that is not listed was written"


def poisoned(ops, rows):
    """The five operand arrays (clips a, times a, clips b, times b, weights) with the rows of unlisted instances made unusable."""
    ca, ta, cb, tb, w = [np.array(a) for a in ops]
    ca[~rows], cb[~rows] = NCLIPS + 5, NCLIPS + 9
    ta[~rows], tb[~rows], w[~rows] = np.nan, np.nan, np.nan
    return ca, ta, cb, tb, w


# ---------------------------------------------------------------------------------------- CPU ----
def test_select_entry_points_are_declared_exported_and_bound(hip_lib):
    syms = declared_symbols()
    for name in SELECT_ENTRY_POINTS:
        assert name in syms and hasattr(hip_lib, name) and name in api.SIGNATURES, name
    assert [len(api.SIGNATURES[n][1]) for n in SELECT_ENTRY_POINTS] == [5, 5, 6]
    hdr = open(os.path.join(ROOT, "include", "mmdx.h")).read()
    assert "#define MMDX_ABI_VERSION 3u" in hdr and hip_lib.mmdx_abi_version() == 3
    assert "is not selected: it runs for every instance" not in hdr           # rule 10 of mmdx_skeleton_solve_select, reworded
    for name in ("blend_bones_time_select_device", "blend_morphs_time_select_device"):
        assert callable(getattr(vmd.MotionSet, name))
    assert callable(vmd.Skeleton.solve_motion_set_blend_time_select_device) and callable(vmd.Skeleton.solve_motion_set_blend_time_select)
    poser = open(os.path.join(ROOT, "simple_mmd_renderer_amd", "host", "mmdx_poser.hpp")).read()
    for name in SELECT_ENTRY_POINTS:
        assert name + "(" in poser, name


def test_argument_errors_precede_any_device_call():
    """Every refusal of rules 5 and 6 is MMDX_ERR_INVALID_ARGUMENT -- on a machine without a GPU too, where the first call that
    reaches the device would say MMDX_ERR_NO_DEVICE instead.  Operand and output pointers are never followed."""
    lib = api.lib()
    names = ["センター", "首"]
    v = vmd.Vmd(vmd.write_vmd(synth.make_bone_keys(names, 1, keys_per=3), [("あ", 0, 0.5), ("あ", 9, 1.0)]))
    bm, mm = v.bind_bones(names), v.bind_morphs(["あ"])
    both = vmd.MotionSet([bm, bm], [mm, mm])
    bones_only, morphs_only = vmd.MotionSet([bm, bm]), vmd.MotionSet(morph_motions=[mm, mm])
    sk, sk3 = vmd.Skeleton(*synth.make_skeleton(2, 1)), vmd.Skeleton(*synth.make_skeleton(3, 1))
    dev = vmd.TIMES_ON_DEVICE | api.OUT_ON_DEVICE
    err = lambda: lib.mmdx_last_error_string().decode()          # noqa: E731
    out = 0x9000                                                  # "device" addresses: validation must not look behind them

    def args(n=2, flags=dev, struct_size=None, **replace):
        ptrs = dict(clips_a=0x1000, clips_b=0x2000, times_a=0x3000, times_b=0x4000, weights=0x5000)
        ptrs.update(replace)
        return vmd.MotionBlendArgs(C.sizeof(vmd.MotionBlendArgs) if struct_size is None else struct_size, n,
                                   *[ptrs[k] for k in ("clips_a", "clips_b", "times_a", "times_b", "weights")], flags)

    def sel(flags=api.SELECT_ON_DEVICE, size=C.sizeof(api.InstanceSelect), ids_ptr=0x6000, count=None, n_ids=2, reserved0=0):
        s = api.InstanceSelect()
        s.struct_size, s.flags, s.ids, s.count, s.n_ids, s.reserved0 = size, flags, ids_ptr, count, n_ids, reserved0
        return s

    calls = {   # name -> (call(set, args*, select*, out), the set that lacks the side)
        "bones": (lambda st, a, s, o: lib.mmdx_motion_set_blend_bones_time_select(st, None, a, s, o), morphs_only),
        "morphs": (lambda st, a, s, o: lib.mmdx_motion_set_blend_morphs_time_select(st, None, a, s, o), bones_only),
        "solve": (lambda st, a, s, o: lib.mmdx_skeleton_solve_motion_set_blend_time_select(sk.h, st, None, a, s, o), morphs_only),
    }
    bad = np.array([1, 2, 0], np.uint32)
    ids = np.array([0, 1], np.uint32)
    n_dev = C.c_int32()
    no_gpu = lib.mmdx_device_count(C.byref(n_dev)) != 0 or n_dev.value < 1
    for what, (call, lacking) in calls.items():
        assert call(None, C.byref(args()), C.byref(sel()), out) == 1, what                          # NULL set
        assert call(both.h, None, C.byref(sel()), out) == 1, what                                   # NULL args
        assert call(both.h, C.byref(args()), C.byref(sel()), None) == 1, what                       # NULL output
        for k in ("clips_a", "clips_b", "times_a", "times_b", "weights"):
            assert call(both.h, C.byref(args(**{k: None})), C.byref(sel()), out) == 1 and "NULL" in err(), (what, k)
        assert call(both.h, C.byref(args(n=0)), C.byref(sel()), out) == 1 and "n_instances" in err(), what
        for size in (0, C.sizeof(vmd.MotionBlendArgs) - 8, C.sizeof(vmd.MotionBlendArgs) + 8):
            assert call(both.h, C.byref(args(struct_size=size)), C.byref(sel()), out) == 1 and "struct_size" in err(), (what, size)
        for bit in (1 << 1, 1 << 3, 1 << 4, 1 << 10, 1 << 31):                                      # bits of other calls, unknown bits
            assert call(both.h, C.byref(args(flags=dev | bit)), C.byref(sel()), out) == 1 and "unknown flag" in err(), (what, bit)
        for fl in (0, vmd.TIMES_ON_DEVICE, api.OUT_ON_DEVICE):                                      # host operands or a host output
            assert call(both.h, C.byref(args(flags=fl)), C.byref(sel()), out) == 1 and "device operands only" in err(), (what, fl)
        assert call(lacking.h, C.byref(args()), C.byref(sel()), out) == 1 and "created without" in err(), what
        assert call(both.h, C.byref(args()), None, out) == 1 and "select is NULL" in err(), what
        assert call(both.h, C.byref(args()), C.byref(sel(size=C.sizeof(api.InstanceSelect) - 4)), out) == 1 and "struct_size" in err(), what
        assert call(both.h, C.byref(args()), C.byref(sel(flags=api.SELECT_ON_DEVICE | 2)), out) == 1
        assert "mmdx_instance_select.flags" in err(), what
        assert call(both.h, C.byref(args()), C.byref(sel(reserved0=1)), out) == 1 and "reserved0" in err(), what
        assert call(both.h, C.byref(args()), C.byref(sel(ids_ptr=None)), out) == 1 and "ids is NULL" in err(), what
        assert call(both.h, C.byref(args()), C.byref(sel(ids_ptr=0x6002)), out) == 1 and "aligned" in err(), what
        # a host list is read on the host: an id that is no row fails there, inside the count only
        assert call(both.h, C.byref(args()), C.byref(sel(flags=0, ids_ptr=bad.ctypes.data, n_ids=3)), out) == 1
        assert "ids[1] = 2" in err(), what
        two = np.array([2], np.uint32)
        assert call(both.h, C.byref(args()), C.byref(sel(flags=0, ids_ptr=bad.ctypes.data, count=two.ctypes.data, n_ids=3)), out) == 1
        assert "ids[1] = 2" in err(), what
        if no_gpu:                                    # valid arguments must say that there is no device, not compute
            one = np.array([1], np.uint32)            # (an id behind the count is not looked at)
            assert call(both.h, C.byref(args()), C.byref(sel(flags=0, ids_ptr=bad.ctypes.data, count=one.ctypes.data, n_ids=3)), out) == 3
            assert "no HIP device" in err(), what
            assert call(both.h, C.byref(args()), C.byref(sel(flags=0, ids_ptr=ids.ctypes.data, n_ids=2)), out) == 3, what
            assert call(both.h, C.byref(args()), C.byref(sel()), out) == 3 and "no HIP device" in err(), what
    fn = lib.mmdx_skeleton_solve_motion_set_blend_time_select
    assert fn(None, both.h, None, C.byref(args()), C.byref(sel()), out) == 1                        # NULL skeleton
    assert fn(sk3.h, both.h, None, C.byref(args()), C.byref(sel()), out) == 1 and "3" in err()      # another bone count
    for x in (both, bones_only, morphs_only, sk, sk3, bm, mm, v):
        x.close()


# ---------------------------------------------------------------------------------------- GPU ----
_cache = {}


def track_case():
    """The crowd of test_motion_blend.py with weights of every class, the list, and the PLAIN calls' poses and rates on the clean
    operands: computed once, shared, never written."""
    if "tracks" in _cache:
        return _cache["tracks"]
    z = _crowd()
    rng = np.random.RandomState(47)
    w = np.r_[mb.WEIGHTS, mb.WEIGHTS, np.float32(np.nan), rng.uniform(0, 1, NI - 2 * mb.WEIGHTS.size - 1).astype(np.float32)].astype(np.float32)
    w = w[rng.permutation(NI)]
    ops = (z["ca"], z["ta"], z["cb"], z["tb"], w)
    ms = _crowd_set(z)
    poses, rates = _run_blend(ms, *ops)
    _close(ms)
    # 150 entries drawn from 50 of the 67 instances (17 are never listed): duplicates, not ascending, three entries that are no row
    pool = rng.permutation(NI)[:50]
    ids = pool[rng.randint(0, pool.size, CAPACITY)].astype(np.uint32)
    ids[[3, 20, 100]] = [NI, 1000, 0xFFFFFFFF]
    # the NaN weight and one plain A, B and mix row lead the list, so every count from 5 up lists every weight class
    side, nan = mb.side_of(w), np.isnan(w)
    ids[[0, 1, 2, 4]] = [np.flatnonzero(nan)[0]] + [np.flatnonzero((side == s) & ~nan)[0] for s in (0, 1, 2)]
    for a in (w, poses, rates, ids):
        a.setflags(write=False)
    _cache["tracks"] = dict(z=z, ops=ops, w=w, poses=poses, rates=rates, ids=ids)
    return _cache["tracks"]


def boundary_counts():
    """List positions per workgroup: 256 // 41 = 6 whole positions for the bones, 256 // 7 = 36 for the morphs; the counts on either
    side of both, the ends, and None = no count word."""
    per_bone, per_morph = THREADS // NB, THREADS // NM
    return [0, 1, per_bone, per_bone + 1, per_morph, per_morph + 1, CAPACITY, None]


def run_tracks(ms, ops, ids, count, n_ids=None, host_list=False, model=None):
    """Both track select calls into pattern-filled outputs -> the WHOLE pose array [NI, NB, 8] and rate array [NI, NM]."""
    ds = _device_operands(*ops)
    d_pose, d_w = DeviceBuffer(NI * NB * 32), DeviceBuffer(NI * NM * 4)
    d_pose.memset(PATTERN); d_w.memset(PATTERN)
    n_ids = ids.size if n_ids is None else n_ids
    cnt = None if count is None else np.array([count], np.uint32)
    bufs = [d_pose, d_w]
    if host_list:
        lst = dict(ids_ptr=ids.ctypes.data, n_ids=n_ids, count_ptr=cnt.ctypes.data if cnt is not None else None, select_on_device=False)
    else:
        bufs.append(DeviceBuffer.from_numpy(ids))
        lst = dict(ids_ptr=bufs[-1].ptr, n_ids=n_ids, count_ptr=None)
        if cnt is not None:
            bufs.append(DeviceBuffer.from_numpy(cnt))
            lst["count_ptr"] = bufs[-1].ptr
    ms.blend_bones_time_select_device(NI, *_ptrs(ds), d_pose.ptr, model=model, **lst)
    ms.blend_morphs_time_select_device(NI, *_ptrs(ds), d_w.ptr, model=model, **lst)
    if not host_list:                                            # (a host-list call has completed when it returns)
        api.check(api.lib().mmdx_sync(model.h) if model is not None else api.lib().mmdx_device_synchronize())
    poses, rates = d_pose.download((NI, NB, 8), np.float32), d_w.download((NI, NM), np.float32)
    _close(ds, bufs)
    return poses, rates


@pytest.mark.gpu
def test_gpu_track_calls_listed_rows_and_untouched_rows():
    """Counts 0, 1, 6, 7, 36, 37, 150 and no count word of the capacity-150 list: listed rows are the plain call's, bit for bit;
    every other byte of both outputs is still 0xA5; the operand rows of unlisted instances are poison."""
    assert device_count() >= 1, "no HIP device visible: the GPU tests must run on the MI355X box"
    c = track_case()
    counts = boundary_counts()
    assert counts == [0, 1, 6, 7, 36, 37, 150, None]             # (derived from NB = 41 and NM = 7 above)
    assert THREADS % NB and THREADS % NM                         # a workgroup ends inside a list position: lanes of one wave differ
    ms = _crowd_set(c["z"])
    side = mb.side_of(c["w"])
    for count in counts:
        rows = listed_rows(c["ids"], count, NI)
        what = f"count {count}"
        if count is None or count >= THREADS // NM:              # the comparison cannot go vacuous
            assert all((side[rows] == s).any() for s in (0, 1, 2)) and np.isnan(c["w"][rows]).any(), what
            assert (~rows).sum() >= 10, what
        poses, rates = run_tracks(ms, poisoned(c["ops"], rows), c["ids"], count)
        check(poses, c["poses"], rows, what + ": poses")
        check(rates, c["rates"], rows, what + ": rates")
    assert listed_rows(c["ids"], 0, NI).sum() == 0 and listed_rows(c["ids"], None, NI).sum() <= 50
    # the three entries that are no row lie inside the larger counts, and ids occur more than once
    assert (c["ids"][:37] >= NI).sum() == 2 and (c["ids"] >= NI).sum() == 3 and np.unique(c["ids"]).size < CAPACITY - 50
    _close(ms)


@pytest.mark.gpu
def test_gpu_track_calls_host_list_equals_device_list():
    """The list and its count in host memory: the device list's bytes, readable as soon as the call returns; a capacity above the
    count whose tail holds ids that are no rows; an empty list."""
    c = track_case()
    ms = _crowd_set(c["z"])
    ids = np.ascontiguousarray(c["ids"][30:67])                  # 37 entries, none of the three bad ones
    assert (ids < NI).all()
    rows = listed_rows(ids, None, NI)
    ops = poisoned(c["ops"], rows)
    dev = run_tracks(ms, ops, ids, ids.size)
    check(dev[0], c["poses"], rows, "device list: poses")
    check(dev[1], c["rates"], rows, "device list: rates")
    padded = np.r_[ids, np.full(9, 1000, np.uint32)].astype(np.uint32)
    for what, got in (("count word", run_tracks(ms, ops, ids, ids.size, host_list=True)),
                      ("no count word", run_tracks(ms, ops, ids, None, host_list=True)),
                      ("capacity above the count", run_tracks(ms, ops, padded, ids.size, host_list=True))):
        gu.assert_bits_equal(got[0], dev[0], "host list, " + what + ": poses")
        gu.assert_bits_equal(got[1], dev[1], "host list, " + what + ": rates")
    for got in run_tracks(ms, ops, ids, 0, host_list=True):
        assert (got.view(np.uint8) == PATTERN).all()
    with pytest.raises(api.MmdxError) as e:                      # inside the count, a host id that is no row is refused
        run_tracks(ms, ops, padded, padded.size, host_list=True)
    assert e.value.status == 1
    _close(ms)


def palette_case(rig):
    """(skeleton, solver, motion set, clean operands of 9 instances, the plain one-call palettes)"""
    sk, solver = _solve_cases(rig)
    nb, ni = sk.nb, 9
    names = [f"b{i}" for i in range(nb)]
    vs = [vmd.Vmd(vmd.write_vmd(synth.make_bone_keys(names[k::1 + k], 80 + k, keys_per=3 + k, span=90), [])) for k in range(3)]
    bms = [v.bind_bones(names) for v in vs]
    ms = vmd.MotionSet(bms)
    _close(bms, vs)
    ca, cb = np.array([0, 1, 2, NONE, 1, 2, 0, 1, 2], np.uint32), np.array([1, 2, 0, 2, 9, NONE, 2, 0, 1], np.uint32)
    ta, tb = np.linspace(0.1, 2.9, ni), np.linspace(2.5, 0.2, ni)
    w = np.array([0.0, 0.3, 0.4, 0.5, 1e-7, np.nan, 0.75, 1 - 5e-8, 0.25], np.float32)
    ops = (ca, ta, cb, tb, w)
    ds = _device_operands(*ops)
    d_pal = DeviceBuffer(ni * nb * 64)
    d_pal.memset(0xFF)
    sk.solve_motion_set_blend_time_device(ms, ni, *_ptrs(ds), d_pal.ptr)
    want = d_pal.download((ni, nb, 16), np.float32)
    _close(ds, d_pal)
    return sk, solver, ms, ops, want


@pytest.mark.gpu
@pytest.mark.parametrize("rig", ["fk41", "fk1030", "ik"])
def test_gpu_palette_call_listed_rows_and_untouched_rows(rig):
    """NI = 9, list [7, 2, 2, 5, 11], counts 0, 3 and 5 on a parallel-FK rig of 41 bones, one of 1 030 (two bones per thread in the
    one-launch kernel) and the IK / append rig of rig_ik_expect.npz (blend select into the set's scratch, then solve select):
    listed palette rows equal the plain one-call result, the others keep the pattern, and the skeleton reports the solver."""
    sk, solver, ms, ops, want = palette_case(rig)
    assert sk.info["solver"] == solver
    ni, nb = 9, sk.nb
    ids = np.array([7, 2, 2, 5, 11], np.uint32)
    side = mb.side_of(ops[4])
    assert [int(side[i]) for i in (2, 5, 7)] == [2, 0, 1] and np.isnan(ops[4][5])        # a mix row, an A row (NaN) and a B row
    for count in (0, 3, 5):
        rows = listed_rows(ids, count, ni)
        assert np.flatnonzero(rows).tolist() == {0: [], 3: [2, 7], 5: [2, 5, 7]}[count]
        ds = _device_operands(*poisoned(ops, rows))
        d_pal, d_ids, d_cnt = DeviceBuffer(ni * nb * 64), DeviceBuffer.from_numpy(ids), DeviceBuffer.from_numpy(np.array([count], np.uint32))
        d_pal.memset(PATTERN)
        sk.solve_motion_set_blend_time_select_device(ms, ni, *_ptrs(ds), d_pal.ptr, d_ids.ptr, ids.size, d_cnt.ptr)
        api.check(api.lib().mmdx_device_synchronize())
        check(d_pal.download((ni, nb, 16), np.float32), want, rows, f"{rig}: count {count}")
        shape = sk.last_solve_shape()
        assert shape["solver"] == ("ordered" if solver == vmd.SOLVER_SERIAL else "parallel_fk"), shape
        if solver == vmd.SOLVER_SERIAL:
            assert shape["select"] == 1, shape
        _close(ds, d_pal, d_ids, d_cnt)
    # the convenience call (uploads, calls, downloads the whole array) and a host list
    rows = listed_rows(ids, None, ni)
    pat = np.full((ni, nb, 16), PATTERN * 0x01010101, np.uint32).view(np.float32)
    check(sk.solve_motion_set_blend_time_select(ms, *poisoned(ops, rows), ids, out=pat), want, rows, f"{rig}: convenience call")
    host_ids = np.array([7, 2, 2, 5], np.uint32)
    ds = _device_operands(*poisoned(ops, rows))
    d_pal = DeviceBuffer(ni * nb * 64)
    d_pal.memset(PATTERN)
    sk.solve_motion_set_blend_time_select_device(ms, ni, *_ptrs(ds), d_pal.ptr, host_ids.ctypes.data, 4, None, select_on_device=False)
    check(d_pal.download((ni, nb, 16), np.float32), want, rows, f"{rig}: host list")
    _close(ds, d_pal, ms, sk)


@pytest.mark.gpu
def test_gpu_recorded_first_frame_reads_list_count_dt_and_requests_at_replay():
    """{advance with dt on the device, palette select, morph-rate select, mmdx_deform_batched_select} recorded once after one eager
    run, on the 2 048-vertex mini model, NI = 4.  Replayed; ids, *count, dt and one clip request rewritten in place; replayed
    again.  The listed instances' vertices equal the direct plain calls' on a second animator, the others keep the pattern.  A
    host list is refused while recording."""
    from tests.test_motion_set import _crowd_clips
    m = synth.make_model(2048, 64, 8, 200, 112)                                   # the size of g12_mini_model
    names, mnames, data = _crowd_clips(m, (91, 92, 93, 94))
    ni, cap = 4, 6
    sk = vmd.Skeleton(m.bone_pos, np.asarray(m.bone_parent, np.int32))
    vs = [vmd.Vmd(d) for d in data]
    bms, mms = [v.bind_bones(names) for v in vs], [v.bind_morphs(mnames) for v in vs]
    ms = vmd.MotionSet(bms, mms)
    _close(bms, mms, vs)
    flags = api.PALETTE_ON_DEVICE | api.WEIGHTS_ON_DEVICE | api.OUT_ON_DEVICE
    start = dict(clips_a=np.array([0, 1, 2, 3], np.uint32), times_a=np.array([0.5, 1.25, 2.0, 3.1]),
                 clips_b=np.array([1, NONE, 0, 2], np.uint32), times_b=np.array([1.5, 0.0, 2.2, 0.4]),
                 weights=np.array([0.0, 0.0, 0.25, 0.5], np.float32), fade_rate=np.array([0.0, 0.0, 0.5, 1.0], np.float32))
    steps = [(np.array([3, 1, 3, 9, 0, 0], np.uint32), 3, 1 / 60, None),
             (np.array([2, 0, 1, 3, 3, 2], np.uint32), 2, 0.25, (np.array([0], np.uint32), np.array([3], np.uint32), np.array([0.5], np.float32)))]
    with DeformModel(m) as dm:
        eager, replayed = vmd.Animator(ms, ni), vmd.Animator(ms, ni)
        d_dt = DeviceBuffer.from_numpy(np.array([0.0], np.float64))
        d_ids, d_cnt = DeviceBuffer(cap * 4), DeviceBuffer(4)
        d_pal, d_w = DeviceBuffer(ni * m.nb * 64), DeviceBuffer(ni * m.nm * 4)
        sa, sb = dm.out_sizes(api.OUT_SOA, ni)
        d_a, d_b = DeviceBuffer(sa), DeviceBuffer(sb)

        def frame(an):
            an.advance_device_dt(d_dt.ptr, dm)
            sk.solve_motion_set_blend_time_select_device(ms, ni, *an.operand_ptrs(), d_pal.ptr, d_ids.ptr, cap, d_cnt.ptr, dm)
            ms.blend_morphs_time_select_device(ni, *an.operand_ptrs(), d_w.ptr, d_ids.ptr, cap, d_cnt.ptr, dm)
            dm.deform_batched_raw(ni, d_w.ptr, d_pal.ptr, d_a.ptr, d_b.ptr, api.OUT_SOA, flags, select_ptr=d_ids.ptr,
                                  select_count_ptr=d_cnt.ptr, n_select=cap)

        def direct(an):
            an.advance_device_dt(d_dt.ptr, dm)
            sk.solve_motion_set_blend_time_device(ms, ni, *an.operand_ptrs(), d_pal.ptr, dm)
            ms.blend_morphs_time_device(ni, *an.operand_ptrs(), d_w.ptr, dm)
            dm.deform_batched_raw(ni, d_w.ptr, d_pal.ptr, d_a.ptr, d_b.ptr, api.OUT_SOA, flags)
            dm.sync()
            return d_a.download((ni, m.nv * 12), np.uint8), d_b.download((ni, m.nv * 12), np.uint8)

        def stage(ids, n, dt):
            d_ids.upload(ids)
            d_cnt.upload(np.array([n], np.uint32))
            d_dt.upload(np.array([dt], np.float64))
            for d in (d_pal, d_w, d_a, d_b):
                d.memset(PATTERN)

        eager.set_state(dm, **start)
        stage(steps[0][0], steps[0][1], 0.0)
        frame(replayed)                                           # the run before recording, as the header requires
        dm.sync()
        replayed.set_state(dm, **start)
        dm.graph_begin()
        frame(replayed)
        with pytest.raises(api.MmdxError, match="MMDX_SELECT_ON_DEVICE") as e:
            ms.blend_morphs_time_select_device(ni, *replayed.operand_ptrs(), d_w.ptr, steps[0][0].ctypes.data, cap, None, dm,
                                               select_on_device=False)
        assert e.value.status == 1
        g = dm.graph_end()
        seen = []
        for k, (ids, n, dt, request) in enumerate(steps):
            what = f"replay {k}"
            if request is not None:
                eager.request(*request, model=dm)
                replayed.request(*request, model=dm)
            stage(ids, n, dt)
            want = direct(eager)
            stage(ids, n, dt)
            g.launch()
            dm.sync()
            rows = listed_rows(ids, n, ni)
            assert 0 < rows.sum() < ni, what
            for got, w in ((d_a.download((ni, m.nv * 12), np.uint8), want[0]), (d_b.download((ni, m.nv * 12), np.uint8), want[1])):
                assert np.array_equal(got[rows], w[rows]), what + ": vertices differ from the direct plain calls"
                assert (got[~rows] == PATTERN).all(), what + ": an instance outside the list was deformed"
            pal = d_pal.download((ni, m.nb, 16), np.float32)
            assert (pal[~rows].view(np.uint8) == PATTERN).all() and not (pal[rows].view(np.uint8) == PATTERN).all(), what
            seen.append((tuple(np.flatnonzero(rows)), want[0][rows].tobytes()))
        assert seen[0][0] != seen[1][0] and seen[0][1] != seen[1][1]               # other instances, other vertices
        st_e, st_r = eager.get_state(dm), replayed.get_state(dm)
        for key in ("clips_a", "clips_b", "times_a", "times_b", "weights"):         # the clocks ran for everyone, listed or not
            gu.assert_bits_equal(st_r[key], st_e[key], "animator state: " + key)
        g.close()
        _close(eager, replayed, d_dt, d_ids, d_cnt, d_pal, d_w, d_a, d_b)
    _close(ms, sk)


@pytest.mark.gpu
def test_gpu_recorded_whole_loop_with_selected_tracks():
    """The loop for IK rigs, small, as one graph: mmdx_animator_advance (dt on the device) -> mmdx_cull_bounds on last frame's boxes
    -> the two track select calls with list 0 -> mmdx_skeleton_solve_select -> mmdx_palette_place -> mmdx_palette_bounds ->
    mmdx_cull_bounds -> mmdx_deform_batched_select, replayed with the view and dt rewritten.  (The first cull stands in front of
    the tracks: its list is what they take.)  Last frame's boxes are those of the unselected sequence at the same clocks, so what
    the second cull lists was evaluated and solved; an instance that was not keeps the model-space palette it had (here the
    pattern, which places its box at the origin, outside every view).  For the instances of the final list the vertices equal the
    unselected sequence's."""
    ni, nb, nv, spacing = 70, 44, 600, 12.0
    rig = RIGS["ik44"]()
    m = synth.make_model(nv, nb, 8, 64, seed=7500)
    names, mnames = [f"b{i}" for i in range(nb)], [f"m{i}" for i in range(m.nm)]
    rng = np.random.RandomState(77)
    data = []
    for k in range(3):
        mk = [(n, int(f), float(np.float32(rng.uniform(0, 1)))) for n in mnames[k::2] for f in (0, 40 + k, 110)]
        data.append(vmd.write_vmd(synth.make_bone_keys(names[k::1 + k], 60 + k, keys_per=4 + k, span=120), mk))
    vs = [vmd.Vmd(d) for d in data]
    bms, mms = [v.bind_bones(names) for v in vs], [v.bind_morphs(mnames) for v in vs]
    ms = vmd.MotionSet(bms, mms)
    _close(bms, mms, vs)
    sk = vmd.Skeleton(*rig)
    start = dict(clips_a=rng.randint(0, 3, ni).astype(np.uint32), times_a=rng.uniform(0, 3.5, ni),
                 clips_b=rng.randint(0, 3, ni).astype(np.uint32), times_b=rng.uniform(0, 3.5, ni),
                 weights=rng.choice([0.0, 0.3, 0.6], ni).astype(np.float32))
    place = np.zeros((ni, 8), F)
    place[:, 0] = (np.arange(ni) - ni / 2) * spacing
    yaw = 0.05 + 0.03 * np.arange(ni)
    place[:, 5], place[:, 7] = np.sin(yaw / 2), np.cos(yaw / 2)

    def camera(x, fov):
        eye = (x, 10.0, 80.0)
        cam = mat_mul(perspective(fov, 1.0, 0.1, 1000.0), look_at(eye, (x, 10.0, 0.0)))
        return View(planes_from_matrix(cam, True), 6, 1, eye, 0.0, (0.0, 0.0, 0.0))

    views = [camera(-150.0, 50.0), camera(200.0, 35.0), camera(-300.0, 40.0)]
    dts = [1 / 60, 0.2, 1 / 30]
    dev = api.PALETTE_ON_DEVICE | api.OUT_ON_DEVICE
    dflags = dev | api.WEIGHTS_ON_DEVICE
    pal_shape = (ni, nb, 16)
    with DeformModel(m) as dm:
        eager, replayed = vmd.Animator(ms, ni), vmd.Animator(ms, ni)
        na, nbytes_b = dm.out_sizes(api.OUT_SOA, ni)
        d_pose, d_model = DeviceBuffer(ni * nb * 32), DeviceBuffer(ni * nb * 64)
        d_place, d_pal = DeviceBuffer.from_numpy(place), DeviceBuffer(ni * nb * 64)
        d_last, d_bnd = DeviceBuffer(ni * 24), DeviceBuffer(ni * 24)
        d_ids0, d_cnt0, d_ids, d_cnt = DeviceBuffer(ni * 4), DeviceBuffer(16), DeviceBuffer(ni * 4), DeviceBuffer(16)
        d_view = DeviceBuffer.from_numpy(np.frombuffer(bytes(views[0].struct()), np.uint8))
        d_a, d_b, d_w = DeviceBuffer(na), DeviceBuffer(nbytes_b), DeviceBuffer(ni * m.nm * 4)
        d_dt = DeviceBuffer.from_numpy(np.array([0.0], np.float64))

        def unselected(an):
            """advance, plain tracks, plain solve, place, palette bounds (= "last frame's boxes"), plain deform"""
            an.advance_device_dt(d_dt.ptr, dm)
            ms.blend_bones_time_device(ni, *an.operand_ptrs(), d_pose.ptr, dm)
            ms.blend_morphs_time_device(ni, *an.operand_ptrs(), d_w.ptr, dm)
            sk.solve_device(ni, d_pose.ptr, d_model.ptr, dm)
            dm.place_palettes(ni, d_model.ptr, d_place.ptr, d_pal.ptr, dev | api.PLACE_ON_DEVICE)
            dm.palette_bounds_raw(ni, d_pal.ptr, d_last.ptr, dev, 1.0, 1.0)
            dm.deform_batched_raw(ni, d_w.ptr, d_pal.ptr, d_a.ptr, d_b.ptr, api.OUT_SOA, dflags)
            dm.sync()
            return (d_model.download(pal_shape, F), d_last.download((ni, 6), F), d_a.download((ni, nv * 12), np.uint8),
                    d_b.download((ni, nv * 12), np.uint8))

        def frame(an):
            an.advance_device_dt(d_dt.ptr, dm)
            dm.cull_bounds(d_last, d_view, ni, d_ids0, d_cnt0)
            ms.blend_bones_time_select_device(ni, *an.operand_ptrs(), d_pose.ptr, d_ids0.ptr, ni, d_cnt0.ptr, dm)
            ms.blend_morphs_time_select_device(ni, *an.operand_ptrs(), d_w.ptr, d_ids0.ptr, ni, d_cnt0.ptr, dm)
            sk.solve_select_device(ni, d_pose.ptr, d_model.ptr, d_ids0.ptr, ni, d_cnt0.ptr, dm)
            dm.place_palettes(ni, d_model.ptr, d_place.ptr, d_pal.ptr, dev | api.PLACE_ON_DEVICE)
            dm.palette_bounds_raw(ni, d_pal.ptr, d_bnd.ptr, dev, 1.0, 1.0)
            dm.cull_bounds(d_bnd, d_view, ni, d_ids, d_cnt)
            dm.deform_batched_raw(ni, d_w.ptr, d_pal.ptr, d_a.ptr, d_b.ptr, api.OUT_SOA, dflags, select_ptr=d_ids.ptr,
                                  select_count_ptr=d_cnt.ptr, n_select=ni)

        eager.set_state(dm, **start)
        unselected(replayed)                                      # (sizes the plain scratch; the boxes for the run below)
        frame(replayed)                                           # once un-recorded: sizes every scratch
        dm.sync()
        replayed.set_state(dm, **start)
        dm.graph_begin()
        frame(replayed)
        graph = dm.graph_end()
        seen = []
        for k, (view, dt) in enumerate(zip(views, dts)):
            what = "replay %d" % k
            d_dt.upload(np.array([dt], np.float64))
            model_space, boxes, want_a, want_b = unselected(eager)        # leaves this frame's boxes in d_last
            first = view.ref(boxes, True)[0][0]
            assert 0 < first.size < ni, what
            rows = listed_rows(first, None, ni)
            d_view.upload(np.frombuffer(bytes(view.struct()), np.uint8))
            for buf in (d_pose, d_w, d_model, d_a, d_b):          # a pose or rate row that is not listed is never read
                buf.memset(PATTERN)
            for buf in (d_ids0, d_ids):
                buf.upload(np.full(ni, SENT, np.uint32))
            graph.launch()
            dm.sync()
            assert d_cnt0.download((4,), np.uint32)[0] == first.size, what
            assert np.array_equal(d_ids0.download((ni,), np.uint32)[:first.size], first), what
            got_model = d_model.download(pal_shape, F)
            gu.assert_bits_equal(got_model[rows], model_space[rows], what + ": model-space palettes of the listed instances")
            assert (got_model[~rows].view(np.uint8) == PATTERN).all(), what + ": an unlisted instance was solved"
            assert (d_pose.download((ni, nb, 8), F)[~rows].view(np.uint8) == PATTERN).all(), what + ": an unlisted pose row was written"
            assert (d_w.download((ni, m.nm), F)[~rows].view(np.uint8) == PATTERN).all(), what + ": an unlisted rate row was written"
            n = int(d_cnt.download((4,), np.uint32)[0])
            final = d_ids.download((ni,), np.uint32)[:n]
            assert n > 0 and rows[final].all(), what + ": the final list holds an instance that was not solved"
            assert np.array_equal(final, first), what + ": this frame's boxes of the solved instances are the unselected sequence's"
            shown = listed_rows(final, None, ni)
            for got, w in ((d_a.download((ni, nv * 12), np.uint8), want_a), (d_b.download((ni, nv * 12), np.uint8), want_b)):
                assert np.array_equal(got[shown], w[shown]), what + ": vertices differ from the unselected sequence"
                assert (got[~shown] == PATTERN).all(), what + ": an instance outside the final list was deformed"
            seen.append((tuple(sorted(final.tolist())), want_a[shown].tobytes()))
        assert len({s[0] for s in seen}) == len(views)            # every view listed other instances
        st_e, st_r = eager.get_state(dm), replayed.get_state(dm)
        for key in ("clips_a", "clips_b", "times_a", "times_b", "weights"):         # the clocks ran for everyone
            gu.assert_bits_equal(st_r[key], st_e[key], "animator state: " + key)
        graph.close()
        _close(eager, replayed, d_pose, d_model, d_place, d_pal, d_last, d_bnd, d_ids0, d_cnt0, d_ids, d_cnt, d_view, d_a, d_b, d_w, d_dt)
    _close(ms, sk)

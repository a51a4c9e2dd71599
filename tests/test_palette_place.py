"""Where every crowd instance stands: mmdx_palette_place (include/mmdx.h), out[i][b] = S[i][b] * W[i] with W[i] from a pose
{tx, ty, tz, 0, qx, qy, qz, qw} or, with MMDX_PLACE_MATRIX, from 16 floats.

The operation is libmmd's Matrix4x4<float>::operator* (and Quaternion::ToRotateMatrix for the pose form), so everything is compared
as bit patterns; the one exception is that a NaN only has to be a NaN (its sign and payload are not part of the contract):
  * tests/golden/palette_place_expect.npz comes from the real libmmd (tests/palette_place_driver.cpp, tests/gen_palette_place_golden.py);
  * tests/palette_place_ref.py restates the arithmetic in numpy float32 and reproduces that fixture on the CPU;
  * tests/place_math_driver.cpp runs csrc/place_math.hpp -- the lines the kernel compiles -- on the CPU, also under ASan + UBSan;
  * on the GPU the fixture goes through the call in both forms, shapes around the launch's edges are held to the restatement with
    sentinels around the output, and solve -> place -> deform + bounds -> cull runs end to end, direct and as a replayed graph.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from simple_mmd_renderer_amd import _capi as api
from simple_mmd_renderer_amd import synth, vmd
from simple_mmd_renderer_amd.engine import DeformModel, DeviceBuffer, device_count
from tests import golden_util as gu
from tests import host_program as hp
from tests import motion_time_ref as mt
from tests import palette_place_ref as pp
from tests.test_capi_symbols import declared_symbols

F = np.float32
INVALID, NO_DEVICE = 1, 3
ALL_DEV = api.PALETTE_ON_DEVICE | api.PLACE_ON_DEVICE | api.OUT_ON_DEVICE
GUARD = 256                    # sentinel bytes in front of and behind an output array
NB_FIXTURE = 24                # rig_small's bone count
needs_driver = pytest.mark.skipif(not mt.driver_available(), reason="the reference's libmmd headers are not present")


@pytest.fixture(autouse=True)
def _lib(hip_lib):
    return hip_lib


# ---------------------------------------------------------------------------------------- CPU ----
def test_place_entry_point_is_declared_exported_and_bound(hip_lib):
    assert "mmdx_palette_place" in declared_symbols() and hasattr(hip_lib, "mmdx_palette_place")
    assert "mmdx_palette_place" in api.SIGNATURES
    inc = os.path.join(pp.ROOT, "include")
    hdr = open(os.path.join(inc, "mmdx.h")).read()
    assert "typedef struct mmdx_place_args {" in hdr and "#define MMDX_ABI_VERSION 3u" in hdr and "g_state.model_matrix" in hdr
    assert hip_lib.mmdx_abi_version() == 3
    # the struct size and the flag values as the header gives them to a C compiler
    size, place_dev, place_matrix, pal_dev, out_dev, pose_floats = hp.c_values([
        "sizeof(mmdx_place_args)", "MMDX_PLACE_ON_DEVICE", "MMDX_PLACE_MATRIX", "MMDX_PALETTE_ON_DEVICE", "MMDX_OUT_ON_DEVICE", "MMDX_POSE_FLOATS"])
    assert C.sizeof(api.PlaceArgs) == size == 4 * 4 + 3 * 8
    assert (api.PLACE_ON_DEVICE, api.PLACE_MATRIX, api.PALETTE_ON_DEVICE, api.OUT_ON_DEVICE, api.POSE_FLOATS) == \
        (place_dev, place_matrix, pal_dev, out_dev, pose_floats)
    # the new bits are no other flag's (mmdx_deform_args uses bits 0..7)
    assert place_dev == 1 << 8 and place_matrix == 1 << 9
    assert callable(DeformModel.place_palettes) and callable(DeformModel.place)
    poser = open(os.path.join(pp.ROOT, "simple_mmd_renderer_amd", "host", "mmdx_poser.hpp")).read()
    assert "mmdx_palette_place(" in poser


def test_numpy_restatement_reproduces_the_libmmd_fixture():
    z = pp.fixture()
    assert 280 <= z["form"].size <= 320 and os.path.getsize(pp.FIXTURE) < 64 * 1024
    pp.assert_rows_equal(pp.place_rows(z["form"], z["s"], z["placement"]), z["expect"], "restatement vs libmmd")


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan-ubsan"])
def test_place_math_header_reproduces_the_fixture_on_the_cpu(sanitize):
    """csrc/place_math.hpp, the code the kernel compiles, as a stand-alone host program (-ffp-contract=off; the second build with
    -fsanitize=address,undefined, run directly)."""
    z = pp.fixture()
    got = pp.run_driver(pp.build_math_driver(sanitize), z["form"], z["s"], z["placement"])
    pp.assert_rows_equal(got, z["expect"], "place_math.hpp vs libmmd")


def test_fixture_covers_what_it_claims():
    z = pp.fixture()
    form, s, p, e, kind = z["form"], z["s"], z["placement"], z["expect"], np.array(z["kind"])
    pose, mat = form == pp.POSE, form == pp.MATRIX
    assert pose.sum() >= 100 and mat.sum() >= 100
    finite = np.isfinite(p).all(axis=1) & np.isfinite(s).all(axis=1)
    qw = p[pose & finite, 7]
    assert (qw > 0).sum() >= 30 and (qw < 0).sum() >= 30                                      # both hemispheres
    norm2 = (p[pose & finite, 4:8].astype(np.float64) ** 2).sum(axis=1)
    assert (np.abs(norm2 - 1) > 0.1).sum() >= 10 and (norm2 == 0).any()                       # non-unit quaternions, the zero one
    t = np.abs(p[pose & finite, :3])
    assert t[t > 0].min() <= 1e-3 and t.max() >= 1e4                                          # translations 1e-3 .. 1e4
    assert (p[pose, 3] != 0).sum() >= 30                                                      # the ignored fourth float is set
    # an identity placement changes a zero's sign, in both forms
    ident = np.eye(4, dtype=F).reshape(16)
    is_ident = np.where(pose, (p[:, :8] == pp.IDENTITY_POSE).all(axis=1), (p == ident).all(axis=1))
    neg_in, neg_out = gu.bits(s) == 0x80000000, gu.bits(e) == 0x80000000
    for f in (pose, mat):
        rows = f & is_ident
        assert rows.sum() >= 8 and (neg_in[rows] & ~neg_out[rows] & (e[rows] == 0)).any()
    # matrix form: rigid, scaled and sheared rows are what they say
    lin = p[:, [0, 1, 2, 4, 5, 6, 8, 9, 10]].reshape(-1, 3, 3).astype(np.float64)
    with np.errstate(invalid="ignore"):                       # the planted infinities and NaN of the special rows
        gram = lin @ lin.transpose(0, 2, 1)
        off = np.abs(gram - gram * np.eye(3)).max(axis=(1, 2))
    diag = np.einsum("nii->ni", gram)
    assert (np.abs(diag[kind == "rigid"] - 1) < 1e-5).all() and (off[kind == "rigid"] < 1e-5).all()
    assert (np.abs(diag[kind == "scaled"] - 1) > 0.05).any(axis=1).all() and (off[kind == "scaled"] < 1e-3 * diag[kind == "scaled"].max(axis=1)).all()
    assert (off[kind == "sheared"] > 1e-3).all()
    # every special class, in S and in the placement, in both forms
    tiny = np.finfo(F).tiny
    live = np.ones(16, bool)
    for f, width in ((pose, 8), (mat, 16)):
        live[:] = False
        live[:width] = True
        if width == 8:
            live[3] = False
        for what, hit in (("-0", lambda a: gu.bits(a) == 0x80000000), ("denormal", lambda a: (a != 0) & (np.abs(a) < tiny)),
                          ("inf", np.isinf), ("nan", np.isnan)):
            assert hit(s[f]).any() and hit(p[f][:, live]).any(), (width, what)
    assert ((e != 0) & (np.abs(e) < tiny)).any() and np.isnan(e).any() and np.isinf(e).any()
    assert {"unit", "identity", "nonunit", "rigid", "scaled", "sheared", "negzero", "denormal", "inf", "nan"} == set(kind)
    # the skinning matrices are rig_small's real palettes (rows the generator did not plant anything into)
    real = {r.tobytes() for r in np.load(os.path.join(gu.GOLDEN_DIR, "rig_small_expect.npz"))["expect_palettes"].reshape(-1, 16)}
    assert sum(r.tobytes() in real for r in s) >= 200


@needs_driver
def test_fixture_equals_a_fresh_run_of_libmmd():
    z = pp.fixture()
    got = pp.run_driver(pp.build_libmmd_driver(), z["form"], z["s"], z["placement"])
    pp.assert_rows_equal(got, z["expect"], "fresh libmmd run")


def test_place_refuses_bad_arguments():
    """Everything is decided before the first HIP call, so a host-only handle shows it without a GPU: a valid call gets as far as
    MMDX_ERR_NO_DEVICE, every mistake is MMDX_ERR_INVALID_ARGUMENT first."""
    lib = api.lib()
    err = lambda: lib.mmdx_last_error_string().decode()          # noqa: E731
    ni, nb = 3, 5
    m = synth.make_model(64, nb, 0, 0, seed=11)
    pal = np.zeros((ni, nb, 16), F)
    out = np.zeros((ni, nb, 16), F)
    poses = np.tile(pp.IDENTITY_POSE, (ni, 1))

    def args(n=ni, flags=0, struct_size=None, reserved0=0, palettes=pal.ctypes.data, placements=poses.ctypes.data,
             out_palettes=out.ctypes.data):
        a = api.PlaceArgs()
        a.struct_size = C.sizeof(api.PlaceArgs) if struct_size is None else struct_size
        a.flags, a.n_instances, a.reserved0 = flags, n, reserved0
        a.palettes, a.placements, a.out_palettes = palettes, placements, out_palettes
        return a
    with DeformModel(m, host_only=True) as dm:
        call = lambda a, h=dm.h: lib.mmdx_palette_place(h, C.byref(a) if a is not None else None)          # noqa: E731
        assert call(args(), None) == INVALID and "NULL" in err()                              # NULL model
        assert call(None) == INVALID and "NULL" in err()                                      # NULL args
        for k in ("palettes", "placements", "out_palettes"):
            assert call(args(**{k: None})) == INVALID and "NULL" in err(), k
        for size in (0, C.sizeof(api.PlaceArgs) - 8, C.sizeof(api.PlaceArgs) + 8):
            assert call(args(struct_size=size)) == INVALID and "struct_size" in err(), size
        for bad in (1 << 1, 1 << 3, 1 << 4, 1 << 7, 1 << 10, 1 << 31):
            assert call(args(flags=bad)) == INVALID and "unknown flag" in err(), bad
        assert call(args(reserved0=1)) == INVALID and "reserved0" in err()
        # palettes and out_palettes: the same array is fine, a shifted one is not
        big = np.zeros((ni + 1, nb, 16), F)
        base = big.ctypes.data
        assert call(args(palettes=base, out_palettes=base)) == NO_DEVICE                      # in place: valid
        for shift in (64, nb * 64, (ni * nb - 1) * 64):
            assert call(args(palettes=base, out_palettes=base + shift)) == INVALID and "overlap" in err(), shift
            assert call(args(palettes=base + shift, out_palettes=base)) == INVALID and "overlap" in err(), shift
        # placements inside, or straddling an end of, out_palettes
        for at in (base, base + 64, base + ni * nb * 64 - 4, base - ni * 32 + 4):
            assert call(args(out_palettes=base, placements=at)) == INVALID and "placements overlaps" in err(), at - base
        assert call(args(out_palettes=base, placements=base + ni * nb * 64)) == NO_DEVICE     # directly behind: valid
        assert call(args(out_palettes=base, placements=base + 64, flags=api.PLACE_MATRIX)) == INVALID
        # device operands: alignment
        assert call(args(flags=api.PALETTE_ON_DEVICE, palettes=base + 8)) == INVALID and "16-byte" in err()
        assert call(args(flags=api.OUT_ON_DEVICE, out_palettes=base + 4)) == INVALID and "16-byte" in err()
        assert call(args(flags=api.PLACE_ON_DEVICE, placements=poses.ctypes.data + 2)) == INVALID and "4-byte" in err()
        # nothing to do is not an error, whatever the pointers; a valid call needs a device
        assert call(args(n=0)) == api.OK and call(args(n=0, palettes=None, placements=None, out_palettes=None)) == api.OK
        for flags in (0, api.PLACE_MATRIX, ALL_DEV):
            assert call(args(flags=flags)) == NO_DEVICE, flags
        with pytest.raises(api.MmdxError) as e:
            dm.place(pal, poses)
        assert e.value.status == NO_DEVICE
        with pytest.raises(ValueError):
            dm.place(pal, np.zeros((ni, 7), F))


def test_place_kernels_have_no_spills_and_no_scratch(hip_lib):
    import sys
    out = subprocess.run([sys.executable, os.path.join(pp.ROOT, "tools", "kernel_resources.py"), api.LIB_PATH, "palette_place"],
                         capture_output=True, text=True, check=True).stdout.splitlines()
    assert {l.split()[0] for l in out} == {"palette_place_kernel<true>", "palette_place_kernel<false>"}
    for l in out:
        f = l.split()
        res = dict(zip(f[1::2], (int(v) for v in f[2::2])))
        assert res["spill"] == 0 and res["scratch"] == 0 and res["lds"] == 0 and res["vgpr"] <= 32, l


# ---------------------------------------------------------------------------------------- GPU ----
def _guarded(nbytes, fill=None):
    """A device range of nbytes with GUARD sentinel bytes on both sides -> (buffer, address of the range)."""
    buf = DeviceBuffer(nbytes + 2 * GUARD)
    buf.memset(0xEE)
    if fill is not None:
        buf.upload(fill, GUARD)
    return buf, buf.ptr + GUARD


def _guards_intact(buf, nbytes):
    raw = buf.download((nbytes + 2 * GUARD,), np.uint8)
    return (raw[:GUARD] == 0xEE).all() and (raw[GUARD + nbytes:] == 0xEE).all()


def _place_both_ways(dm, pal, placements, matrix, want, what):
    """The call out of place and in place on device operands, the output between sentinels; then with host operands."""
    ni, nb = pal.shape[:2]
    nbytes = pal.nbytes
    flags = ALL_DEV | (api.PLACE_MATRIX if matrix else 0)
    d_in, d_pl = DeviceBuffer.from_numpy(pal), DeviceBuffer.from_numpy(placements)
    d_out, out_ptr = _guarded(nbytes)
    dm.place_palettes(ni, d_in.ptr, d_pl.ptr, out_ptr, flags)
    dm.sync()
    pp.assert_rows_equal(d_out.download((ni, nb, 16), F, GUARD), want, what + ": out of place")
    assert _guards_intact(d_out, nbytes), what + ": out of place wrote outside its array"
    gu.assert_bits_equal(d_in.download((ni, nb, 16), F), pal, what + ": out of place changed its input")
    d_io, io_ptr = _guarded(nbytes, pal)
    dm.place_palettes(ni, io_ptr, d_pl.ptr, io_ptr, flags)
    dm.sync()
    pp.assert_rows_equal(d_io.download((ni, nb, 16), F, GUARD), want, what + ": in place")
    assert _guards_intact(d_io, nbytes), what + ": in place wrote outside its array"
    gu.assert_bits_equal(d_pl.download(placements.shape, F), placements, what + ": the placements changed")
    pp.assert_rows_equal(dm.place(pal, placements), want, what + ": host operands")
    for d in (d_in, d_pl, d_out, d_io):
        d.free()


@pytest.mark.gpu
@pytest.mark.parametrize("matrix", [False, True], ids=["pose", "matrix"])
def test_gpu_fixture_through_the_call(matrix):
    """The libmmd fixture as a crowd: one instance per row of the form, rig_small's 24 bones per instance, every bone of instance i
    holding row i's skinning matrix, instance i taking placement i -- every bone of instance i must come out as row i's S * W."""
    assert device_count() >= 1, "no HIP device visible: the GPU tests must run on the MI355X box"
    z = pp.fixture()
    rows = z["form"] == (pp.MATRIX if matrix else pp.POSE)
    s, p, e = z["s"][rows], z["placement"][rows], z["expect"][rows]
    ni = int(rows.sum())
    pal = np.ascontiguousarray(np.broadcast_to(s[:, None, :], (ni, NB_FIXTURE, 16)))
    want = np.ascontiguousarray(np.broadcast_to(e[:, None, :], (ni, NB_FIXTURE, 16)))
    placements = np.ascontiguousarray(p if matrix else p[:, :8])
    with DeformModel(synth.make_model(64, NB_FIXTURE, 0, 0, seed=12)) as dm:
        _place_both_ways(dm, pal, placements, matrix, want, "fixture")


def _shape_palettes(ni, nb, rng):
    """Real palettes for the shape: the fk41 / fk1030 rigs of tests/test_motion_blend.py solved from random poses, synth palettes
    for the rest."""
    if nb in (41, 1030):
        from tests.test_motion_blend import _solve_cases
        sk, _ = _solve_cases("fk%d" % nb)
        poses = np.zeros((ni, nb, 8), F)
        poses[..., :3] = rng.uniform(-2, 2, (ni, nb, 3))
        q = rng.normal(size=(ni, nb, 4))
        poses[..., 4:] = q / np.linalg.norm(q, axis=-1, keepdims=True)
        pal = sk.solve(poses)
        sk.close()
        return pal
    return synth.make_palettes(synth.make_model(64, nb, 0, 0, seed=13), np.arange(ni) * 7 + 1).copy()


@pytest.mark.gpu
@pytest.mark.parametrize("ni,nb", [(1, 1), (3, 1), (5, 17), (2, 41), (2, 1030)])
def test_gpu_shapes_equal_the_restatement(ni, nb):
    """4 rows in one partial wave; 68 and 164 rows per instance (no multiple of 64: a partial last wave per instance); 4 120 rows per
    instance (17 workgroups, the last one partial).  Both forms, out of place and in place, 256 sentinel bytes around the output."""
    assert device_count() >= 1, "no HIP device visible: the GPU tests must run on the MI355X box"
    rng = np.random.RandomState(100 * ni + nb)
    pal = _shape_palettes(ni, nb, rng)
    assert pal.shape == (ni, nb, 16) and np.isfinite(pal).all()
    q = rng.normal(size=(ni, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    poses = np.zeros((ni, 8), F)
    poses[:, :3], poses[:, 3], poses[:, 4:] = rng.uniform(-50, 50, (ni, 3)), 9.0, q
    mats = pp.matrix_from_pose(poses) * F(1.5)
    mats[:, 4] += F(0.25)                                          # scaled and sheared
    with DeformModel(synth.make_model(64, nb, 0, 0, seed=14)) as dm:
        for matrix, placements in ((False, poses), (True, mats)):
            want = pp.place_crowd(pal, placements, matrix)
            assert len({want[i].tobytes() for i in range(ni)}) == ni
            _place_both_ways(dm, pal, placements, matrix, want, "%dx%d %s" % (ni, nb, "matrix" if matrix else "pose"))


NI, NV, NB, SPACING = 24, 300, 41, 12.0
DEV = api.PALETTE_ON_DEVICE | api.OUT_ON_DEVICE


def crowd_placements(yaw_of):
    """Pose form: instance i at x = (i - NI/2) * SPACING as in tests/test_cull_loop.py, turned about y by yaw_of(i)."""
    p = np.zeros((NI, 8), F)
    p[:, 0] = (np.arange(NI) - NI / 2) * SPACING
    yaw = np.array([yaw_of(i) for i in range(NI)], np.float64)
    p[:, 5], p[:, 7] = np.sin(yaw / 2), np.cos(yaw / 2)
    return p


class _Loop:
    """The fk41 rig, a motion set of two clips on it, a 41-bone model of 300 vertices and the device arrays of the loop
    solve -> place -> deform + bounds."""

    def __init__(self):
        from tests.test_motion_blend import _solve_cases
        self.sk, _ = _solve_cases("fk41")
        names = [f"b{i}" for i in range(NB)]
        vs = [vmd.Vmd(vmd.write_vmd(synth.make_bone_keys(names[k::2 + k], 70 + k, keys_per=4, span=90), [])) for k in range(2)]
        bms = [v.bind_bones(names) for v in vs]
        self.ms = vmd.MotionSet(bms)
        for x in bms + vs:
            x.close()
        self.dm = DeformModel(synth.make_model(NV, NB, 0, 0, seed=7301))
        self.clips = np.arange(NI, dtype=np.uint32) % 2
        self.times = (np.arange(NI) * 0.37) % 3.0
        self.d_clips, self.d_times = DeviceBuffer.from_numpy(self.clips), DeviceBuffer.from_numpy(self.times)
        self.d_place = DeviceBuffer(NI * 32)
        self.d_pal = DeviceBuffer(NI * NB * 64)
        na, nb = self.dm.out_sizes(api.OUT_SOA, NI)
        self.d_a, self.d_b, self.d_bnd = DeviceBuffer(na), DeviceBuffer(nb), DeviceBuffer(NI * 24)

    def frame(self):
        self.sk.solve_motion_set_time_device(self.ms, NI, self.d_clips.ptr, self.d_times.ptr, self.d_pal.ptr, self.dm)
        self.dm.place_palettes(NI, self.d_pal.ptr, self.d_place.ptr, self.d_pal.ptr, ALL_DEV)
        self.dm.deform_batched_raw(NI, None, self.d_pal.ptr, self.d_a.ptr, self.d_b.ptr, api.OUT_SOA, DEV, bounds_ptr=self.d_bnd.ptr)

    def results(self):
        self.dm.sync()
        return (self.d_pal.download((NI, NB, 16), F), self.d_a.download((NI, NV, 3), F), self.d_b.download((NI, NV, 3), F),
                self.d_bnd.download((NI, 6), F))

    def clear(self):
        for d in (self.d_pal, self.d_a, self.d_b, self.d_bnd):
            d.memset(0xFF)

    def from_host(self, placed):
        """The same deform fed palettes uploaded from the host -> (pos, nrm, bounds)."""
        d = DeviceBuffer.from_numpy(placed)
        self.dm.deform_batched_raw(NI, None, d.ptr, self.d_a.ptr, self.d_b.ptr, api.OUT_SOA, DEV, bounds_ptr=self.d_bnd.ptr)
        out = self.results()[1:]
        d.free()
        return out

    def close(self):
        for x in (self.d_clips, self.d_times, self.d_place, self.d_pal, self.d_a, self.d_b, self.d_bnd):
            x.free()
        for x in (self.dm, self.ms, self.sk):
            x.close()


@pytest.mark.gpu
def test_gpu_solve_place_deform_cull_end_to_end():
    """mmdx_skeleton_solve_motion_set_time -> mmdx_palette_place (pose form, in place) -> mmdx_deform_batched_bounds, everything in
    device memory: vertices and boxes equal, byte for byte, the same deform fed the restatement's placed palettes from the host; the
    boxes stand SPACING apart along x in instance order; the "frustum moved" camera of tests/test_cull_loop.py then sees a proper,
    non-empty part of the crowd."""
    assert device_count() >= 1, "no HIP device visible: the GPU tests must run on the MI355X box"
    from tests.test_cull_loop import loop_views
    lp = _Loop()
    placements = crowd_placements(lambda i: 0.05 + 0.01 * i)
    model_space = lp.sk.solve_motion_set_time(lp.ms, lp.clips, lp.times, lp.dm)
    unplaced = lp.from_host(model_space)[2]
    lp.d_place.upload(placements)
    lp.clear()
    lp.frame()
    pal, pos, nrm, bounds = lp.results()
    placed = pp.place_crowd(model_space, placements, False)
    gu.assert_bits_equal(pal, placed, "placed palettes")
    want_pos, want_nrm, want_bounds = lp.from_host(placed)
    gu.assert_bits_equal(pos, want_pos, "positions")
    gu.assert_bits_equal(nrm, want_nrm, "normals")
    gu.assert_bits_equal(bounds, want_bounds, "bounds")
    # in world space: a yaw keeps every vertex within its distance from the y axis, so box i lies inside x = t_i +- extent, the
    # extent being the largest such distance the un-placed boxes allow; and the centres follow the instances' order
    assert np.isfinite(bounds).all() and np.isfinite(unplaced).all()
    extent = float(np.sqrt(np.abs(unplaced[:, [0, 3]]).max() ** 2 + np.abs(unplaced[:, [2, 5]]).max() ** 2))
    tx = placements[:, 0].astype(np.float64)
    cx = (bounds[:, 0].astype(np.float64) + bounds[:, 3]) / 2
    print("extent %.2f, centre - t: %.2f .. %.2f, centre steps %.2f .. %.2f" % (extent, (cx - tx).min(), (cx - tx).max(),
                                                                                np.diff(cx).min(), np.diff(cx).max()))
    assert (bounds[:, 0] >= tx - extent - 1e-3).all() and (bounds[:, 3] <= tx + extent + 1e-3).all()
    assert (np.diff(cx) > 0).all() and (np.abs(np.diff(cx) - SPACING) <= extent).all()
    # the cull sees a part of the crowd, and exactly the part the restatement of the cull names
    what, view = loop_views()[0]
    assert what == "frustum moved"
    d_ids, d_cnt, d_lvl = DeviceBuffer(2 * NI * 4), DeviceBuffer(4 * 4), DeviceBuffer(NI * 4)
    lp.dm.cull_bounds(lp.d_bnd, view.struct(), NI, d_ids, d_cnt, d_lvl)
    lp.dm.sync()
    lists, levels = view.ref(bounds, False)
    cnt, ids, lvl = d_cnt.download((4,), np.uint32), d_ids.download((2, NI), np.uint32), d_lvl.download((NI,), np.uint32)
    assert cnt.tolist() == [len(lists[0]), len(lists[1]), 0, 0] and np.array_equal(lvl, levels)
    for l in range(2):
        assert np.array_equal(ids[l, :cnt[l]], lists[l])
    visible = int(cnt[0] + cnt[1])
    assert 0 < visible < NI, visible
    for d in (d_ids, d_cnt, d_lvl):
        d.free()
    lp.close()


@pytest.mark.gpu
def test_gpu_graph_of_solve_place_deform():
    """The three calls recorded once (after one direct run) and replayed three times, the placement array rewritten in device memory
    between replays -- the third time with identity placements.  After each replay the palette and the vertices equal the direct
    calls with those placements."""
    assert device_count() >= 1, "no HIP device visible: the GPU tests must run on the MI355X box"
    lp = _Loop()
    frames = [crowd_placements(lambda i: 0.05 + 0.01 * i), crowd_placements(lambda i: -0.7 + 0.11 * i)[::-1].copy(),
              np.tile(pp.IDENTITY_POSE, (NI, 1))]
    direct = []
    for placements in frames:
        lp.d_place.upload(placements)
        lp.clear()
        lp.frame()
        direct.append(lp.results())
    assert len({d[0].tobytes() for d in direct}) == 3 and len({d[1].tobytes() for d in direct}) == 3
    lp.dm.graph_begin()
    lp.frame()
    graph = lp.dm.graph_end()
    for k, placements in enumerate(frames):
        lp.d_place.upload(placements)
        lp.clear()
        graph.launch()
        got = lp.results()
        for name, g, w in zip(("palettes", "positions", "normals", "bounds"), got, direct[k]):
            gu.assert_bits_equal(g, w, "replay %d: %s" % (k + 1, name))
    graph.close()
    lp.close()

"""Bone sockets: mmdx_socket_set_* and mmdx_palette_sockets (include/mmdx.h), out[s][i] = (O[s] *) G[s] * S[i][bone[s]] with G the
identity whose row 4 is the bone's rest position (libmmd's global_offset_matrix_inv_) and O the socket's optional local offset.

Every product is libmmd's Matrix4x4<float>::operator*, so everything is compared as bit patterns; the one exception is that a NaN
only has to be a NaN (its sign and payload are not part of the contract):
  * tests/golden/palette_sockets_expect.npz comes from the real libmmd (tests/palette_sockets_driver.cpp,
    tests/gen_palette_sockets_golden.py);
  * tests/palette_sockets_ref.py restates the arithmetic in numpy float32 and reproduces that fixture on the CPU;
  * tests/socket_math_driver.cpp runs csrc/socket_math.hpp -- the lines the kernel compiles -- and the host table builder
    csrc/socket_table.hpp on the CPU, also under ASan + UBSan, as a stand-alone program;
  * on the GPU (rig_small: 24 bones) crowds of 1, 3, 65 and 257 instances and sets of 1, 3 and 17 sockets are held to the restatement
    on model-space and on placed palettes, with device and with host operands and sentinels around the output; the fixture's own
    rows go through the kernel as a synthetic palette; select lists in host and in device memory leave every unlisted byte alone;
    and solve -> place -> sockets -> place of a prop crowd at a socket slab -> deform of the prop is recorded and replayed.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from simple_mmd_renderer_amd import _capi as api
from simple_mmd_renderer_amd import synth, vmd
from simple_mmd_renderer_amd.engine import DeformModel, DeviceBuffer, SocketSet, device_count, device_synchronize
from tests import golden_util as gu
from tests import host_program as hp
from tests import motion_time_ref as mt
from tests import palette_place_ref as pp
from tests import palette_sockets_ref as ps
from tests.test_capi_symbols import declared_symbols

F = np.float32
INVALID, BAD_INDEX, NO_DEVICE = 1, 2, 3
DEV = api.PALETTE_ON_DEVICE | api.OUT_ON_DEVICE
PLACE_DEV = api.PALETTE_ON_DEVICE | api.PLACE_ON_DEVICE | api.OUT_ON_DEVICE
GUARD = 256                    # sentinel bytes in front of and behind an output array
SENT = 0xEE
NB = 24                        # rig_small's bone count
needs_driver = pytest.mark.skipif(not mt.driver_available(), reason="the reference's libmmd headers are not present")
NEW_SYMBOLS = ("mmdx_socket_set_create", "mmdx_socket_set_destroy", "mmdx_socket_set_get_info", "mmdx_palette_sockets")


@pytest.fixture(autouse=True)
def _lib(hip_lib):
    return hip_lib


def rig_small():
    return np.load(os.path.join(gu.GOLDEN_DIR, "rig_small_expect.npz"))


def rig_model(**kw):
    """A model with rig_small's 24 bones (the sockets call takes nothing else from its model)."""
    return DeformModel(synth.make_model(64, NB, 0, 0, seed=31), **kw)


# ---------------------------------------------------------------------------------------- CPU ----
def test_socket_entry_points_are_declared_exported_and_bound(hip_lib):
    for name in NEW_SYMBOLS:
        assert name in declared_symbols() and hasattr(hip_lib, name) and name in api.SIGNATURES, name
    inc = os.path.join(ps.ROOT, "include")
    hdr = open(os.path.join(inc, "mmdx.h")).read()
    assert "typedef struct mmdx_sockets_args {" in hdr and "#define MMDX_ABI_VERSION 3u" in hdr and "global_offset_matrix_inv_" in hdr
    assert "SOCKET-major" in hdr and "MMDX_PLACE_MATRIX | MMDX_PLACE_ON_DEVICE" in hdr.split("} mmdx_sockets_args;")[1]
    assert hip_lib.mmdx_abi_version() == 3
    desc, info, args, flag = hp.c_values(["sizeof(mmdx_socket_set_desc)", "sizeof(mmdx_socket_set_info)", "sizeof(mmdx_sockets_args)",
                                          "MMDX_SOCKET_OFFSET_MATRIX"])
    assert C.sizeof(api.SocketSetDesc) == desc == 4 * 4 + 4 * 8
    assert C.sizeof(api.SocketSetInfo) == info == 6 * 4
    assert C.sizeof(api.SocketsArgs) == args == 4 * 4 + 3 * 8
    assert api.SOCKET_OFFSET_MATRIX == flag == 1
    assert callable(SocketSet.sockets) and callable(SocketSet.sockets_host) and callable(SocketSet.from_pmx) and callable(SocketSet.from_skeleton)
    poser = open(os.path.join(ps.ROOT, "simple_mmd_renderer_amd", "host", "mmdx_poser.hpp")).read()
    assert "mmdx_palette_sockets(" in poser and "class SocketSet" in poser


def test_numpy_restatement_reproduces_the_libmmd_fixture():
    z = ps.fixture()
    assert 280 <= z["form"].size <= 360 and os.path.getsize(ps.FIXTURE) < 64 * 1024
    ps.assert_rows_equal(ps.socket_rows(z["form"], z["s"], z["rest"], z["offset"]), z["expect"], "restatement vs libmmd")


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan-ubsan"])
def test_socket_math_header_and_table_builder_reproduce_the_fixture_on_the_cpu(sanitize):
    """csrc/socket_math.hpp, the code the kernel compiles, behind csrc/socket_table.hpp, the code mmdx_socket_set_create runs, as a
    stand-alone host program (-ffp-contract=off; the second build with -fsanitize=address,undefined, run directly)."""
    z = ps.fixture()
    got = ps.run_driver(ps.build_math_driver(sanitize), z["form"], z["s"], z["rest"], z["offset"])
    ps.assert_rows_equal(got, z["expect"], "socket_math.hpp vs libmmd")


def test_a_pose_offset_equals_its_expanded_matrix_offset_bit_for_bit():
    """On the fixture's pose rows: the same rows with the offset replaced by the matrix it expands to, through the header driver
    (which expands a pose where the library does) and through the restatement, against libmmd's own pose-form results."""
    z = ps.fixture()
    rows = z["form"] == ps.POSE
    s, rest, off, want = z["s"][rows], z["rest"][rows], z["offset"][rows], z["expect"][rows]
    expanded = pp.matrix_from_pose(off[:, :8])
    as_matrix = np.full(int(rows.sum()), ps.MATRIX, np.uint8)
    ps.assert_rows_equal(ps.run_driver(ps.build_math_driver(), as_matrix, s, rest, expanded), want, "header: matrix form of a pose offset")
    ps.assert_rows_equal(ps.socket_rows(as_matrix, s, rest, expanded), want, "restatement: matrix form of a pose offset")


def test_rows_1_to_3_of_a_socket_without_offset_are_the_skinning_matrix_rows():
    """G's first three rows are the identity's: wherever S and p are finite the full four-term sums give S's rows back (compared with
    ==, so +-0 are equal)."""
    z = ps.fixture()
    rows = (z["form"] == ps.NONE) & np.isfinite(z["s"]).all(axis=1) & np.isfinite(z["rest"]).all(axis=1)
    assert rows.sum() >= 90
    assert (z["expect"][rows][:, :12] == z["s"][rows][:, :12]).all()
    # ... and row 4 is p taken through S: the bone's origin.  With the identity as S it is p itself.
    ident = np.eye(4, dtype=F).reshape(1, 16)
    p = z["rest"][rows]
    assert (ps.bone_frame(ident, p)[:, 12:15] == p).all()


def test_fixture_covers_what_it_claims():
    z = ps.fixture()
    form, s, p, o, e, kind = z["form"], z["s"], z["rest"], z["offset"], z["expect"], np.array(z["kind"])
    none, pose, mat = form == ps.NONE, form == ps.POSE, form == ps.MATRIX
    assert none.sum() >= 100 and pose.sum() >= 90 and mat.sum() >= 90
    assert {"bone", "rest", "unit", "nonunit", "rigid", "scaled", "sheared", "negzero", "denormal", "inf", "nan"} == set(kind)
    tiny = np.finfo(F).tiny
    # the rest positions: rig_small's own, and 0, -0, a denormal and 1e4
    rig = {r.tobytes() for r in rig_small()["rest"].astype(F)}
    assert sum(r.tobytes() in rig for r in p) >= 250
    rest = p[kind == "rest"]
    assert (gu.bits(rest) == 0x80000000).any() and (gu.bits(rest) == 0).any() and ((rest != 0) & (np.abs(rest) < tiny)).any() and (rest == 1e4).any()
    # pose offsets: both hemispheres, non-unit, the zero quaternion, the ignored fourth float set
    fin = np.isfinite(o).all(axis=1) & np.isfinite(s).all(axis=1) & np.isfinite(p).all(axis=1)
    qw = o[pose & fin, 7]
    assert (qw > 0).sum() >= 25 and (qw < 0).sum() >= 25
    norm2 = (o[pose & fin, 4:8].astype(np.float64) ** 2).sum(axis=1)
    assert (np.abs(norm2 - 1) > 0.1).sum() >= 8 and (norm2 == 0).any() and (o[pose, 3] != 0).sum() >= 25
    # matrix offsets: a fourth column other than (0, 0, 0, 1)
    assert (o[kind == "sheared"][:, [3, 7, 11]] != 0).any() and (o[kind == "sheared"][:, 15] != 1).any()
    # every special class in S, in p and -- where the form has one -- in the offset
    for f, width in ((none, 0), (pose, 8), (mat, 16)):
        live = np.zeros(16, bool)
        live[:width] = True
        if width == 8:
            live[3] = False
        for what, hit in (("-0", lambda a: gu.bits(a) == 0x80000000), ("denormal", lambda a: (a != 0) & (np.abs(a) < tiny)),
                          ("inf", np.isinf), ("nan", np.isnan)):
            assert hit(s[f]).any() and hit(p[f]).any() and (not width or hit(o[f][:, live]).any()), (width, what)
    assert np.isnan(e).any() and np.isinf(e).any()
    real = {r.tobytes() for r in rig_small()["expect_palettes"].reshape(-1, 16)}
    assert sum(r.tobytes() in real for r in s) >= 250


@needs_driver
def test_fixture_equals_a_fresh_run_of_libmmd():
    z = ps.fixture()
    got = ps.run_driver(ps.build_libmmd_driver(), z["form"], z["s"], z["rest"], z["offset"])
    ps.assert_rows_equal(got, z["expect"], "fresh libmmd run")


def _desc(bone, rest, offset=None, flags=0, n=None, struct_size=None, reserved0=0, has=None):
    d = api.SocketSetDesc()
    d.struct_size = C.sizeof(api.SocketSetDesc) if struct_size is None else struct_size
    d.flags, d.n_sockets, d.reserved0 = flags, (len(bone) if n is None else n), reserved0
    d.bone = bone.ctypes.data if bone is not None else None
    d.rest_position = rest.ctypes.data if rest is not None else None
    d.offset = offset.ctypes.data if offset is not None else None
    d.has_offset = has.ctypes.data if has is not None else None
    return d


def test_socket_set_create_refuses_bad_descs():
    lib = api.lib()
    err = lambda: lib.mmdx_last_error_string().decode()          # noqa: E731
    bone, rest, off = np.array([0, 4, 4], np.uint32), np.zeros((3, 3), F), np.zeros((3, 16), F)
    with DeformModel(synth.make_model(64, 5, 0, 0, seed=11), host_only=True) as dm:
        h = C.c_void_p()
        create = lambda d, m=dm.h, out=h: lib.mmdx_socket_set_create(m, C.byref(d) if d is not None else None,          # noqa: E731
                                                                      C.byref(out) if out is not None else None)
        assert create(_desc(bone, rest), None) == INVALID and "NULL" in err()
        assert create(None) == INVALID and "NULL" in err()
        assert create(_desc(bone, rest), dm.h, None) == INVALID and "NULL" in err()
        assert create(_desc(None, rest, n=3)) == INVALID and "NULL" in err()
        assert create(_desc(bone, None)) == INVALID and "NULL" in err()
        assert create(_desc(bone, rest, n=0)) == INVALID and "n_sockets" in err()
        assert create(_desc(bone, rest, n=65536)) == INVALID and "n_sockets" in err()
        for size in (0, C.sizeof(api.SocketSetDesc) - 8, C.sizeof(api.SocketSetDesc) + 8):
            assert create(_desc(bone, rest, struct_size=size)) == INVALID and "struct_size" in err(), size
        for bad in (1 << 1, 1 << 8, 1 << 31):
            assert create(_desc(bone, rest, flags=bad)) == INVALID and "unknown flag" in err(), bad
        assert create(_desc(bone, rest, reserved0=1)) == INVALID and "reserved0" in err()
        assert create(_desc(bone, rest, has=np.ones(3, np.uint8))) == INVALID and "has_offset" in err()
        assert create(_desc(np.array([0, 5, 1], np.uint32), rest)) == BAD_INDEX and "bone[1] = 5" in err()
        assert h.value is None
        # valid: no offsets, pose offsets, matrix offsets on some sockets; the info says what was created
        for d, n_off in ((_desc(bone, rest), 0), (_desc(bone, rest, off[:, :8].copy()), 3),
                         (_desc(bone, rest, off, api.SOCKET_OFFSET_MATRIX, has=np.array([0, 1, 0], np.uint8)), 1)):
            assert create(d) == api.OK and h.value
            info = api.SocketSetInfo()
            assert lib.mmdx_socket_set_get_info(h, C.byref(info)) == INVALID and "struct_size" in err()
            info.struct_size = C.sizeof(api.SocketSetInfo)
            assert lib.mmdx_socket_set_get_info(h, C.byref(info)) == api.OK
            assert (info.n_sockets, info.n_offsets, info.n_bones, info.device_ordinal) == (3, n_off, 5, -1)
            lib.mmdx_socket_set_destroy(h)
        lib.mmdx_socket_set_destroy(None)


def test_sockets_call_refuses_bad_arguments():
    """Everything is decided before the first HIP call, so a set on a host-only model shows it without a GPU: a valid call gets as far
    as MMDX_ERR_NO_DEVICE, every mistake is MMDX_ERR_INVALID_ARGUMENT first."""
    lib = api.lib()
    err = lambda: lib.mmdx_last_error_string().decode()          # noqa: E731
    ni, nb, ns = 3, 5, 2
    pal = np.zeros((ni, nb, 16), F)
    out = np.zeros((ns, ni, 16), F)
    ids = np.array([2, 0, 1], np.uint32)
    keep = []

    def args(n=ni, flags=0, struct_size=None, reserved0=0, palettes=pal.ctypes.data, out_sockets=out.ctypes.data, select=None):
        a = api.SocketsArgs()
        a.struct_size = C.sizeof(api.SocketsArgs) if struct_size is None else struct_size
        a.flags, a.n_instances, a.reserved0 = flags, n, reserved0
        a.palettes, a.out_sockets = palettes, out_sockets
        if select is not None:
            keep.append(select)
            a.select = C.pointer(select)
        return a
    dm = DeformModel(synth.make_model(64, nb, 0, 0, seed=11), host_only=True)
    sset = SocketSet(dm, [0, 4], np.zeros((2, 3), F))
    call = lambda a, h=sset.h: lib.mmdx_palette_sockets(h, C.byref(a) if a is not None else None)          # noqa: E731
    assert call(args(), None) == INVALID and "NULL" in err()
    assert call(None) == INVALID and "NULL" in err()
    for k in ("palettes", "out_sockets"):
        assert call(args(**{k: None})) == INVALID and "NULL" in err(), k
    for size in (0, C.sizeof(api.SocketsArgs) - 8, C.sizeof(api.SocketsArgs) + 8):
        assert call(args(struct_size=size)) == INVALID and "struct_size" in err(), size
    for bad in (1 << 1, 1 << 3, 1 << 8, 1 << 9, 1 << 31):
        assert call(args(flags=bad)) == INVALID and "unknown flag" in err(), bad
    assert call(args(reserved0=1)) == INVALID and "reserved0" in err()
    # out_sockets inside, or straddling an end of, palettes; directly behind or in front is fine
    big = np.zeros((ni * nb + 2 * ns * ni + 2) * 16, F)
    base = big.ctypes.data + ns * ni * 64
    for at in (base, base + 64, base + ni * nb * 64 - 4, base - ns * ni * 64 + 4):
        assert call(args(palettes=base, out_sockets=at)) == INVALID and "overlaps" in err(), at - base
    assert call(args(palettes=base, out_sockets=base + ni * nb * 64)) == NO_DEVICE
    assert call(args(palettes=base, out_sockets=base - ns * ni * 64)) == NO_DEVICE
    # device operands: alignment
    assert call(args(flags=api.PALETTE_ON_DEVICE, palettes=pal.ctypes.data + 8)) == INVALID and "16-byte" in err()
    assert call(args(flags=api.OUT_ON_DEVICE, out_sockets=out.ctypes.data + 4)) == INVALID and "16-byte" in err()
    # the list: its header, host operands with a list, a host id that is no instance
    sel = vmd.instance_select(ids.ctypes.data, 2, on_device=False)
    assert call(args(flags=DEV, select=sel)) == NO_DEVICE
    assert call(args(select=sel)) == INVALID and "select list" in err()
    bad_sel = vmd.instance_select(ids.ctypes.data, 2, on_device=False)
    bad_sel.struct_size -= 8
    assert call(args(flags=DEV, select=bad_sel)) == INVALID and "mmdx_instance_select" in err()
    bad_sel = vmd.instance_select(ids.ctypes.data, 2, on_device=False)
    bad_sel.flags = 2
    assert call(args(flags=DEV, select=bad_sel)) == INVALID and "mmdx_instance_select" in err()
    no_instance = np.array([0, 3], np.uint32)
    assert call(args(flags=DEV, select=vmd.instance_select(no_instance.ctypes.data, 2, on_device=False))) == INVALID and "ids[1] = 3" in err()
    assert call(args(flags=DEV, select=vmd.instance_select(ids.ctypes.data + 2, 2))) == INVALID and "4-byte" in err()
    # nothing to do is not an error, whatever the pointers; a valid call needs a device
    assert call(args(n=0)) == api.OK and call(args(n=0, palettes=None, out_sockets=None)) == api.OK
    for flags in (0, api.PALETTE_ON_DEVICE, DEV):
        assert call(args(flags=flags)) == NO_DEVICE, flags
    with pytest.raises(api.MmdxError) as e:
        sset.sockets_host(pal)
    assert e.value.status == NO_DEVICE
    # the model goes first: the set refuses every call and can still be destroyed
    dm.close()
    assert call(args()) == INVALID and "destroyed" in err()
    sset.close()


def test_python_helpers_build_the_desc_from_pmx_arrays_and_from_a_skeleton():
    """SocketSet.from_pmx takes bone names or indices and the loaded model's rest positions, SocketSet.from_skeleton a
    vmd.Skeleton's; both go through the constructor, whose arrays the GPU tests hold to the restatement."""
    from simple_mmd_renderer_amd import pmx
    pm = pmx.load_pmx(os.path.join(gu.GOLDEN_DIR, "pmx_small.pmx"))
    nb = len(pm.bone_names)
    seen = {}

    class Spy(SocketSet):
        def __init__(self, model, bones, rest_position, offsets=None, has_offset=None):
            seen["bones"], seen["rest"] = np.asarray(bones), np.asarray(rest_position, F)
            super().__init__(model, bones, rest_position, offsets, has_offset)
    with DeformModel(pm.flat, host_only=True) as dm:
        with Spy.from_pmx(dm, pm, [pm.bone_names[nb - 1], 0, pm.bone_names[1]]) as s:
            assert (s.ns, s.nb, s.info["n_offsets"], s.info["device_ordinal"]) == (3, nb, 0, -1)
            assert seen["bones"].tolist() == [nb - 1, 0, 1]
            gu.assert_bits_equal(seen["rest"], np.asarray(pm.flat.bone_pos, F)[[nb - 1, 0, 1]], "rest positions from the PMX arrays")
        with pytest.raises(ValueError):
            Spy.from_pmx(dm, pm, ["no such bone"])
        sk = pm.skeleton()
        off = np.tile(pp.IDENTITY_POSE, (2, 1))
        with Spy.from_skeleton(dm, sk, [1, nb - 1], off, [True, False]) as s:
            assert (s.ns, s.info["n_offsets"]) == (2, 1)
            gu.assert_bits_equal(seen["rest"], np.asarray(pm.flat.bone_pos, F)[[1, nb - 1]], "rest positions from the skeleton")
        with pytest.raises(api.MmdxError) as e:
            SocketSet(dm, [nb], np.zeros((1, 3), F))
        assert e.value.status == BAD_INDEX
        sk.close()


def test_socket_kernels_have_no_spills_and_no_scratch(hip_lib):
    out = subprocess.run([sys.executable, os.path.join(ps.ROOT, "tools", "kernel_resources.py"), api.LIB_PATH, "palette_sockets"],
                         capture_output=True, text=True, check=True).stdout.splitlines()
    names = {l.split(" vgpr ")[0].strip() for l in out}
    assert names == {"palette_sockets_kernel<%s, %s>" % (a, b) for a in ("true", "false") for b in ("true", "false")}
    for l in out:
        f = ("vgpr " + l.split(" vgpr ")[1]).split()
        res = dict(zip(f[0::2], (int(v) for v in f[1::2])))
        assert res["spill"] == 0 and res["scratch"] == 0 and res["lds"] == 0 and res["vgpr"] <= 64, l


# ---------------------------------------------------------------------------------------- GPU ----
class Out:
    """A device output of `nbytes` with GUARD sentinel bytes on both sides; `ptr` is what the library is given."""

    def __init__(self, nbytes):
        self.nbytes = int(nbytes)
        self.buf = DeviceBuffer(self.nbytes + 2 * GUARD)
        self.ptr = self.buf.ptr + GUARD
        self.buf.memset(SENT)

    def fill(self):
        self.buf.memset(SENT)

    def read(self, what):
        raw = self.buf.download((self.nbytes + 2 * GUARD,), np.uint8)
        assert (raw[:GUARD] == SENT).all() and (raw[GUARD + self.nbytes:] == SENT).all(), f"{what}: bytes outside the output were written"
        return raw[GUARD:GUARD + self.nbytes].copy()

    def free(self):
        self.buf.free()


@pytest.fixture(scope="module")
def gpu(hip_lib):
    assert device_count() >= 1, "no HIP device visible: the GPU tests must run on the MI355X box"
    return hip_lib


def crowd_poses(ni, shift=0.0):
    """rig_small's own evaluated poses, frame (i mod 75) for instance i, each lap moved a little so that no two instances agree."""
    z = rig_small()
    poses = z["expect_poses"][np.arange(ni) % 75].copy()
    poses[:, :, 0] += (np.arange(ni) // 75 * 0.125 + shift).astype(F)[:, None]
    return poses


def crowd_placements(ni):
    p = np.zeros((ni, 8), F)
    p[:, 0], p[:, 2] = (np.arange(ni) % 16 - 8) * 12.0, (np.arange(ni) // 16) * 9.0
    yaw = 0.05 + 0.37 * np.arange(ni)
    p[:, 5], p[:, 7] = np.sin(yaw / 2), np.cos(yaw / 2)
    return p


_crowds = {}


def crowd(ni):
    """(model-space palettes, placed palettes) of the ni-instance crowd, computed once: mmdx_skeleton_solve on rig_small's skeleton,
    then the restatement of mmdx_palette_place (tests/test_palette_place.py pins the call to it)."""
    if ni not in _crowds:
        z = rig_small()
        sk = vmd.Skeleton(z["rest"], z["parent"], z["level"], z["flags"])
        with rig_model() as dm:
            pal = sk.solve(crowd_poses(ni), dm)
        sk.close()
        assert np.isfinite(pal).all()
        _crowds[ni] = (pal, pp.place_crowd(pal, crowd_placements(ni), False))
    return _crowds[ni]


def socket_set_args(ns):
    """(bones, offsets or None, matrix form?, has_offset or None): bone 0, the last bone and a repeated bone in every set of more than
    one socket; no offsets (ns = 1), pose offsets on some sockets (3), matrix offsets -- scaled and sheared -- on some (17)."""
    rng = np.random.RandomState(500 + ns)
    if ns == 1:
        return np.array([NB - 1], np.uint32), None, False, None
    bones = np.concatenate([[0, NB - 1, 7, 7], rng.randint(0, NB, size=ns)]).astype(np.uint32)[:ns]
    if ns == 3:
        bones = np.array([0, NB - 1, NB - 1], np.uint32)
        q = rng.normal(size=(ns, 4))
        off = np.zeros((ns, 8), F)
        off[:, :3], off[:, 3], off[:, 4:] = rng.uniform(-2, 2, (ns, 3)), 5.0, q / np.linalg.norm(q, axis=1, keepdims=True)
        return bones, off, False, np.array([1, 0, 1], bool)
    from tests.gen_palette_place_golden import matrices
    return bones, matrices(rng, ns, sheared=True), True, (np.arange(ns) % 3 != 1)


def make_set(dm, ns):
    bones, off, matrix, has = socket_set_args(ns)
    rest = rig_small()["rest"].astype(F)[bones]
    sset = SocketSet(dm, bones, rest, off, has)
    assert sset.info["n_offsets"] == (0 if off is None else int(has.sum())) and sset.info["device_ordinal"] >= 0
    return sset, lambda pal: ps.sockets(pal, bones, rest, off, matrix, has)


@pytest.mark.gpu
@pytest.mark.parametrize("ns", [1, 3, 17])
@pytest.mark.parametrize("ni", [1, 3, 65, 257])
def test_gpu_sockets_equal_the_restatement(gpu, ni, ns):
    """4 rows in a partial wave, 12 rows, 260 rows (two workgroups, the second of one partial wave) and 1 028 rows (five workgroups)
    per socket.  Model-space palettes from mmdx_skeleton_solve and the same palettes placed (the socket is then G * (S * W)); device
    operands with 256 sentinel bytes around the output, then host operands."""
    model_space, placed = crowd(ni)
    with rig_model() as dm:
        sset, ref = make_set(dm, ns)
        out = Out(ns * ni * 64)
        for what, pal in (("model space", model_space), ("placed", placed)):
            want = ref(pal)
            assert want.shape == (ns, ni, 16) and np.isfinite(want).all()
            d_pal = DeviceBuffer.from_numpy(pal)
            out.fill()
            sset.sockets(d_pal, out.ptr)
            dm.sync()
            gu.assert_bits_equal(out.read(what).view(F).reshape(ns, ni, 16), want, f"{ni}x{ns} {what}: device operands")
            gu.assert_bits_equal(d_pal.download(pal.shape, F), pal, f"{ni}x{ns} {what}: the call changed its input")
            gu.assert_bits_equal(sset.sockets_host(pal), want, f"{ni}x{ns} {what}: host operands")
            # mixed: host palettes to a device output, device palettes to a host output
            out.fill()
            sset.sockets_raw(ni, pal.ctypes.data, out.ptr, api.OUT_ON_DEVICE)
            gu.assert_bits_equal(out.read(what).view(F).reshape(ns, ni, 16), want, f"{ni}x{ns} {what}: host palettes, device output")
            host = np.empty((ns, ni, 16), F)
            sset.sockets_raw(ni, d_pal.ptr, host.ctypes.data, api.PALETTE_ON_DEVICE)
            gu.assert_bits_equal(host, want, f"{ni}x{ns} {what}: device palettes, host output")
            d_pal.free()
        # placed: the bone's world frame, the model-space frame taken through W up to the rounding of the products (float64 here)
        rest0 = rig_small()["rest"].astype(F)[0]
        w = pp.world_matrices(crowd_placements(ni), False).astype(np.float64).reshape(ni, 4, 4)
        b = ps.bone_frame(model_space[:, 0, :], rest0).astype(np.float64).reshape(ni, 4, 4)
        world = ps.bone_frame(placed[:, 0, :], rest0).astype(np.float64).reshape(ni, 4, 4)
        assert np.abs(world - b @ w).max() <= 1e-3
        out.free()
        sset.close()


@pytest.mark.gpu
@pytest.mark.parametrize("form", [ps.POSE, ps.MATRIX], ids=["none+pose", "none+matrix"])
def test_gpu_fixture_rows_through_the_kernel(gpu, form):
    """The libmmd fixture as a synthetic crowd: row r of the rows without an offset and with an offset of `form` becomes socket r of a
    set (its own rest position, its own offset) on bone r mod 24, and its S becomes bone r mod 24 of instance r div 24.  Socket r of
    instance r div 24 must be libmmd's row; every other (socket, instance) pair must be the restatement's."""
    z = ps.fixture()
    rows = (z["form"] == ps.NONE) | (z["form"] == form)
    s, rest, off, expect, has = z["s"][rows], z["rest"][rows], z["offset"][rows], z["expect"][rows], z["form"][rows] != ps.NONE
    n = int(rows.sum())
    ni = (n + NB - 1) // NB
    pal = np.zeros((ni * NB, 16), F)
    pal[:] = np.eye(4, dtype=F).reshape(16)
    pal[:n] = s
    pal = pal.reshape(ni, NB, 16)
    bones = (np.arange(n) % NB).astype(np.uint32)
    offsets = off if form == ps.MATRIX else np.ascontiguousarray(off[:, :8])
    with rig_model() as dm:
        sset = SocketSet(dm, bones, rest, offsets, has)
        d_pal, out = DeviceBuffer.from_numpy(pal), Out(n * ni * 64)
        sset.sockets(d_pal, out.ptr)
        dm.sync()
        got = out.read("fixture").view(F).reshape(n, ni, 16)
        ps.assert_rows_equal(got[np.arange(n), np.arange(n) // NB], expect, "fixture rows through the kernel vs libmmd")
        ps.assert_rows_equal(got, ps.sockets(pal, bones, rest, offsets, form == ps.MATRIX, has), "every pair vs the restatement")
        ps.assert_rows_equal(sset.sockets_host(pal), got, "host operands")
        d_pal.free()
        out.free()
        sset.close()


SEL_IDS = np.array([3, 64, 0, 7, 7, 33, 1, 12], np.uint32)                  # capacity 8, one instance twice
SEL_IDS_DEV = np.array([3, 64, 0, 70, 7, 7, 0xFFFFFFFF, 12], np.uint32)     # device list: 70 and 2^32-1 are no instances of 65


def _expect_selected(want, ids, ni):
    """The sentinel everywhere, the restatement's rows for the listed instances that exist -> u8 [NS, NI, 64]."""
    exp = np.full((want.shape[0], want.shape[1], 64), SENT, np.uint8)
    live = [int(i) for i in ids if i < ni]
    exp[:, live] = want.view(np.uint8).reshape(want.shape[0], want.shape[1], 64)[:, live]
    return exp


@pytest.mark.gpu
@pytest.mark.parametrize("where", ["host list", "device list"])
def test_gpu_select_leaves_every_unlisted_byte_alone(gpu, where):
    """65 instances, 3 sockets (offsets on two), the output prefilled with 0xEE and 256 sentinel bytes around it: count NULL, 0, 5 and
    100 (> n_ids); a device list also holds two ids that are no instance.  Rows of unlisted instances, in every slab, and the bytes
    past the slab ends keep every byte."""
    ni, ns = 65, 3
    _, placed = crowd(ni)
    with rig_model() as dm:
        sset, ref = make_set(dm, ns)
        want = ref(placed)
        d_pal, out = DeviceBuffer.from_numpy(placed), Out(ns * ni * 64)
        ids = SEL_IDS if where == "host list" else SEL_IDS_DEV
        d_ids, d_cnt = DeviceBuffer.from_numpy(ids), DeviceBuffer(4)
        for count in (None, 0, 5, 100):
            out.fill()
            if where == "host list":
                cnt = C.c_uint32(count or 0)
                sel = vmd.instance_select(ids.ctypes.data, ids.size, C.addressof(cnt) if count is not None else None, on_device=False)
            else:
                d_cnt.upload(np.array([count or 0], np.uint32))
                sel = vmd.instance_select(d_ids.ptr, ids.size, d_cnt.ptr if count is not None else None)
            sset.sockets(d_pal, out.ptr, select=sel, n_instances=ni)
            dm.sync()
            used = ids if count is None else ids[:min(count, ids.size)]
            got = out.read(f"{where}, count {count}").reshape(ns, ni, 64)
            exp = _expect_selected(want, used, ni)
            bad = np.argwhere((got != exp).any(axis=2))
            assert not bad.size, f"{where}, count {count}: (socket, instance) {bad[:4].tolist()} differ"
            assert (got != SENT).any() == bool(len(used))
        # a list of capacity 0
        out.fill()
        sset.sockets(d_pal, out.ptr, select=vmd.instance_select(d_ids.ptr, 0), n_instances=ni)
        dm.sync()
        assert (out.read("n_ids 0") == SENT).all()
        for d in (d_pal, d_ids, d_cnt):
            d.free()
        out.free()
        sset.close()


class _PropFrame:
    """Characters (rig_small, 65 instances) holding props: solve -> place -> sockets -> place of the prop crowd's palettes at slab
    SLAB -> deform of the prop, all in device memory, both models on one stream."""
    NI, NS, SLAB, PROP_NV, PROP_NB = 65, 3, 2, 130, 3

    def __init__(self):
        z = rig_small()
        self.z = z
        self.sk = vmd.Skeleton(z["rest"], z["parent"], z["level"], z["flags"])
        self.dm = rig_model()
        self.prop = synth.make_model(self.PROP_NV, self.PROP_NB, 0, 0, seed=77)
        self.pm = DeformModel(self.prop)
        self.sset, self.ref = make_set(self.dm, self.NS)
        ni = self.NI
        self.placements = crowd_placements(ni)
        self.prop_pal = np.ascontiguousarray(synth.make_palettes(self.prop, np.arange(ni) % 5 + 1), F).reshape(ni, self.PROP_NB, 16)
        self.d_poses = DeviceBuffer(ni * NB * 32)
        self.d_pal = Out(ni * NB * 64)
        self.d_place = DeviceBuffer.from_numpy(self.placements)
        self.d_sock = Out(self.NS * ni * 64)
        self.d_prop_pal = DeviceBuffer.from_numpy(self.prop_pal)
        self.d_prop_placed = Out(ni * self.PROP_NB * 64)
        na, nb = self.pm.out_sizes(api.OUT_SOA, ni)
        self.d_pos, self.d_nrm = Out(na), Out(nb)
        self.outs = dict(palettes=self.d_pal, sockets=self.d_sock, prop_palettes=self.d_prop_placed, positions=self.d_pos, normals=self.d_nrm)

    def frame(self):
        ni = self.NI
        self.sk.solve_device(ni, self.d_poses.ptr, self.d_pal.ptr, self.dm)
        self.dm.place_palettes(ni, self.d_pal.ptr, self.d_place.ptr, self.d_pal.ptr, PLACE_DEV)
        self.sset.sockets(self.d_pal.ptr, self.d_sock.ptr, n_instances=ni)
        self.pm.place_palettes(ni, self.d_prop_pal.ptr, self.d_sock.ptr + self.SLAB * ni * 64, self.d_prop_placed.ptr,
                               PLACE_DEV | api.PLACE_MATRIX)
        self.pm.deform_batched_raw(ni, None, self.d_prop_placed.ptr, self.d_pos.ptr, self.d_nrm.ptr, api.OUT_SOA, DEV)

    def fill(self):
        for o in self.outs.values():
            o.fill()

    def read(self, what):
        return {k: o.read(f"{what}: {k}") for k, o in self.outs.items()}

    def expect(self, poses, oracle):
        """The numpy socket matrices of the oracle's palettes, and the oracle's deform of the prop under them."""
        ni, z = self.NI, self.z
        pal = np.stack([oracle.bone_solve(z["rest"], z["parent"], poses[i], z["level"], z["flags"]) for i in range(ni)])
        placed = pp.place_crowd(pal, self.placements, False)
        sockets = self.ref(placed)
        prop_placed = pp.place_crowd(self.prop_pal, sockets[self.SLAB], True)
        skin = oracle.normalize(self.prop)
        pos, nrm = zip(*(oracle.skin(self.prop, prop_placed[i], None, skin) for i in range(ni)))
        return dict(palettes=placed, sockets=sockets, prop_palettes=prop_placed, positions=np.stack(pos), normals=np.stack(nrm))

    def close(self):
        for o in self.outs.values():
            o.free()
        for d in (self.d_poses, self.d_place, self.d_prop_pal):
            d.free()
        self.sset.close()
        for x in (self.pm, self.dm, self.sk):
            x.close()


@pytest.mark.gpu
def test_gpu_graph_of_solve_place_sockets_prop_place_deform_on_a_borrowed_stream(gpu, oracle):
    """The five calls run once directly on a stream of the test's that both models borrow, are recorded on it -- after the recording
    and a device-wide synchronisation every output byte still holds its sentinel, so nothing ran and nothing went to another stream --
    and are replayed twice with the poses rewritten in device memory in between.  After each replay the sockets equal the restatement
    on the oracle's placed palettes, and the prop's vertices the oracle's deform under those socket matrices."""
    from tests import hip_stream_util as hs
    hs.hip()
    fr = _PropFrame()
    frames = [crowd_poses(fr.NI), crowd_poses(fr.NI, shift=0.5)[::-1].copy()]
    want = [fr.expect(p, oracle) for p in frames]
    assert want[0]["sockets"].tobytes() != want[1]["sockets"].tobytes()

    def check(got, w, what):
        for k in ("palettes", "sockets", "prop_palettes", "positions", "normals"):
            gu.assert_bits_equal(got[k].view(F).reshape(w[k].shape), w[k], f"{what}: {k}")
    try:
        with hs.Stream() as S:
            try:
                fr.dm.set_stream(S.ptr)
                fr.pm.set_stream(S.ptr)
                fr.d_poses.upload(frames[1])
                fr.fill()
                fr.frame()                                    # sizes every scratch; on S alone
                S.synchronize()
                check(fr.read("direct on the borrowed stream"), want[1], "direct on the borrowed stream")
                fr.fill()
                fr.dm.graph_begin()
                try:
                    assert S.capture_status() == hs.CAPTURE_ACTIVE
                    fr.frame()
                    assert S.capture_status() == hs.CAPTURE_ACTIVE
                finally:
                    graph = fr.dm.graph_end()
                try:
                    device_synchronize()
                    for k, raw in fr.read("after the recording").items():
                        assert (raw == SENT).all(), f"output {k} was written although the calls were only recorded"
                    for k, poses in enumerate(frames):
                        fr.d_poses.upload(poses)
                        fr.fill()
                        graph.launch()
                        S.synchronize()
                        check(fr.read(f"replay {k + 1}"), want[k], f"replay {k + 1}")
                finally:
                    graph.close()
            finally:
                fr.dm.set_stream(None)
                fr.pm.set_stream(None)
    finally:
        fr.close()

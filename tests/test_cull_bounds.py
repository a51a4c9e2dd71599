"""Culling and LOD on the device (mmdx_cull_bounds): the boxes of mmdx_deform_batched_bounds against up to 16 planes and up to 3
distances, compacted into up to 4 instance lists in ascending instance order -- the lists mmdx_deform_batched_select takes.
The contract is a stated float32 arithmetic (include/mmdx.h); cull_ref() below restates it in numpy, every operation on np.float32,
and lists, counts and levels are compared with NO tolerance.
CPU: the ABI (header, struct layout against the header, exports, binding), mmdx_cull_planes_from_matrix bit for bit, the planner
(tests/cull_shape_driver.cpp under ASan + UBSan), host-side validation on a host-only handle (so provably before any device call),
the new kernels' resources.
GPU: synthetic bounds uploaded from numpy; both forms and both extreme chunk sizes forced, each call's form and chunk count proved
with mmdx_debug_last_launch_shape.

A note on NaN bounds.  The arithmetic decides, and it says: a plane culls when s < 0, and s is NaN exactly when the corner that the
plane's signs select holds a NaN (or the plane does); a NaN on one side of one axis leaves the other side's subtraction in m(a, b).
So a row that is NaN THROUGHOUT (a row never written) is never culled and has level 0 (d2 = 0 for positive distances), which is
asserted outright; a row with ONE NaN component is only exempt from the planes that read that component, and its level follows
from the remaining components -- those rows are held to the restatement, bit for bit, like everything else."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from simple_mmd_renderer_amd import _capi as api
from simple_mmd_renderer_amd import synth
from simple_mmd_renderer_amd.engine import DeformModel, DeviceBuffer, device_count, make_cull_view, planes_from_matrix
from tests import host_program as hp
from tests.host_program import ROOT

HEADER = os.path.join(ROOT, "include", "mmdx.h")
BENCH_HEADER = os.path.join(ROOT, "include", "mmdx_bench.h")
F = np.float32
INVALID, NO_DEVICE = 1, 3
SENT = 0xEEEEEEEE          # what every output word holds before a call
TAIL = 8                   # sentinel words behind every output array
CROSSOVER = 4096           # cull_shape.hpp kCullCrossover


# ---- the restatement -------------------------------------------------------------------------------------------------------------
def cull_ref(bounds, planes, n_planes, n_lods, eye, margin, lod_distance, clamp=False):
    """include/mmdx.h, "The arithmetic", in numpy float32: (lists[4], levels[NI] with CULLED).  clamp: a device view's counts."""
    b = np.asarray(bounds, F).reshape(-1, 6)
    planes = np.asarray(planes, F).reshape(-1, 4)
    if clamp:
        n_planes, n_lods = min(n_planes, 16), min(max(n_lods, 1), 4)
    mn, mx = b[:, :3], b[:, 3:]
    margin, eye, zero = F(margin), np.asarray(eye, F), F(0)
    m = lambda x, y: np.where(x > y, x, y)
    with np.errstate(all="ignore"):
        lo, hi = mn - margin, mx + margin
        culled = np.zeros(len(b), bool)
        for p in range(n_planes):
            a, bb, c, d = planes[p]
            px = hi[:, 0] if a >= 0 else lo[:, 0]
            py = hi[:, 1] if bb >= 0 else lo[:, 1]
            pz = hi[:, 2] if c >= 0 else lo[:, 2]
            s = ((a * px + bb * py) + c * pz) + d
            assert s.dtype == F
            culled |= s < 0
        dx = m(m(mn[:, 0] - eye[0], eye[0] - mx[:, 0]), zero)
        dy = m(m(mn[:, 1] - eye[1], eye[1] - mx[:, 1]), zero)
        dz = m(m(mn[:, 2] - eye[2], eye[2] - mx[:, 2]), zero)
        d2 = (dx * dx + dy * dy) + dz * dz
        assert d2.dtype == F
        level = np.zeros(len(b), np.uint32)
        for k in range(n_lods - 1):
            t = F(lod_distance[k])
            level += (d2 >= t * t).astype(np.uint32)
    levels = np.where(culled, np.uint32(api.CULLED), level).astype(np.uint32)
    lists = [np.nonzero(~culled & (level == l))[0].astype(np.uint32) if l < n_lods else np.zeros(0, np.uint32) for l in range(4)]
    return lists, levels


class View:
    """One mmdx_cull_view as plain arrays (16 plane slots, 3 distance slots always filled) + the counts written into it."""

    def __init__(self, planes, n_planes, n_lods, eye, margin, lod):
        self.planes = np.zeros((16, 4), F)
        pl = np.asarray(planes, F).reshape(-1, 4)
        self.planes[:len(pl)] = pl
        self.n_planes, self.n_lods, self.eye, self.margin = n_planes, n_lods, np.asarray(eye, F), F(margin)
        self.lod = np.asarray(lod, F)
        assert self.lod.shape == (3,)

    def struct(self):
        return make_cull_view(self.planes, self.eye, self.lod, float(self.margin), n_planes=self.n_planes, n_lods=self.n_lods)

    def ref(self, bounds, clamp):
        return cull_ref(bounds, self.planes, self.n_planes, self.n_lods, self.eye, self.margin, self.lod, clamp)


# ---- matrices (column-major, element (r, c) at m[c*4+r]; right-handed, depth 0..1 unless said: what the reference builds) ---------------
def perspective(fov_deg, aspect, near, far, zero_to_one=True):
    m = np.zeros(16, F)
    cot = 1.0 / np.tan(np.radians(fov_deg) / 2)
    m[0], m[5], m[11] = cot / aspect, cot, -1.0
    if zero_to_one:
        m[10], m[14] = far / (near - far), near * far / (near - far)
    else:
        m[10], m[14] = (near + far) / (near - far), 2 * near * far / (near - far)
    return m


def orthographic(l, r, b, t, near, far, zero_to_one=True):
    m = np.zeros(16, F)
    m[0], m[5], m[15] = 2 / (r - l), 2 / (t - b), 1.0
    m[12], m[13] = (l + r) / (l - r), (b + t) / (b - t)
    if zero_to_one:
        m[10], m[14] = 1 / (near - far), near / (near - far)
    else:
        m[10], m[14] = 2 / (near - far), (far + near) / (near - far)
    return m


def look_at(eye, target, up=(0, 1, 0)):
    eye, target, up = (np.asarray(x, np.float64) for x in (eye, target, up))
    f = target - eye
    f /= np.linalg.norm(f)
    s = np.cross(f, up)
    s /= np.linalg.norm(s)
    u = np.cross(s, f)
    m = np.eye(4)
    m[0, :3], m[1, :3], m[2, :3] = s, u, -f
    m[:3, 3] = [-s @ eye, -u @ eye, f @ eye]
    return m.T.astype(F).reshape(16)            # rows of m.T are the columns: column-major flat


def mat_mul(a, b):
    """a * b of two column-major flat matrices, in float32"""
    A, B = a.reshape(4, 4).T, b.reshape(4, 4).T
    return (A @ B).astype(F).T.reshape(16)


def planes_ref(m, zero_to_one):
    m = np.asarray(m, F)
    row = [np.array([m[r], m[4 + r], m[8 + r], m[12 + r]], F) for r in range(4)]
    return np.stack([row[3] + row[0], row[3] - row[0], row[3] + row[1], row[3] - row[1],
                     row[2] if zero_to_one else row[3] + row[2], row[3] - row[2]]).astype(F)


EYE = (0.0, 5.0, 40.0)
VIEWPROJ = mat_mul(perspective(50.0, 16 / 9, 0.1, 1000.0), look_at(EYE, (0, 5, 0)))


def frustum_view(n_planes, n_lods, margin=0.0, seed=77):
    """The camera's six planes first, then seeded planes that keep a ball of radius 25 around the origin."""
    rng = np.random.default_rng(seed)
    n = rng.normal(size=(10, 3))
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    extra = np.concatenate([n, np.full((10, 1), 25.0)], axis=1).astype(F)
    planes = np.concatenate([planes_ref(VIEWPROJ, True), extra])
    return View(planes, n_planes, n_lods, EYE, margin, (30.0, 45.0, 70.0))


def scene(ni, seed=4100):
    """Seeded boxes around the origin: many straddle the camera's planes, the LOD rings cut through the crowd."""
    rng = np.random.default_rng(seed + ni)
    c = rng.uniform(-30, 30, (ni, 3))
    h = rng.uniform(0, 3, (ni, 3))
    return np.concatenate([c - h, c + h], axis=1).astype(F)


# ---- CPU: the ABI ----------------------------------------------------------------------------------------------------------------
def _defines(text):
    return {k: int(v.rstrip("u"), 0) for k, v in re.findall(r"#define\s+(MMDX_CULL\w+|MMDX_CULLED)\s+(\w+)", text)}


def _layout(text, name):
    """{field: offset} and the size of `typedef struct name {...} name;` from the header's own declarations (LP64 rules)."""
    body = re.search(r"typedef\s+struct\s+%s\s*\{(.*?)\}\s*%s\s*;" % (name, name), text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    defs = _defines(text)
    off, align_max, out = 0, 1, {}
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        mt = re.match(r"(const\s+)?(\w+)\s*(.*)$", decl, re.S)
        base, rest = mt.group(2), mt.group(3)
        for item in (x.strip() for x in rest.split(",")):
            ptr = item.startswith("*")
            ident = re.match(r"\*?\s*(\w+)", item).group(1)
            count = 1
            for dim in re.findall(r"\[([^\]]+)\]", item):
                count *= eval(dim, {}, defs)
            size = 8 if ptr else {"float": 4, "uint32_t": 4}[base]
            off = (off + size - 1) // size * size
            out[ident] = off
            off += size * count
            align_max = max(align_max, size)
    return out, (off + align_max - 1) // align_max * align_max


def test_header_declares_cull_and_library_exports_it(hip_lib):
    text = open(HEADER).read()
    assert _defines(text) == {"MMDX_CULL_MAX_PLANES": 16, "MMDX_CULL_MAX_LODS": 4, "MMDX_CULLED": 0xFFFFFFFF}
    assert re.search(r"MMDX_CULL_VIEW_ON_DEVICE\s*=\s*1u\s*<<\s*0", text)
    assert re.search(r"MMDX_API\s+mmdx_status\s+mmdx_cull_bounds\s*\(\s*mmdx_model_t\s+model\s*,\s*const\s+mmdx_cull_args\s*\*\s*args\s*\)", text)
    assert re.search(r"MMDX_API\s+mmdx_status\s+mmdx_cull_planes_from_matrix\s*\(\s*const\s+float\s+m\[16\]\s*,\s*uint32_t\s+"
                     r"depth_zero_to_one\s*,\s*float\s+out_planes\[6\]\[4\]\s*\)", text)
    assert "#define MMDX_ABI_VERSION 3u" in text and hip_lib.mmdx_abi_version() == 3 == api.ABI_VERSION
    # the lists are what the select call takes: said where an adopter reads it
    assert re.search(r"mmdx_instance_select\.ids\s*/\s*\.count", text)
    for name in ("mmdx_cull_bounds", "mmdx_cull_planes_from_matrix"):
        assert hasattr(hip_lib, name) and name in api.SIGNATURES
    from tests.test_capi_symbols import declared_symbols
    assert sorted(api.SIGNATURES) == declared_symbols()
    assert re.search(r"MMDX_DEBUG_KERNEL_CULL\s*=\s*4", open(BENCH_HEADER).read()) and api.DEBUG_KERNELS[4] == "cull"
    assert (api.CULL_MAX_PLANES, api.CULL_MAX_LODS, api.CULLED, api.CULL_VIEW_ON_DEVICE) == (16, 4, 0xFFFFFFFF, 1)


def test_struct_layouts_match_the_header():
    text = open(HEADER).read()
    for name, cls in (("mmdx_cull_view", api.CullView), ("mmdx_cull_args", api.CullArgs)):
        offsets, size = _layout(text, name)
        assert list(offsets) == [f for f, _ in cls._fields_], name
        assert {f: getattr(cls, f).offset for f, _ in cls._fields_} == offsets, name
        assert C.sizeof(cls) == size, name
    assert C.sizeof(api.CullView) == 296 and C.sizeof(api.CullArgs) == 56
    assert api.CullView.n_planes.offset == 256 and api.CullView.lod_distance.offset == 280


# ---- CPU: planes from a matrix ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("zero_to_one", [True, False], ids=["depth-0-1", "depth-minus1-1"])
def test_planes_from_matrix_bit_for_bit(hip_lib, zero_to_one):
    light = mat_mul(orthographic(-5, 5, -5, 5, 0.1, 100.0, zero_to_one), look_at((3, 10, 4), (0, 0, 0)))      # the 5 m light box
    cam = mat_mul(perspective(50.0, 16 / 9, 0.1, 1000.0, zero_to_one), look_at(EYE, (1, 5, -2)))
    rng = np.random.default_rng(5)
    for m in (cam, light, rng.normal(size=16).astype(F)):
        got = planes_from_matrix(m, zero_to_one)
        assert got.dtype == F and got.shape == (6, 4)
        assert np.array_equal(got.view(np.uint32), planes_ref(m, zero_to_one).view(np.uint32))
    # what the planes mean: a point well inside the camera's view is inside all six, one behind the camera is not
    pl = planes_from_matrix(cam, zero_to_one).astype(np.float64)
    inside = lambda p: bool((pl[:, :3] @ np.asarray(p, np.float64) + pl[:, 3] >= 0).all())
    assert inside((1, 5, -2)) and not inside((0, 5, 80)) and not inside((500, 5, 0))
    assert hip_lib.mmdx_cull_planes_from_matrix(None, 0, None) == INVALID


# ---- CPU: the planner ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def driver():
    return hp.build("cull_shape_driver", [os.path.join(hp.TESTS, "cull_shape_driver.cpp"), os.path.join(hp.CSRC, "cull_shape.cpp")],
                    opt="-O1", sanitize=True)


def plan_ref(ni, form, chunk):
    f = form if form in (1, 2) else (1 if ni <= CROSSOVER else 2)
    ch = (1024 if f == 1 else 256) if chunk <= 0 else min(max(chunk // 64 * 64, 64), 1024)
    n = max(1, -(-ni // ch))
    return dict(form=f, chunk=ch, threads=ch, nchunks=n, scratch=n * 16 if f == 2 else 0)


def test_planner_sweep_under_sanitizers(driver):
    r = hp.run(driver, ["sweep"])
    assert r.returncode == 0, r.stdout + r.stderr
    counts = dict(kv.split("=") for kv in r.stdout.split())
    assert int(counts["failures"]) == 0 and "ERROR" not in r.stderr
    assert int(counts["rows"]) == 18 * 5 * 16


def test_planner_form_chunk_and_chunk_count(driver):
    """Form by NI (the crossover and its neighbours), forced forms, chunk clamping, chunk count: against this file's own statement."""
    nis = [0, 1, 63, 64, 65, 200, 1023, 1025, 2500, CROSSOVER - 1, CROSSOVER, CROSSOVER + 1, 16384, 262144, 2 ** 32 - 1]
    cases = [(ni, form, chunk) for ni in nis for form in (0, 1, 2, 7) for chunk in (0, -3, 1, 64, 100, 128, 1000, 1024, 1025, 99999)]
    r = hp.run(driver, ["eval"], stdin="".join("%d %d %d\n" % c for c in cases))
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert len(lines) == len(cases)
    for case, line in zip(cases, lines):
        got = {k: int(v) for k, v in (kv.split("=") for kv in line.split())}
        assert got == plan_ref(*case), case
    # spot checks spelled out
    assert plan_ref(4096, 0, 0)["form"] == 1 and plan_ref(4097, 0, 0) == dict(form=2, chunk=256, threads=256, nchunks=17, scratch=272)
    assert plan_ref(0, 2, 64) == dict(form=2, chunk=64, threads=64, nchunks=1, scratch=16)


# ---- CPU: validation happens on the host, before any device call -------------------------------------------------------------------
def _args(view, ni=10, stride=None, flags=0, bounds=0x1000, ids=0x2000, counts=0x3000, levels=0x4000):
    a = api.CullArgs()
    a.struct_size, a.flags, a.n_instances, a.list_stride = C.sizeof(api.CullArgs), flags, ni, ni if stride is None else stride
    a.bounds, a.out_ids, a.out_counts, a.out_levels = bounds, ids, counts, levels
    a.view = C.addressof(view) if isinstance(view, api.CullView) else view
    return a


def test_host_validation_precedes_any_device_call(hip_lib):
    """A host-only handle has no device: a call that passes validation answers MMDX_ERR_NO_DEVICE, every rejected argument
    MMDX_ERR_INVALID_ARGUMENT -- so the rejection cannot depend on a device call.  (The pointers are never dereferenced.)"""
    good = lambda **kw: make_cull_view([[1, 0, 0, 0]], (0, 0, 0), (1.0, 2.0, 3.0), **kw)
    nan = float("nan")
    with DeformModel(synth.make_model(64, 3, 0, 0, seed=1), host_only=True) as dm:
        call = lambda a: hip_lib.mmdx_cull_bounds(dm.h, C.byref(a))
        v = good()
        assert call(_args(v)) == NO_DEVICE
        assert call(_args(v, ni=0, bounds=None, ids=None)) == NO_DEVICE                 # an empty crowd is a valid call
        assert call(_args(good(n_planes=0, n_lods=1))) == NO_DEVICE
        assert call(_args(make_cull_view([], (0, 0, 0), (2.0, 2.0, 5.0)))) == NO_DEVICE   # equal distances ascend
        assert call(_args(make_cull_view([], (0, 0, 0), (3.0, nan), n_lods=2))) == NO_DEVICE   # ... and only n_lods-1 are read
        bad_views = {
            "n_planes 17": good(n_planes=17), "n_lods 0": good(n_lods=0), "n_lods 5": good(n_lods=5),
            "margin < 0": good(margin=-0.5), "margin NaN": good(margin=nan),
            "descending": make_cull_view([], (0, 0, 0), (1.0, 3.0, 2.0)), "NaN distance": make_cull_view([], (0, 0, 0), (1.0, nan, 2.0)),
        }
        for what, bv in bad_views.items():
            assert call(_args(bv)) == INVALID, what
            assert hip_lib.mmdx_last_error_string()
            # the same structure behind the device flag cannot be read by the host: it passes validation
            assert call(_args(bv, flags=api.CULL_VIEW_ON_DEVICE)) == NO_DEVICE, what
        r0 = good()
        r0.reserved0 = 1
        assert call(_args(r0)) == INVALID
        assert call(_args(v, ni=10, stride=9)) == INVALID
        assert call(_args(v, flags=2)) == INVALID and call(_args(v, flags=0x80000001)) == INVALID
        for null in ("bounds", "ids", "counts"):
            assert call(_args(v, **{null: None})) == INVALID, null
        assert call(_args(None)) == INVALID
        assert call(_args(v, levels=None)) == NO_DEVICE                                  # out_levels is optional
        assert call(_args(v, bounds=0x1002)) == INVALID and call(_args(v, levels=0x4001)) == INVALID
        short = _args(v)
        short.struct_size -= 8
        assert call(short) == INVALID
        assert hip_lib.mmdx_cull_bounds(None, C.byref(_args(v))) == INVALID and hip_lib.mmdx_cull_bounds(dm.h, None) == INVALID


# ---- CPU: the kernels' resources -------------------------------------------------------------------------------------------------
def test_cull_kernels_have_no_spills_and_no_scratch(hip_lib):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), api.LIB_PATH, "cull_"],
                         capture_output=True, text=True, check=True).stdout.splitlines()
    names = {l.split()[0] for l in out}
    assert names == {k + v for k in ("cull_walk_kernel", "cull_count_kernel", "cull_scatter_kernel") for v in ("<true>", "<false>")}, out
    for l in out:
        m = re.search(r"spill\s+(\S+)\s+scratch\s+(\S+)\s+lds\s+(\S+)", l)
        assert m and m.group(1) == "0" and m.group(2) == "0" and int(m.group(3)) <= 1024, l


# ---- GPU -------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dm(hip_lib):
    assert device_count() >= 1, "no HIP device visible: the GPU tests must run on the MI355X box"
    with DeformModel(synth.make_model(64, 3, 0, 0, seed=1)) as model:         # the handle: stream, scratch, launch-shape record
        yield model


@pytest.fixture
def cull_env(hip_lib, monkeypatch):
    """MMDX_CULL_FORM / MMDX_CULL_CHUNK for one test; the library re-reads them on request."""
    def _set(form=None, chunk=None):
        for k, v in (("MMDX_CULL_FORM", form), ("MMDX_CULL_CHUNK", chunk)):
            if v is None:
                monkeypatch.delenv(k, raising=False)
            else:
                monkeypatch.setenv(k, str(v))
        hip_lib.mmdx_debug_reload_env()
    yield _set
    monkeypatch.delenv("MMDX_CULL_FORM", raising=False)
    monkeypatch.delenv("MMDX_CULL_CHUNK", raising=False)
    hip_lib.mmdx_debug_reload_env()


def run_cull(dm, bounds, view, on_device, stride=None, levels=True, shape=None):
    """One call into sentinel-filled arrays; returns (ids [4*stride + TAIL], counts [4 + TAIL], levels [ni + TAIL] or None).
    shape = (form, chunk): proved with mmdx_debug_last_launch_shape."""
    bounds = np.ascontiguousarray(bounds, F).reshape(-1, 6)
    ni = len(bounds)
    stride = ni if stride is None else stride
    d_b = DeviceBuffer.from_numpy(bounds if ni else np.zeros(6, F))
    d_ids = DeviceBuffer.from_numpy(np.full(4 * stride + TAIL, SENT, np.uint32))
    d_cnt = DeviceBuffer.from_numpy(np.full(4 + TAIL, SENT, np.uint32))
    d_lvl = DeviceBuffer.from_numpy(np.full(ni + TAIL, SENT, np.uint32)) if levels else None
    st = view.struct()
    d_view = DeviceBuffer.from_numpy(np.frombuffer(bytes(st), np.uint8)) if on_device else None
    dm.cull_bounds(d_b, d_view if on_device else st, ni, d_ids, d_cnt, d_lvl, stride)
    if shape is not None:
        form, chunk = shape
        s = dm.last_launch_shape()
        assert (s["kernel"], s["select"], s["group"], s["threads"], s["ngroups"]) == ("cull", form, chunk, chunk, max(1, -(-ni // chunk))), s
    dm.sync()
    out = (d_ids.download((4 * stride + TAIL,), np.uint32), d_cnt.download((4 + TAIL,), np.uint32),
           d_lvl.download((ni + TAIL,), np.uint32) if levels else None)
    for x in (d_b, d_ids, d_cnt, d_lvl, d_view):
        if x is not None:
            x.free()
    return out


def check(got, ref, ni, stride, n_lods, what):
    """Lists, counts and levels equal the restatement; every other word still holds its sentinel."""
    ids, counts, levels = got
    lists, ref_levels = ref
    stride = ni if stride is None else stride
    want_counts = [len(lists[l]) if l < n_lods else 0 for l in range(4)]
    assert counts[:4].tolist() == want_counts, f"{what}: counts {counts[:4].tolist()} != {want_counts}"
    assert (counts[4:] == SENT).all(), f"{what}: words behind out_counts[4] written"
    expect = np.full_like(ids, SENT)
    for l in range(n_lods):
        expect[l * stride: l * stride + len(lists[l])] = lists[l]
    bad = np.nonzero(ids != expect)[0]
    assert not bad.size, f"{what}: out_ids differs at words {bad[:8].tolist()} (got {ids[bad[:8]].tolist()}, want {expect[bad[:8]].tolist()})"
    if levels is not None:
        assert np.array_equal(levels[:ni], ref_levels), f"{what}: levels differ at {np.nonzero(levels[:ni] != ref_levels)[0][:8].tolist()}"
        assert (levels[ni:] == SENT).all(), f"{what}: words behind out_levels[ni] written"


SWEEP_NI = (0, 1, 63, 64, 65, 200, 1023, 1025, 2500)


@pytest.mark.gpu
@pytest.mark.parametrize("chunk", [64, 1024])
@pytest.mark.parametrize("form", [1, 2])
def test_shape_sweep(dm, cull_env, form, chunk):
    """Every crowd size of the sweep with both forms and both extreme chunk sizes forced: at chunk 64 that is up to 40 chunks with
    running bases, partial last waves (63, 65, 200, 1023, 1025, 2500) and -- with the far LOD ring nearly empty -- chunks without
    a survivor of a level.  A host view (6 planes, 3 lists) and a device view (16 planes, 4 lists) each."""
    cull_env(form, chunk)
    hv, dv = frustum_view(6, 3), frustum_view(16, 4)
    for ni in SWEEP_NI:
        b = scene(ni)
        for view, on_device in ((hv, False), (dv, True)):
            got = run_cull(dm, b, view, on_device, shape=(form, chunk))
            check(got, view.ref(b, on_device), ni, None, view.n_lods, f"form {form} chunk {chunk} ni {ni} {'device' if on_device else 'host'} view")
    # the sweep means something: the big crowd has survivors and victims in every list, and some 64-chunk lacks a level
    lists, levels = dv.ref(scene(2500), True)
    assert all(len(l) > 0 for l in lists) and (levels == api.CULLED).sum() > 100
    per_chunk = [set(levels[k:k + 64].tolist()) for k in range(0, 2500, 64)]
    assert any(3 not in s for s in per_chunk) and any(3 in s for s in per_chunk)


@pytest.mark.gpu
def test_planner_defaults_on_the_device(dm, cull_env):
    """Without overrides: one workgroup of 1024 lanes up to the crossover, 256-instance chunks in two launches above it."""
    cull_env()
    v = frustum_view(6, 2)
    for ni, shape in ((CROSSOVER, (1, 1024)), (CROSSOVER + 1, (2, 256))):
        b = scene(ni)
        check(run_cull(dm, b, v, True, shape=shape), v.ref(b, True), ni, None, 2, f"default shape ni {ni}")


@pytest.mark.gpu
@pytest.mark.parametrize("on_device", [False, True], ids=["host-view", "device-view"])
def test_views(dm, cull_env, on_device):
    """0, 1, 6 and 16 planes x 1..4 lists, with and without a margin; forms as the planner picks them, chunk 128 (several waves,
    several chunks)."""
    cull_env(None, 128)
    b = scene(700)
    for n_planes in (0, 1, 6, 16):
        for n_lods in (1, 2, 3, 4):
            view = frustum_view(n_planes, n_lods, margin=0.0 if n_lods % 2 else 1.5)
            check(run_cull(dm, b, view, on_device, shape=(1, 128)), view.ref(b, on_device), 700, None, n_lods,
                  f"{n_planes} planes {n_lods} lods")
    lists, levels = frustum_view(0, 1).ref(b, False)
    assert len(lists[0]) == 700                                   # no plane: nothing is culled


AXIS = dict(planes=[[1, 0, 0, -2]], n_planes=1, n_lods=4, eye=(0, 0, 0), lod=(5.0, 10.0, 20.0))      # visible: x >= 2
below = lambda x: float(np.nextafter(F(x), F(0)))
EDGE_ROWS = np.array([
    [1, -1, -1, 2, 1, 1],                  # 0 max.x exactly on the plane: s == 0 stays; d2 = 1
    [1, -1, -1, below(2), 1, 1],           # 1 one ulp short of it: culled
    [0, -1, -1, 4, 1, 1],                  # 2 straddles the plane, holds the eye's x: level 0
    [5, -1, -1, 6, 1, 1],                  # 3 exactly at the first distance: d2 == 25 >= 25, level 1
    [below(5), -1, -1, 6, 1, 1],           # 4 one ulp nearer: level 0
    [10, 0, 0, 10, 0, 0],                  # 5 a zero-size box at the second distance: level 2
    [2, 0, 0, 2, 0, 0],                    # 6 a zero-size box on the plane: stays, level 0
    [-1, -1, -1, 3, 1, 1],                 # 7 holds the eye: d2 == 0, level 0
    [20, 0, 0, 21, 0, 0],                  # 8 at the third distance: level 3
    [3, 3, 4, 4, 4, 5],                    # 9 d2 = 9 + 9 + 16 = 34: level 1
    [-9, -1, -1, -8, 1, 1],                # 10 wholly outside: culled
], F)
EDGE_LEVELS = [0, api.CULLED, 0, 1, 0, 2, 0, 0, 3, 1, api.CULLED]


@pytest.mark.gpu
@pytest.mark.parametrize("form", [1, 2])
def test_boxes_on_planes_and_at_distances(dm, cull_env, form):
    cull_env(form, 64)
    # the restatement itself first: the rows mean what their comments say
    view = View(margin=0.0, **AXIS)
    lists, levels = view.ref(EDGE_ROWS, False)
    assert levels.tolist() == EDGE_LEVELS
    reps = np.tile(EDGE_ROWS, (13, 1))                          # 143 rows: the edge rows in every lane position of three waves
    for on_device in (False, True):
        check(run_cull(dm, reps, view, on_device, shape=(form, 64)), view.ref(reps, on_device), len(reps), None, 4, "edge rows")
    # the margin grows the box for the planes only: row 1 and nothing else comes back, no level moves
    grown = View(margin=0.5, **AXIS)
    want = list(EDGE_LEVELS)
    want[1] = 0
    assert grown.ref(EDGE_ROWS, False)[1].tolist() == want
    check(run_cull(dm, reps, grown, True), grown.ref(reps, True), len(reps), None, 4, "edge rows with a margin")
    # a first distance of 0: d2 == 0 reaches it (>=)
    zero = View(planes=[], n_planes=0, n_lods=2, eye=(0, 0, 0), margin=0.0, lod=(0.0, 0.0, 0.0))
    assert zero.ref(EDGE_ROWS, False)[1].tolist() == [1] * len(EDGE_ROWS)
    check(run_cull(dm, EDGE_ROWS, zero, False), zero.ref(EDGE_ROWS, False), len(EDGE_ROWS), None, 2, "distance 0")


@pytest.mark.gpu
@pytest.mark.parametrize("form", [1, 2])
def test_nan_and_inf(dm, cull_env, form):
    """See the note at the top of the file: rows that are NaN throughout are never culled and have level 0; one NaN component, +-inf
    bounds and NaN planes follow the arithmetic, bit for bit."""
    cull_env(form, 64)
    nan, inf = np.nan, np.inf
    base = scene(80, seed=99)
    rows = []
    for src in (base[3], base[17], EDGE_ROWS[10], EDGE_ROWS[8]):          # visible and culled rows, near and far
        for k in range(6):
            r = src.copy()
            r[k] = nan
            rows.append(r)
    n_single = len(rows)
    rows += [np.full(6, nan, F)] * 3
    rows += [np.array(r, F) for r in ([-inf, -inf, -inf, inf, inf, inf], [inf, inf, inf, inf, inf, inf], [-inf] * 6,
                                      [-inf, 0, 0, 1, 1, 1], [0, 0, 0, 1, inf, 1], [inf, 0, 0, -inf, 1, 1], [3, 0, 0, 4, 1, nan])]
    b = np.concatenate([base, np.array(rows, F)])
    all_nan = slice(80 + n_single, 80 + n_single + 3)
    views = [frustum_view(16, 4), frustum_view(6, 3, margin=2.0), View(margin=0.0, **AXIS)]
    nan_plane = frustum_view(16, 4)
    nan_plane.planes[2, 1] = nan                                      # one NaN coefficient: that plane culls nothing
    nan_plane.planes[9] = nan
    views.append(nan_plane)
    for vi, view in enumerate(views):
        for on_device in (False, True):
            ref = view.ref(b, on_device)
            assert (ref[1][all_nan] == 0).all()                       # never culled, level 0
            got = run_cull(dm, b, view, on_device, shape=(form, 64))
            check(got, ref, len(b), None, view.n_lods, f"NaN / inf rows, view {vi}")
            assert (got[2][:len(b)][all_nan] == 0).all()
    # a view whose every plane is NaN culls nothing at all
    blind = frustum_view(6, 1)
    blind.planes[:6, 3] = nan
    got = run_cull(dm, b, blind, True)
    check(got, blind.ref(b, True), len(b), None, 1, "NaN planes")
    assert got[1][0] == len(b)
    # a NaN margin and a negative one in a device view act as the arithmetic says (a host view would be rejected)
    for margin in (nan, -1.0):
        odd = frustum_view(6, 2, margin=margin)
        check(run_cull(dm, b, odd, True), odd.ref(b, True), len(b), None, 2, f"margin {margin}")


@pytest.mark.gpu
@pytest.mark.parametrize("form", [1, 2])
def test_all_culled_all_visible_sentinels_stride_and_no_levels(dm, cull_env, form):
    cull_env(form, 64)
    ni = 333
    b = scene(ni)
    none = View(planes=[[0, 0, 0, -1]], n_planes=1, n_lods=3, eye=EYE, margin=0.0, lod=(30.0, 45.0, 60.0))
    every = View(planes=[[0, 0, 0, 1]], n_planes=1, n_lods=3, eye=EYE, margin=0.0, lod=(30.0, 45.0, 60.0))
    got = run_cull(dm, b, none, True, shape=(form, 64))
    check(got, none.ref(b, True), ni, None, 3, "all culled")
    assert got[1][:4].tolist() == [0, 0, 0, 0] and (got[0] == SENT).all() and (got[2][:ni] == api.CULLED).all()
    got = run_cull(dm, b, every, False, shape=(form, 64))
    check(got, every.ref(b, False), ni, None, 3, "all visible")
    assert got[1][:3].sum() == ni and got[1][3] == 0
    # list_stride > NI: the gap between the lists keeps its sentinel (check() compares every word); out_levels == NULL works
    v = frustum_view(6, 4)
    for stride in (ni + 1, ni + 77):
        check(run_cull(dm, b, v, True, stride=stride), v.ref(b, True), ni, stride, 4, f"stride {stride}")
    got = run_cull(dm, b, v, False, levels=False, shape=(form, 64))
    check(got, v.ref(b, False), ni, None, 4, "without out_levels")


@pytest.mark.gpu
@pytest.mark.parametrize("form", [1, 2])
def test_device_view_out_of_range_clamps_and_calls_are_deterministic(dm, cull_env, form):
    cull_env(form, 64)
    b = scene(500)
    wild = frustum_view(40, 9)                   # n_planes = 40 acts as 16, n_lods = 9 as 4
    ref = wild.ref(b, True)
    assert [len(l) for l in ref[0]] == [len(l) for l in frustum_view(16, 4).ref(b, True)[0]]
    first = run_cull(dm, b, wild, True, shape=(form, 64))
    check(first, ref, 500, None, 4, "n_planes 40, n_lods 9")
    none = frustum_view(6, 0)                    # n_lods = 0 acts as 1
    check(run_cull(dm, b, none, True), none.ref(b, True), 500, None, 1, "n_lods 0")
    second = run_cull(dm, b, wild, True)
    for x, y in zip(first, second):
        assert np.array_equal(x, y)

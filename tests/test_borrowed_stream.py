"""mmdx_model_set_stream: the renderer's own HIP stream under every entry point that takes its stream from the model.

CPU: the refusals that need no device, and the Python wrapper.
GPU 1 (test_family_queues_on_the_borrowed_stream_only): for every call family, with every operand in device memory, the library's
      own recorder is the witness.  The call runs eagerly on the handle's own stream (the expected bits W; the deform families and
      the FK solve also against the oracle, the others are pinned to their restatements at these shapes by their own tests), then
      eagerly on a borrowed stream S, then between mmdx_graph_begin and mmdx_graph_end with S capturing.  After the recording and a
      device-wide synchronisation every output byte must still hold its sentinel: anything that was enqueued on another stream
      than S -- the own stream, the null stream -- would have run by then.  The replay must then give W, the 256 sentinel bytes on
      both sides of every output untouched, and so must the eager call after mmdx_model_set_stream(NULL).
      The deform sweep runs on synth.make_model(nv, 17, 6, 60) for nv = 1000 and nv = 4099 (nine tiles, the last of three
      vertices), 21 instances.
GPU 2: the host-operand forms on a borrowed stream hold the own-stream / oracle bits at the moment they return.
GPU 3: a switch orders the new stream behind the old one, without ever blocking the host (gates: tests/hip_stream_util.py).
GPU 4: misuse -- a switch while recording, a switch to the current stream, a stream of another device.
(Destroying a borrowed stream that is still in use is undefined by contract and not tested.)"""
import ctypes as C

import numpy as np
import pytest

from simple_mmd_renderer_amd import _capi as api
from simple_mmd_renderer_amd import synth, vmd
from simple_mmd_renderer_amd.engine import DeformModel, DeviceBuffer, device_count, device_select, device_synchronize, make_cull_view
from tests import golden_util as gu
from tests import hip_stream_util as hs

F = np.float32
INVALID, NO_DEVICE = 1, 3
SENT = 0xEE                     # every output byte before a call
GUARD = 256                     # sentinel bytes in front of and behind every output (keeps the outputs' alignment)
DEV = api.PALETTE_ON_DEVICE | api.WEIGHTS_ON_DEVICE | api.OUT_ON_DEVICE
PAL_OUT = api.PALETTE_ON_DEVICE | api.OUT_ON_DEVICE
PLACE_DEV = api.PALETTE_ON_DEVICE | api.PLACE_ON_DEVICE | api.OUT_ON_DEVICE


# ---- CPU -------------------------------------------------------------------------------------------------------------------------
def test_set_stream_refusals_that_need_no_device(hip_lib):
    assert hip_lib.mmdx_model_set_stream(None, None) == INVALID
    assert hip_lib.mmdx_model_set_stream(None, 0x1000) == INVALID
    with DeformModel(synth.make_model(64, 3, 0, 0, seed=1), host_only=True) as dm:
        assert hip_lib.mmdx_model_set_stream(dm.h, None) == NO_DEVICE
        assert hip_lib.mmdx_model_set_stream(dm.h, 0x1000) == NO_DEVICE          # never dereferenced
        assert hip_lib.mmdx_last_error_string()


def test_python_wrapper_exists_and_reports_the_status(hip_lib):
    assert callable(getattr(DeformModel, "set_stream", None))
    with DeformModel(synth.make_model(64, 3, 0, 0, seed=1), host_only=True) as dm:
        for stream in (None, 0x1000, C.c_void_p(0x1000)):
            with pytest.raises(api.MmdxError) as e:
                dm.set_stream(stream)
            assert e.value.status == NO_DEVICE


# ---- GPU: outputs between sentinels ------------------------------------------------------------------------------------------------
class Out:
    """A device output of `nbytes` with GUARD sentinel bytes on both sides; `ptr` is what the library is given."""

    def __init__(self, nbytes):
        self.nbytes = int(nbytes)
        self.buf = DeviceBuffer(self.nbytes + 2 * GUARD)
        self.ptr = self.buf.ptr + GUARD
        self.fill()

    def fill(self):
        self.buf.memset(SENT)

    def read(self, what):
        raw = self.buf.download((self.nbytes + 2 * GUARD,), np.uint8)
        assert (raw[:GUARD] == SENT).all() and (raw[GUARD + self.nbytes:] == SENT).all(), f"{what}: bytes outside the output were written"
        return raw[GUARD:GUARD + self.nbytes].copy()

    def free(self):
        self.buf.free()


def f32(raw, *shape):
    return raw.view(F).reshape(shape)


class Family:
    """One call family: `call()` makes the library calls on `dm`; `outs` are its outputs; `inputs` the DeviceBuffers and handles to
    release.  nan_ok: the family's own test lets NaN match NaN (the CCD-IK of degenerate chains).  check(W): W against the oracle or
    the restatement, where the family has one here.  after_first(): asserted once, after the eager run on the own stream."""

    def __init__(self, dm, outs, call, inputs=(), nan_ok=False, check=None, after_first=None):
        self.dm, self.outs, self.call, self.inputs = dm, outs, call, list(inputs)
        self.nan_ok, self.check, self.after_first = nan_ok, check, after_first

    def fill(self):
        for o in self.outs.values():
            o.fill()

    def read(self, what):
        return {k: o.read(f"{what}: {k}") for k, o in self.outs.items()}

    def assert_equal(self, got, want, what):
        for k in want:
            g, w = got[k], want[k]
            same = g == w
            if self.nan_ok:
                gf, wf = g.view(F), w.view(F)
                same = (g.view(np.uint32) == w.view(np.uint32)) | (np.isnan(gf) & np.isnan(wf))
            bad = np.nonzero(~same)[0]
            assert not bad.size, f"{what}: output {k} differs in {bad.size} of {same.size} places, first at {bad[0]}"

    def assert_untouched(self, what):
        for k, raw in self.read(what).items():
            bad = np.nonzero(raw != SENT)[0]
            assert not bad.size, (f"{what}: {bad.size} bytes of output {k} were written (first at {bad[0]}) although the call was only "
                                  "recorded: something was enqueued on another stream than the model's")

    def close(self):
        for o in self.outs.values():
            o.free()
        for x in self.inputs:
            x.free() if isinstance(x, DeviceBuffer) else x.close()
        self.dm.close()


def sweep(fam, what):
    """Steps 1-7 of the module's docstring for one family."""
    dm = fam.dm
    # 1. eagerly on the own stream: W
    fam.fill()
    fam.call()
    dm.sync()
    W = fam.read(f"{what}, own stream")
    assert any((raw != SENT).any() for raw in W.values()), f"{what}: the call wrote nothing"
    if fam.after_first:
        fam.after_first()
    if fam.check:
        fam.check(W)
    with hs.Stream() as S:
        try:
            # 2. eagerly on S (sizes whatever scratch the call needs): S alone is waited for
            dm.set_stream(S.ptr)
            fam.fill()
            fam.call()
            S.synchronize()
            fam.assert_equal(fam.read(f"{what}, eager on S"), W, f"{what}, eager on the borrowed stream")
            # 3-4. recorded on S
            fam.fill()
            dm.graph_begin()
            try:
                assert S.capture_status() == hs.CAPTURE_ACTIVE, f"{what}: mmdx_graph_begin did not start a capture on the borrowed stream"
                fam.call()
                assert S.capture_status() == hs.CAPTURE_ACTIVE, f"{what}: the recorded call ended or broke the capture"
            finally:
                g = dm.graph_end()
            try:
                assert S.capture_status() == hs.CAPTURE_NONE
                # 5. nothing ran
                device_synchronize()
                fam.assert_untouched(f"{what}, after the recording")
                # 6. the replay, on S
                g.launch()
                S.synchronize()
                fam.assert_equal(fam.read(f"{what}, replay"), W, f"{what}, replay on the borrowed stream")
            finally:
                g.close()
        finally:
            # 7. back on the own stream (also on the way out of a failure: S is about to be destroyed)
            dm.set_stream(None)
        fam.fill()
        fam.call()
        dm.sync()
        assert S.query() == hs.SUCCESS
        fam.assert_equal(fam.read(f"{what}, own stream again"), W, f"{what}, after mmdx_model_set_stream(NULL)")


@pytest.fixture(scope="module")
def gpu(hip_lib):
    assert device_count() >= 1, "no HIP device visible: the GPU tests must run on the MI355X box"
    hs.hip()
    return hip_lib


# ---- GPU 1: the deform families ----------------------------------------------------------------------------------------------------
DEFORM_KINDS = ("per-instance", "shared-pass-twice", "bounds", "select", "frame", "pitched")
SEL_IDS = np.array([3, 20, 0, 7, 11, 12, 19, 1, 2, 4], np.uint32)      # capacity 10 ...
SEL_LIVE = 7                                                             # ... of which the device count says 7 are in use


def deform_family(kind, nv, oracle):
    m = synth.make_model(nv, 17, 6, 60, seed=8800 + nv)
    ni = 1 if kind == "frame" else 21
    frames = np.arange(ni) * 5 + 2
    pals = synth.make_palettes(m, frames)
    shared = kind in ("shared-pass-twice", "select", "frame")
    rates = synth.morph_weights(m.nm, 31)[0] if shared else synth.morph_weights(m.nm, frames)
    dm = DeformModel(m)
    pitch = dm.output_pitch(api.OUT_SOA) if kind == "pitched" else 0
    assert kind != "pitched" or pitch > nv
    rows = pitch or nv
    d_pal, d_w = DeviceBuffer.from_numpy(pals), DeviceBuffer.from_numpy(rates)
    inputs = [d_pal, d_w]
    outs = dict(a=Out(ni * rows * 12), b=Out(ni * rows * 12))
    flags = DEV | (api.WEIGHTS_SHARED if shared and ni > 1 else 0)
    kw = {}
    if kind in ("bounds", "select"):
        outs["bounds"] = Out(ni * 24)
        kw["bounds_ptr"] = outs["bounds"].ptr
    if kind == "select":
        d_ids, d_cnt = DeviceBuffer.from_numpy(SEL_IDS), DeviceBuffer.from_numpy(np.array([SEL_LIVE], np.uint32))
        inputs += [d_ids, d_cnt]
        kw.update(select_ptr=d_ids.ptr, select_count_ptr=d_cnt.ptr, n_select=len(SEL_IDS))
    listed = sorted(SEL_IDS[:SEL_LIVE].tolist()) if kind == "select" else list(range(ni))

    def once():
        dm.deform_batched_raw(ni, d_w.ptr, d_pal.ptr, outs["a"].ptr, outs["b"].ptr, api.OUT_SOA, flags, pitch=pitch, **kw)

    def call():
        once()
        if kind == "shared-pass-twice":
            once()                          # the same rates again: the morph pass finds them unchanged on the device

    def after_first():
        shape = dm.last_launch_shape()
        assert shape["kernel"] == ("frame" if kind == "frame" else "deform"), shape
        assert shape["select"] == (kind == "select") and shape["bounds"] == (kind in ("bounds", "select")), shape
        if kind == "shared-pass-twice":
            assert dm.morph_pass_stats() == (1, 1, 0), "the second call did not take the device-side auto-skip"
        if kind == "select":
            assert dm.morph_pass_stats()[0] == 1, "the select call did not run the separate morph pass"

    def check(W):
        skin = oracle.normalize(m)
        pos, nrm = f32(W["a"], ni, rows, 3), f32(W["b"], ni, rows, 3)
        vimg = oracle.morph(m, rates) if shared else None
        for i in range(ni):
            if i not in listed:
                assert (W["a"].reshape(ni, -1)[i] == SENT).all() and (W["b"].reshape(ni, -1)[i] == SENT).all(), f"unlisted instance {i} written"
                continue
            ep, en = oracle.skin(m, pals[i], vimg if shared else oracle.morph(m, rates[i]), skin)
            gu.assert_bits_equal(pos[i, :nv], ep, f"{kind} nv {nv}: positions of instance {i} against the oracle")
            gu.assert_bits_equal(nrm[i, :nv], en, f"{kind} nv {nv}: normals of instance {i} against the oracle")
            if "bounds" in W:
                want = np.concatenate([ep.min(axis=0), ep.max(axis=0)])
                gu.assert_bits_equal(f32(W["bounds"], ni, 6)[i], want, f"{kind} nv {nv}: box of instance {i} against the oracle's positions")
        if pitch:
            assert (W["a"].reshape(ni, rows, 12)[:, nv:] == SENT).all() and (W["b"].reshape(ni, rows, 12)[:, nv:] == SENT).all()

    return Family(dm, outs, call, inputs, check=check, after_first=after_first)


@pytest.mark.gpu
@pytest.mark.parametrize("nv", [1000, 4099])
@pytest.mark.parametrize("kind", DEFORM_KINDS)
def test_deform_family_queues_on_the_borrowed_stream_only(gpu, oracle, kind, nv):
    fam = deform_family(kind, nv, oracle)
    try:
        sweep(fam, f"deform {kind}, nv {nv}")
    finally:
        fam.close()


# ---- GPU 1: cull, place, palette bounds --------------------------------------------------------------------------------------------
def small_model(nb=3):
    return DeformModel(synth.make_model(64, nb, 0, 0, seed=1))


def upload_struct(s):
    return DeviceBuffer.from_numpy(np.frombuffer(bytes(s), np.uint8))


@pytest.mark.gpu
@pytest.mark.parametrize("form", [1, 2], ids=["one-launch", "count-then-scatter"])
def test_cull_family_queues_on_the_borrowed_stream_only(gpu, monkeypatch, form):
    """Both forms, forced as tests/test_cull_bounds.py forces them (MMDX_CULL_FORM, chunks of 64): 200 instances are four chunks,
    the last one partial; form 2 is two launches with the handle's count scratch between them.  W against that file's restatement."""
    from tests.test_cull_bounds import check as cull_check, frustum_view, scene
    ni = 200
    monkeypatch.setenv("MMDX_CULL_FORM", str(form))
    monkeypatch.setenv("MMDX_CULL_CHUNK", "64")
    gpu.mmdx_debug_reload_env()
    view, b = frustum_view(16, 4), scene(ni)
    dm = small_model()
    d_b, d_view = DeviceBuffer.from_numpy(b), upload_struct(view.struct())
    outs = dict(ids=Out(4 * ni * 4), counts=Out(16), levels=Out(ni * 4))

    def call():
        dm.cull_bounds(d_b, d_view, ni, outs["ids"].ptr, outs["counts"].ptr, outs["levels"].ptr)

    def after_first():
        s = dm.last_launch_shape()
        assert (s["kernel"], s["select"], s["group"], s["ngroups"]) == ("cull", form, 64, 4), s

    def check(W):
        tail = np.full(8, 0xEEEEEEEE, np.uint32)           # that file's check() wants its sentinel words behind every array
        got = [np.concatenate([W[k].view(np.uint32), tail]) for k in ("ids", "counts", "levels")]
        cull_check(got, view.ref(b, True), ni, None, 4, f"form {form}")
    fam = Family(dm, outs, call, [d_b, d_view], check=check, after_first=after_first)
    try:
        sweep(fam, f"cull form {form}")
    finally:
        fam.close()
        monkeypatch.delenv("MMDX_CULL_FORM")
        monkeypatch.delenv("MMDX_CULL_CHUNK")
        gpu.mmdx_debug_reload_env()


def place_operands(ni, nb):
    """5 x 17 of tests/test_palette_place.py: 68 rows per instance, a partial last wave each; poses and sheared matrices."""
    from tests import palette_place_ref as pp
    rng = np.random.RandomState(100 * ni + nb)
    pal = synth.make_palettes(synth.make_model(64, nb, 0, 0, seed=13), np.arange(ni) * 7 + 1).copy()
    q = rng.normal(size=(ni, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    poses = np.zeros((ni, 8), F)
    poses[:, :3], poses[:, 3], poses[:, 4:] = rng.uniform(-50, 50, (ni, 3)), 9.0, q
    mats = pp.matrix_from_pose(poses) * F(1.5)
    mats[:, 4] += F(0.25)
    return pal, poses, np.ascontiguousarray(mats, F), pp


@pytest.mark.gpu
@pytest.mark.parametrize("matrix", [False, True], ids=["pose", "matrix"])
def test_place_family_queues_on_the_borrowed_stream_only(gpu, matrix):
    ni, nb = 5, 17
    pal, poses, mats, pp = place_operands(ni, nb)
    placements = mats if matrix else poses
    dm = small_model(nb)
    d_pal, d_pl = DeviceBuffer.from_numpy(pal), DeviceBuffer.from_numpy(placements)
    outs = dict(placed=Out(pal.nbytes))
    flags = PLACE_DEV | (api.PLACE_MATRIX if matrix else 0)
    fam = Family(dm, outs, lambda: dm.place_palettes(ni, d_pal.ptr, d_pl.ptr, outs["placed"].ptr, flags), [d_pal, d_pl],
                 check=lambda W: pp.assert_rows_equal(f32(W["placed"], ni, nb, 16), pp.place_crowd(pal, placements, matrix), "placed"))
    try:
        sweep(fam, "place " + ("matrix" if matrix else "pose"))
    finally:
        fam.close()


@pytest.mark.gpu
@pytest.mark.parametrize("nb", [63, 65], ids=["wave-per-instance", "workgroup-per-instance"])
def test_palette_bounds_family_queues_on_the_borrowed_stream_only(gpu, nb):
    """Table lengths on both sides of the wave edge of tests/test_palette_bounds.py, three instances; W against its restatement."""
    from tests import palette_bounds_ref as pb
    ni = 3
    m = synth.make_model(8 * nb, nb, 2, 16, seed=900 + nb)
    pals = np.ascontiguousarray(synth.make_palettes(m, np.arange(ni) * 0.83 + 1))
    dm = DeformModel(m)
    d_pal = DeviceBuffer.from_numpy(pals)
    outs = dict(boxes=Out(ni * 24))
    fam = Family(dm, outs, lambda: dm.palette_bounds_raw(ni, d_pal.ptr, outs["boxes"].ptr, PAL_OUT, 0.1, 1.0), [d_pal],
                 check=lambda W: gu.assert_bits_equal(f32(W["boxes"], ni, 6), pb.palette_bounds(dm.bone_boxes(), pals, 0.1, 1.0), "boxes"))
    try:
        sweep(fam, f"palette bounds, {nb} boxes")
    finally:
        fam.close()


# ---- GPU 1: motion and rig -----------------------------------------------------------------------------------------------------------
NI_M, NB_M, NM_M = 67, 41, 7          # the crowd of tests/test_motion_blend.py: a wave of the track kernels spans several instances
NAMES = [f"bone{i}" for i in range(NB_M)]
MNAMES = [f"m{i}" for i in range(NM_M)]


class Motions:
    """Three clips over 41 bones and 7 morphs, their single-clip motions, the set of them, the parallel-FK rig of 41 bones, and 67
    instances' clip ids, frames, times and cross-fade weights in device memory."""

    def __init__(self):
        rng = np.random.RandomState(41)
        data = []
        for seed, sub in enumerate((NAMES[:35], NAMES[4:], NAMES[::2])):
            mk = [(n, int(f), float(F(rng.uniform(-0.2, 1.2)))) for n in MNAMES[:5 + seed] for f in sorted(rng.choice(150, 5, replace=False))]
            data.append(vmd.write_vmd(synth.make_bone_keys(sub, 30 + seed, keys_per=4 + seed, span=150), mk))
        self.vs = [vmd.Vmd(d) for d in data]
        self.bms, self.mms = [v.bind_bones(NAMES) for v in self.vs], [v.bind_morphs(MNAMES) for v in self.vs]
        self.ms = vmd.MotionSet(self.bms, self.mms)
        self.sk = vmd.Skeleton(*synth.make_skeleton(NB_M, 3, 5, 0.25, 3))
        assert self.sk.info["solver"] == vmd.SOLVER_PARALLEL_FK
        ca, cb = rng.randint(0, 3, NI_M).astype(np.uint32), rng.randint(0, 3, NI_M).astype(np.uint32)
        ca[5], cb[6], ca[7], cb[7] = vmd.CLIP_NONE, vmd.CLIP_NONE, 3 + 5, vmd.CLIP_NONE
        ta, tb = rng.uniform(-0.2, 5.5, NI_M), rng.uniform(-0.2, 5.5, NI_M)
        w = rng.uniform(0, 1, NI_M).astype(F)
        w[:4] = (0.0, 1.0, 5e-8, 2.0)
        self.frames = (np.arange(NI_M) * 7 % 160).astype(np.uint32)
        self.host = dict(ca=ca, ta=ta, cb=cb, tb=tb, w=w)
        self.d = {k: DeviceBuffer.from_numpy(a) for k, a in dict(self.host, frames=self.frames).items()}
        self.blend_ptrs = [self.d[k].ptr for k in ("ca", "ta", "cb", "tb", "w")]

    def close(self):
        for x in list(self.d.values()):
            x.free()
        for x in [self.ms, self.sk] + self.bms + self.mms + self.vs:
            x.close()


POSE_B, PAL_B, RATE_B = NI_M * NB_M * 32, NI_M * NB_M * 64, NI_M * NM_M * 4


def motion_family(kind, oracle):
    z = Motions()
    dm = small_model()
    d, n = z.d, NI_M
    fr, ta, ca = d["frames"].ptr, d["ta"].ptr, d["ca"].ptr
    check = None
    if kind == "morph-motion-eval":
        outs = dict(frames=Out(RATE_B), times=Out(RATE_B))

        def call():
            z.mms[1].eval_device(n, fr, outs["frames"].ptr, dm)
            z.mms[1].eval_time_device(n, ta, outs["times"].ptr, dm)
    elif kind == "bone-motion-eval":
        outs = dict(frames=Out(POSE_B), times=Out(POSE_B))

        def call():
            z.bms[1].eval_device(n, fr, outs["frames"].ptr, dm)
            z.bms[1].eval_time_device(n, ta, outs["times"].ptr, dm)
    elif kind == "solve-motion":
        outs = dict(frames=Out(PAL_B), times=Out(PAL_B))

        def call():
            z.sk.solve_motion_device(z.bms[0], n, fr, outs["frames"].ptr, dm)
            z.sk.solve_motion_time_device(z.bms[0], n, ta, outs["times"].ptr, dm)

        def check(W):
            from tests.test_rig import oracle_poses
            rig = synth.make_skeleton(NB_M, 3, 5, 0.25, 3)
            for i in (0, 33, n - 1):
                poses = oracle_poses(oracle, z.vs[0], NAMES, z.frames[i:i + 1])[0]
                gu.assert_bits_equal(f32(W["frames"], n, NB_M, 16)[i], oracle.bone_solve(rig[0], rig[1], poses, rig[2], rig[3]),
                                     f"solve_motion: palette of instance {i} against the oracle")
    elif kind == "motion-set":
        outs = dict(bones=Out(POSE_B), bones_t=Out(POSE_B), morphs=Out(RATE_B), morphs_t=Out(RATE_B), pal=Out(PAL_B), pal_t=Out(PAL_B))

        def call():
            z.ms.eval_bones_device(n, ca, fr, outs["bones"].ptr, dm)
            z.ms.eval_bones_time_device(n, ca, ta, outs["bones_t"].ptr, dm)
            z.ms.eval_morphs_device(n, ca, fr, outs["morphs"].ptr, dm)
            z.ms.eval_morphs_time_device(n, ca, ta, outs["morphs_t"].ptr, dm)
            z.sk.solve_motion_set_device(z.ms, n, ca, fr, outs["pal"].ptr, dm)
            z.sk.solve_motion_set_time_device(z.ms, n, ca, ta, outs["pal_t"].ptr, dm)
    else:
        assert kind == "cross-fade"
        outs = dict(bones=Out(POSE_B), morphs=Out(RATE_B), pal=Out(PAL_B))

        def call():
            z.ms.blend_bones_time_device(n, *z.blend_ptrs, outs["bones"].ptr, dm)
            z.ms.blend_morphs_time_device(n, *z.blend_ptrs, outs["morphs"].ptr, dm)
            z.sk.solve_motion_set_blend_time_device(z.ms, n, *z.blend_ptrs, outs["pal"].ptr, dm)
    return Family(dm, outs, call, [z], check=check)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["morph-motion-eval", "bone-motion-eval", "solve-motion", "motion-set", "cross-fade"])
def test_motion_family_queues_on_the_borrowed_stream_only(gpu, oracle, kind):
    fam = motion_family(kind, oracle)
    try:
        sweep(fam, kind)
    finally:
        fam.close()


@pytest.mark.gpu
@pytest.mark.parametrize("rig", ["fk", "ik"])
def test_skeleton_solve_family_queues_on_the_borrowed_stream_only(gpu, oracle, rig):
    """fk: the 40-bone rig with forward parents, levels and post-physics bones of tests/test_rig.py, five instances, against the oracle.
    ik: synth.make_ik_rig(44, 1, n_ik=3, n_append=4), 70 instances (the last workgroup partly empty) -- the ordered solver, cut into
    segments around its ik_coop_kernel rounds: several dependent launches, each of which has to land on the borrowed stream."""
    from tests.test_rig import random_poses
    if rig == "fk":
        ni, nb, args = 5, 40, synth.make_skeleton(40, 2, 5, 0.25, 3)
        poses = random_poses(ni, nb, 2)
    else:
        ni, nb, args = 70, 44, synth.make_ik_rig(44, 1, n_ik=3, n_append=4)
        poses = random_poses(ni, nb, 201)
    sk = vmd.Skeleton(*args)
    if rig == "ik":
        assert sk.info["solver"] == vmd.SOLVER_SERIAL and sk.info["n_ik_rounds_16_lanes"] > 0, sk.info
    dm = small_model()
    d_poses = DeviceBuffer.from_numpy(poses)
    outs = dict(pal=Out(ni * nb * 64))

    def check(W):
        got = f32(W["pal"], ni, nb, 16)
        for i in range(ni) if rig == "fk" else (0, 34, ni - 1):
            if rig == "fk":
                gu.assert_bits_equal(got[i], oracle.bone_solve(args[0], args[1], poses[i], args[2], args[3]), f"FK palette {i}")
            else:
                gu.assert_bits_equal_or_both_nan(got[i], oracle.bone_solve_full(args[0], args[1], poses[i], *args[2:]), f"IK palette {i}")
    fam = Family(dm, outs, lambda: sk.solve_device(ni, d_poses.ptr, outs["pal"].ptr, dm), [d_poses, sk], nan_ok=rig == "ik", check=check)
    try:
        sweep(fam, f"skeleton solve, {rig} rig")
    finally:
        fam.close()


# ---- GPU 1: the whole chain ----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_whole_chain_recorded_as_one_graph_on_the_borrowed_stream(gpu):
    """solve_motion -> place (in place) -> palette bounds -> cull -> select, every operand in device memory, one graph on S: the
    deform reads the list and the count the cull wrote a launch earlier.  24 instances 12 units apart along x, one plane at x = 0:
    a proper, non-empty subset is deformed, the rest of the outputs keeps its sentinel."""
    ni, nv, spacing = 24, 300, 12.0
    z = Motions()
    dm = DeformModel(synth.make_model(nv, NB_M, 0, 0, seed=7301))
    place = np.zeros((ni, 8), F)
    place[:, 0], place[:, 7] = (np.arange(ni) - ni / 2 + 0.5) * spacing, 1.0
    view = make_cull_view([[1, 0, 0, 0]], (0, 0, 0), ())
    d_fr, d_place, d_view = DeviceBuffer.from_numpy(z.frames[:ni].copy()), DeviceBuffer.from_numpy(place), upload_struct(view)
    outs = dict(pal=Out(ni * NB_M * 64), boxes=Out(ni * 24), ids=Out(4 * ni * 4), counts=Out(16), levels=Out(ni * 4),
                a=Out(ni * nv * 12), b=Out(ni * nv * 12))

    def call():
        z.sk.solve_motion_device(z.bms[0], ni, d_fr.ptr, outs["pal"].ptr, dm)
        dm.place_palettes(ni, outs["pal"].ptr, d_place.ptr, outs["pal"].ptr, PLACE_DEV)
        dm.palette_bounds_raw(ni, outs["pal"].ptr, outs["boxes"].ptr, PAL_OUT)
        dm.cull_bounds(outs["boxes"].ptr, d_view, ni, outs["ids"].ptr, outs["counts"].ptr, outs["levels"].ptr)
        dm.deform_batched_raw(ni, None, outs["pal"].ptr, outs["a"].ptr, outs["b"].ptr, api.OUT_SOA, PAL_OUT,
                              select_ptr=outs["ids"].ptr, select_count_ptr=outs["counts"].ptr, n_select=ni)

    def check(W):
        count = int(W["counts"].view(np.uint32)[0])
        listed = W["ids"].view(np.uint32)[:count].tolist()
        levels = W["levels"].view(np.uint32)
        assert 0 < count < ni and listed == sorted(listed) == np.nonzero(levels == 0)[0].tolist(), (count, listed)
        written = [(W["a"].reshape(ni, -1)[i] != SENT).any() for i in range(ni)]
        assert np.nonzero(written)[0].tolist() == listed, "the deform wrote other instances than the cull listed"
        assert np.isfinite(f32(W["a"], ni, nv, 3)[listed]).all()
    fam = Family(dm, outs, call, [d_fr, d_place, d_view, z], check=check)
    try:
        sweep(fam, "solve -> place -> bounds -> cull -> select")
    finally:
        fam.close()


# ---- GPU 2: host operands on a borrowed stream -----------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_host_operand_forms_return_finished_results_on_a_borrowed_stream(gpu, oracle):
    """Every form that takes or returns host memory waits on the model's stream before it returns -- the borrowed one when one is
    set: the results are read the moment the call returns, with no synchronisation of the caller's, and equal the own-stream bits
    (the deform forms also the oracle's).  The cull's outputs are device memory in either form (its host form is the view): it
    is read after waiting for S alone."""
    from tests.test_cull_bounds import frustum_view, scene
    from tests.test_rig import random_poses
    m = synth.make_model(1000, 17, 6, 60, seed=9800)
    ni = 13
    frames = np.arange(ni) * 5 + 2
    pals, rates = synth.make_palettes(m, frames), synth.morph_weights(m.nm, frames)
    ids = np.array([12, 0, 5, 6], np.uint32)
    pal_p, poses_p, mats_p, _ = place_operands(5, 17)
    rig = synth.make_skeleton(40, 2, 5, 0.25, 3)
    bone_poses = random_poses(5, 40, 2)
    cview, cbounds = frustum_view(6, 3), scene(200)
    z = Motions()
    sk = vmd.Skeleton(*rig)
    with DeformModel(m) as dm, small_model(17) as pm:
        d_pal, d_w, d_cb = DeviceBuffer.from_numpy(pals), DeviceBuffer.from_numpy(rates), DeviceBuffer.from_numpy(cbounds)
        sel_outs = dict(a=Out(ni * m.nv * 12), b=Out(ni * m.nv * 12))
        cull_outs = dict(ids=Out(4 * 200 * 4), counts=Out(16), levels=Out(200 * 4))

        def select_host(wait):
            for o in sel_outs.values():
                o.fill()
            # (per-instance rates of a select call are indexed by instance, like the palettes: the whole [ni][nm] array)
            dm.deform_batched_select(ni, ids, d_w.ptr, d_pal.ptr, sel_outs["a"].ptr, sel_outs["b"].ptr, api.OUT_SOA, DEV)
            return [o.read("host-list select") for o in sel_outs.values()]

        def cull_host(wait):
            for o in cull_outs.values():
                o.fill()
            st = cview.struct()
            dm.cull_bounds(d_cb, st, 200, cull_outs["ids"].ptr, cull_outs["counts"].ptr, cull_outs["levels"].ptr)
            wait()
            return [o.read("host-view cull") for o in cull_outs.values()]
        # (host clip ids are validated: the out-of-range one of the device crowd plays nothing here)
        blend_host = [np.where(z.host[k] == 8, vmd.CLIP_NONE, z.host[k]).astype(np.uint32) if k[0] == "c" else z.host[k] for k in ("ca", "ta", "cb", "tb", "w")]
        forms = {
            "mmdx_deform": lambda wait: dm.deform(rates[3], pals[3]),
            "mmdx_deform_vertex32": lambda wait: [dm.deform_vertex32(rates[3], pals[3])],
            "deform_batched, host arrays": lambda wait: dm.deform_batched(rates, pals),
            "deform_batched, shared rates": lambda wait: dm.deform_batched(rates[0], pals, shared_weights=True),
            "deform_batched_bounds, host arrays": lambda wait: dm.deform_batched(rates, pals, bounds=True),
            "deform_batched_select, host list": select_host,
            "palette_place, poses": lambda wait: [pm.place(pal_p, poses_p)],
            "palette_place, matrices": lambda wait: [pm.place(pal_p, mats_p)],
            "palette_bounds": lambda wait: [dm.palette_bounds(pals, 0.1, 1.0)],
            "cull_bounds, host view": cull_host,
            "skeleton_solve": lambda wait: [sk.solve(bone_poses, dm)],
            "skeleton_solve_motion": lambda wait: [z.sk.solve_motion(z.bms[0], z.frames, dm)],
            "bone_motion_eval": lambda wait: [z.bms[1].eval(z.frames, dm)],
            "morph_motion_eval_time": lambda wait: [z.mms[1].eval_time(z.host["ta"], dm)],
            "motion_set_blend_bones_time": lambda wait: [z.ms.blend_bones_time(*blend_host, model=dm)],
        }
        own = {name: [np.array(x, copy=True) for x in f(dm.sync)] for name, f in forms.items()}
        # the oracle, where these forms have one
        skin = oracle.normalize(m)
        ep, en = oracle.skin(m, pals[3], oracle.morph(m, rates[3]), skin)
        gu.assert_bits_equal(own["mmdx_deform"][0], ep, "mmdx_deform positions")
        gu.assert_bits_equal(own["mmdx_deform"][1], en, "mmdx_deform normals")
        for i in (0, ni - 1):
            ep, en = oracle.skin(m, pals[i], oracle.morph(m, rates[i]), skin)
            gu.assert_bits_equal(own["deform_batched, host arrays"][0][i], ep, f"deform_batched positions {i}")
            gu.assert_bits_equal(own["deform_batched_bounds, host arrays"][2][i], np.concatenate([ep.min(axis=0), ep.max(axis=0)]), f"box {i}")
        sel_pos = f32(own["deform_batched_select, host list"][0], ni, m.nv, 3)
        for i in range(ni):
            if i in ids.tolist():
                gu.assert_bits_equal(sel_pos[i], oracle.skin(m, pals[i], oracle.morph(m, rates[i]), skin)[0], f"host-list select positions {i}")
            else:
                assert (sel_pos[i].view(np.uint8) == SENT).all(), f"host-list select wrote unlisted instance {i}"
        for i in range(5):
            gu.assert_bits_equal(own["skeleton_solve"][0][i], oracle.bone_solve(rig[0], rig[1], bone_poses[i], rig[2], rig[3]), f"FK palette {i}")
        with hs.Stream() as S, hs.Stream() as SP:
            try:
                dm.set_stream(S.ptr)
                pm.set_stream(SP.ptr)
                for name, f in forms.items():
                    got = f(S.synchronize)
                    assert len(got) == len(own[name])
                    for k, (g, w) in enumerate(zip(got, own[name])):
                        assert g.shape == w.shape and g.tobytes() == w.tobytes(), f"{name}: result {k} on the borrowed stream differs from the own stream's"
            finally:
                dm.set_stream(None)
                pm.set_stream(None)
        for x in [d_pal, d_w, d_cb] + list(sel_outs.values()) + list(cull_outs.values()):
            x.free()
    sk.close()
    z.close()


# ---- GPU 3: a switch orders the new stream behind the old ------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("target", ["second-stream", "own-stream"])
@pytest.mark.parametrize("form", ["per-instance", "shared"])
def test_switch_orders_the_new_stream_behind_the_old(gpu, oracle, form, target):
    """Call A (palettes P_A) waits behind a closed gate on S1; after a switch, call B (palettes P_B) goes into the SAME outputs on the
    new stream.  B must not overtake A: while the gate is closed both calls and the switch have returned (a switch never blocks the
    host) and the new stream is not ready; once it opens, the outputs hold B's bits.  shared: A and B also share the model's morphed
    positions, slot weights and the record of the rates they were computed from, with different rates.
    own-stream: the switch goes back with NULL; only the final contents can be checked there."""
    m = synth.make_model(1000, 17, 6, 60, seed=9900)
    ni = 13
    shared = form == "shared"
    P = {k: synth.make_palettes(m, np.arange(ni) * 3 + off) for k, off in (("A", 1), ("B", 40))}
    R = {k: synth.morph_weights(m.nm, fr)[0] if shared else synth.morph_weights(m.nm, np.arange(ni) * 2 + fr) for k, fr in (("A", 10), ("B", 55))}
    flags = DEV | (api.WEIGHTS_SHARED if shared else 0)
    with DeformModel(m) as dm:
        d_pal = {k: DeviceBuffer.from_numpy(P[k]) for k in P}
        d_w = {k: DeviceBuffer.from_numpy(R[k]) for k in R}
        outs = dict(a=Out(ni * m.nv * 12), b=Out(ni * m.nv * 12))

        def call(k):
            dm.deform_batched_raw(ni, d_w[k].ptr, d_pal[k].ptr, outs["a"].ptr, outs["b"].ptr, api.OUT_SOA, flags)

        def read(what):
            return {k: o.read(what) for k, o in outs.items()}
        # B's expected bits: eagerly on the own stream, and against the oracle
        call("A")
        call("B")
        dm.sync()
        want = read("B on the own stream")
        skin = oracle.normalize(m)
        for i in (0, ni - 1):
            ep, en = oracle.skin(m, P["B"][i], oracle.morph(m, R["B"] if shared else R["B"][i]), skin)
            gu.assert_bits_equal(f32(want["a"], ni, m.nv, 3)[i], ep, f"B: positions of instance {i} against the oracle")
            gu.assert_bits_equal(f32(want["b"], ni, m.nv, 3)[i], en, f"B: normals of instance {i} against the oracle")
        call("A")
        dm.sync()
        assert read("A")["a"].tobytes() != want["a"].tobytes()             # A and B differ: the order is visible
        for o in outs.values():
            o.fill()
        with hs.Stream() as S1, hs.Stream() as S2:
            gate = None
            try:
                dm.set_stream(S1.ptr)
                gate = S1.gate()
                call("A")
                dm.set_stream(S2.ptr if target == "second-stream" else None)
                held_after_switch = not gate._done.is_set()
                call("B")
                # what can be seen while the gate is closed: taken down first, judged after the streams have drained
                held_after_calls = not gate._done.is_set()
                s1_state = S1.query()
                s2_states = {S2.query() for _ in range(200)} if target == "second-stream" else None
                held_to_the_end = not gate._done.is_set()
                gate.open()
            finally:
                if gate is not None:
                    gate.release()
                S1.synchronize()
                S2.synchronize()
                dm.set_stream(None)
                dm.sync()
            got = read("after the gate opened")
            holds = {k: "B" if got[k].tobytes() == want[k].tobytes() else "not B" for k in want}
            print(f"switch {form} -> {target}: gate held after the switch {held_after_switch}, after both calls {held_after_calls}, through "
                  f"the queries {held_to_the_end}; S1 {s1_state}; S2 {s2_states}; outputs hold {holds}")
            # both calls and the switch returned while the gate was closed: a switch never blocks the host
            assert held_after_switch and held_after_calls and held_to_the_end, "the gate was gone before the test opened it"
            assert s1_state == hs.ERROR_NOT_READY
            if target == "second-stream":
                assert s2_states == {hs.ERROR_NOT_READY}, "call B ran on the new stream while call A was still waiting on the old one"
            assert set(holds.values()) == {"B"}, f"the outputs do not hold call B's bits ({holds}): the new stream was not ordered behind the old one"
        for x in list(d_pal.values()) + list(d_w.values()) + list(outs.values()):
            x.free()


# ---- GPU 4: misuse -------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_switch_while_recording_is_refused_and_changes_nothing(gpu, oracle):
    m = synth.make_model(1000, 17, 6, 60, seed=9950)
    ni = 13
    frames = np.arange(ni) * 5 + 2
    pals, rates = synth.make_palettes(m, frames), synth.morph_weights(m.nm, frames)
    with DeformModel(m) as dm, hs.Stream() as S, hs.Stream() as S2:
        d_pal, d_w = DeviceBuffer.from_numpy(pals), DeviceBuffer.from_numpy(rates)
        outs = dict(a=Out(ni * m.nv * 12), b=Out(ni * m.nv * 12))

        def call():
            dm.deform_batched_raw(ni, d_w.ptr, d_pal.ptr, outs["a"].ptr, outs["b"].ptr, api.OUT_SOA, DEV)

        def read(what):
            return {k: o.read(what) for k, o in outs.items()}
        call()
        dm.sync()
        want = read("own stream")
        skin = oracle.normalize(m)
        ep, en = oracle.skin(m, pals[ni - 1], oracle.morph(m, rates[ni - 1]), skin)
        gu.assert_bits_equal(f32(want["a"], ni, m.nv, 3)[ni - 1], ep, "positions against the oracle")
        try:
            # a switch to the stream the model already has is a no-op, on the own stream and on a borrowed one
            dm.set_stream(None)
            dm.set_stream(S.ptr)
            dm.set_stream(S.ptr)
            for o in outs.values():
                o.fill()
            dm.graph_begin()
            try:
                for other in (S2.ptr, None, S.ptr):
                    assert gpu.mmdx_model_set_stream(dm.h, other) == INVALID, "a switch was accepted while the model records"
                    assert b"record" in gpu.mmdx_last_error_string()
                assert S.capture_status() == hs.CAPTURE_ACTIVE and S2.capture_status() == hs.CAPTURE_NONE
                call()
            finally:
                g = dm.graph_end()                      # ends cleanly: the capture on S is closed, on S
            try:
                assert S.capture_status() == hs.CAPTURE_NONE
                device_synchronize()
                assert all((raw == SENT).all() for raw in read("after the recording").values())
                g.launch()
                S.synchronize()
                got = read("replay")
                assert all(got[k].tobytes() == want[k].tobytes() for k in want), "the replay after a refused switch differs"
            finally:
                g.close()
            # the model is still on S: an eager call lands there
            for o in outs.values():
                o.fill()
            call()
            S.synchronize()
            got = read("eager on S")
            assert all(got[k].tobytes() == want[k].tobytes() for k in want)
        finally:
            dm.set_stream(None)
        for x in [d_pal, d_w] + list(outs.values()):
            x.free()


@pytest.mark.gpu
def test_stream_of_another_device_is_refused(gpu):
    """Only where a second device is visible; with one device the refusal has nothing to be asked with."""
    if device_count() < 2:
        return
    device_select(0)
    with small_model() as dm:
        with hs.Stream(device=1) as other:
            hs.hip().hipSetDevice(0)
            assert gpu.mmdx_model_set_stream(dm.h, other.ptr) == INVALID
            assert b"device" in gpu.mmdx_last_error_string()
            dm.sync()                                   # still on its own stream, and usable
        hs.hip().hipSetDevice(0)

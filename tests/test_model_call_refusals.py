"""What the calls on a model handle (mmdx_deform_batched / _bounds / _select, mmdx_palette_place, mmdx_palette_bounds,
mmdx_cull_bounds) and the morph-motion calls (mmdx_morph_motion_eval / _eval_time) refuse, in which order, and what they accept
while a graph is being recorded.  Every text below is the library's own, with its status code.  The calls share their plumbing --
the instance-list check, the model-call preamble, the host round trip (csrc/host_runtime.hpp) -- and this file holds the order
of refusals of each entry point in place: where two checks compete, a call that violates both says which one answers.

The part without the gpu mark decides everything on a MMDX_CREATE_HOST_ONLY model (or without a model): nothing there reaches
the device.  The deform calls refuse a host-only model right behind their struct_size, so their flag and list checks are in the
gpu part; the list checks of the rig form (mmdx_skeleton_solve_select, decided before the device is looked for) are here.

The gpu part runs 2 instances of a 64-vertex, 3-bone model with one morph and a VMD with one morph track.  Nothing is compared
numerically.  (A host-flagged list that points at device memory: outside a recording only the deform form classifies the
pointer; the rig form would read it on the host, which is why it is tried there only while recording, where both forms refuse a
host list before they look at it.)"""
import ctypes as C
import threading

import numpy as np
import pytest

from simple_mmd_renderer_amd import _capi as api
from simple_mmd_renderer_amd import synth, vmd
from simple_mmd_renderer_amd.engine import DeformModel, DeviceBuffer, device_count, make_cull_view

NI, NV, NB = 2, 64, 3
INVALID, NO_DEVICE = 1, 3
PAL, WEIGHTS, OUT, PLACE = api.PALETTE_ON_DEVICE, api.WEIGHTS_ON_DEVICE, api.OUT_ON_DEVICE, api.PLACE_ON_DEVICE
FR, POSES = vmd.FRAMES_ON_DEVICE, vmd.POSES_ON_DEVICE

HOST_ONLY = "model was created with MMDX_CREATE_HOST_ONLY: nothing to run on (this engine has no CPU fallback)"
OTHER_THREAD = ("this model's stream is recording a graph on another thread: recorded calls must come from the thread that called "
                "mmdx_graph_begin")
OPERANDS = "while a graph is being recorded every operand must be in device memory"
PLACE_OPERANDS = "while a graph is being recorded palettes, placements and out_palettes must all be in device memory"
PBOUNDS_OPERANDS = "while a graph is being recorded palettes and out_bounds must both be in device memory"
HOST_LIST = "while a graph is being recorded the instance list must be in device memory (MMDX_SELECT_ON_DEVICE)"
LIST_IN_DEVICE_MEMORY = "ids / count of mmdx_instance_select point to device memory: pass MMDX_SELECT_ON_DEVICE"
LIST_SIZE = "mmdx_instance_select.struct_size mismatch"
LIST_BITS = "unknown bits in mmdx_instance_select.flags"
LIST_RESERVED = "mmdx_instance_select.reserved0 must be 0"
LIST_NULL = "mmdx_instance_select.ids is NULL"
LIST_ALIGN = "device ids / count of mmdx_instance_select must be 4-byte aligned"
DEFORM_SELECT_OPERANDS = ("mmdx_deform_batched_select takes device operands only: pass MMDX_PALETTE_ON_DEVICE | MMDX_OUT_ON_DEVICE, "
                          "and MMDX_WEIGHTS_ON_DEVICE with morph_weights")
SOLVE_SELECT_OPERANDS = ("mmdx_skeleton_solve_select takes device operands only: pass MMDX_POSES_ON_DEVICE | MMDX_OUT_ON_DEVICE, and "
                         "MMDX_WEIGHTS_ON_DEVICE with morph_weights")
FIRST_USE = "first use of this motion on the device: run the sequence once before recording it"
WOULD_GROW = (": a scratch buffer of this handle would have to grow, but a recorded graph (mmdx_graph_*) holds its address -- destroy "
              "the graph first, or size the buffers with an un-recorded call of the largest shape before recording")


def model():
    return synth.make_model(NV, NB, 1, 8, seed=5)


def said(status, want_status, want_text, what, exact=True):
    msg = api.lib().mmdx_last_error_string().decode()
    print(f"{what}: status {status}: {msg}")
    assert status == want_status and (msg == want_text if exact else want_text in msg), (what, status, msg, want_text)


def accepted(status, what):
    assert status == 0, (what, status, api.lib().mmdx_last_error_string().decode())


def deform_args(w, pal, a, b, flags, n=NI, size=None):
    return api.DeformArgs(C.sizeof(api.DeformArgs) if size is None else size, flags, n, api.OUT_SOA, w, pal, a, b, 1.0, 0)


def place_args(pal, w, out, flags, n=NI, reserved0=0, size=None):
    return api.PlaceArgs(C.sizeof(api.PlaceArgs) if size is None else size, flags, n, reserved0, pal, w, out)


def pbounds_args(pal, out, flags, n=NI, reserved0=0, size=None, pos_scale=1.0):
    return api.PaletteBoundsArgs(C.sizeof(api.PaletteBoundsArgs) if size is None else size, flags, n, reserved0, pal, out, pos_scale, 0.0)


def cull_args(bounds, view, ids, counts, flags=0, n=NI, stride=NI, size=None):
    return api.CullArgs(C.sizeof(api.CullArgs) if size is None else size, flags, n, stride, bounds, view, ids, counts, None)


def select(ids, n_ids, count=None, on_device=False, size=None, flags=None, reserved0=0):
    s = vmd.instance_select(ids, n_ids, count, on_device=on_device)
    if size is not None:
        s.struct_size = size
    if flags is not None:
        s.flags = flags
    s.reserved0 = reserved0
    return s


class HostArrays:
    """Every operand and output of the calls below in host memory, by name."""

    def __init__(self, n=NI):
        self.a = dict(pal=np.tile(np.eye(4, dtype=np.float32).reshape(16), (n, NB, 1)), w=np.zeros((n, 1), np.float32),
                      out_a=np.zeros((n, NV, 3), np.float32), out_b=np.zeros((n, NV, 3), np.float32), bounds=np.zeros((n, 6), np.float32),
                      place=np.tile(np.array([0, 0, 0, 0, 0, 0, 0, 1], np.float32), (n, 1)), placed=np.zeros((n, NB, 16), np.float32),
                      ids=np.array([1, 0], np.uint32), count=np.array([2], np.uint32), cull_ids=np.zeros(n, np.uint32),
                      cull_counts=np.zeros(api.CULL_MAX_LODS, np.uint32), frames=np.arange(n, dtype=np.uint32),
                      times=np.arange(n, dtype=np.float64) / 30, morphs=np.zeros((n, 1), np.float32))

    def ptr(self, name):
        return self.a[name].ctypes.data


# ---- without a GPU --------------------------------------------------------------------------------------------------------------
def test_deform_calls_on_a_host_only_model_nulls_struct_size_then_the_model(hip_lib):
    lib, h = hip_lib, HostArrays()
    with DeformModel(model(), host_only=True) as dm:
        good = deform_args(h.ptr("w"), h.ptr("pal"), h.ptr("out_a"), h.ptr("out_b"), 0)
        bad_size = deform_args(None, None, None, None, 0x80000000, n=0, size=4)       # ... and everything behind struct_size wrong too
        sel = select(h.ptr("ids"), NI)
        # the NULLs an entry point owns answer first: ahead of a NULL model, ahead of struct_size
        said(lib.mmdx_deform_batched_bounds(None, None, None), INVALID, "out_bounds is NULL", "bounds: every argument NULL")
        said(lib.mmdx_deform_batched_bounds(dm.h, C.byref(bad_size), None), INVALID, "out_bounds is NULL", "bounds: NULL out_bounds + struct_size")
        said(lib.mmdx_deform_batched_select(None, C.byref(bad_size), None, None), INVALID,
             "select is NULL (mmdx_deform_batched / mmdx_deform_batched_bounds deform every instance)", "select: NULL select + NULL model")
        for name, call in (("plain", lambda m, a: lib.mmdx_deform_batched(m, a)),
                           ("bounds", lambda m, a: lib.mmdx_deform_batched_bounds(m, a, h.ptr("bounds"))),
                           ("select", lambda m, a: lib.mmdx_deform_batched_select(m, a, C.byref(sel), None))):
            said(call(None, C.byref(bad_size)), INVALID, "model / args is NULL", f"{name}: NULL model + struct_size")
            said(call(dm.h, None), INVALID, "model / args is NULL", f"{name}: NULL args")
            said(call(dm.h, C.byref(bad_size)), INVALID, "mmdx_deform_args.struct_size mismatch", f"{name}: struct_size + flag bits + NULLs")
            # a host-only model is refused next: ahead of n_instances, flag bits, NULL operands and (select) the list's header
            bad = deform_args(None, None, None, None, 0x80000000, n=0)
            sel_bad = select(None, NI, size=4, flags=0x10, reserved0=1)
            refuse = call if name != "select" else lambda m, a: lib.mmdx_deform_batched_select(m, a, C.byref(sel_bad), None)
            said(refuse(dm.h, C.byref(bad)), NO_DEVICE, HOST_ONLY, f"{name}: host-only model + everything behind it")
            said(call(dm.h, C.byref(good)), NO_DEVICE, HOST_ONLY, f"{name}: host-only model, a good call")


def test_palette_place_on_a_host_only_model_bits_before_nulls_the_model_last(hip_lib):
    lib, h = hip_lib, HostArrays()
    with DeformModel(model(), host_only=True) as dm:
        call = lambda a: lib.mmdx_palette_place(dm.h, C.byref(a))                     # noqa: E731
        pal, w, out = h.ptr("pal"), h.ptr("place"), h.ptr("placed")
        said(lib.mmdx_palette_place(None, C.byref(place_args(pal, w, out, 0, size=4))), INVALID, "model / args is NULL", "NULL model + struct_size")
        said(lib.mmdx_palette_place(dm.h, None), INVALID, "model / args is NULL", "NULL args")
        said(call(place_args(None, None, None, 0x80000000, reserved0=1, size=4)), INVALID, "mmdx_place_args.struct_size mismatch", "struct_size + rest")
        said(call(place_args(None, None, None, 0x80000000, reserved0=1)), INVALID, "unknown flag bits in mmdx_place_args.flags",
             "unknown bits + reserved0 + NULL operands: the bits answer")
        said(call(place_args(None, None, None, 0, reserved0=1)), INVALID, "mmdx_place_args.reserved0 must be 0", "reserved0 + NULL operands")
        accepted(call(place_args(None, None, None, 0, n=0)), "no instances: nothing to do, even on a host-only model")
        said(call(place_args(pal, None, out, 0)), INVALID, "palettes / placements / out_palettes is NULL", "NULL placements")
        said(call(place_args(pal, w, pal + 64, 0)), INVALID,
             "palettes and out_palettes overlap without being the same array (in place is out_palettes == palettes)", "overlap")
        said(call(place_args(pal + 4, w, out, PAL)), INVALID, "device palettes / out_palettes must be 16-byte aligned", "alignment")
        said(call(place_args(pal, w, out, 0)), NO_DEVICE, HOST_ONLY, "host-only model, a good call with host operands")
        said(call(place_args(pal, w, out, PAL | PLACE | OUT)), NO_DEVICE, HOST_ONLY, "host-only model, a good call with device flags")


def test_palette_bounds_on_a_host_only_model_bits_before_nulls_the_model_last(hip_lib):
    lib, h = hip_lib, HostArrays()
    with DeformModel(model(), host_only=True) as dm:
        call = lambda a: lib.mmdx_palette_bounds(dm.h, C.byref(a))                    # noqa: E731
        pal, out = h.ptr("pal"), h.ptr("bounds")
        said(lib.mmdx_palette_bounds(None, C.byref(pbounds_args(pal, out, 0, size=4))), INVALID, "model / args is NULL", "NULL model + struct_size")
        said(lib.mmdx_palette_bounds(dm.h, None), INVALID, "model / args is NULL", "NULL args")
        said(call(pbounds_args(None, None, 0x80000000, reserved0=1, size=4)), INVALID, "mmdx_palette_bounds_args.struct_size mismatch", "struct_size + rest")
        said(call(pbounds_args(None, None, 0x80000000, reserved0=1)), INVALID, "unknown flag bits in mmdx_palette_bounds_args.flags",
             "unknown bits + reserved0 + NULL operands: the bits answer")
        said(call(pbounds_args(None, None, 0, reserved0=1)), INVALID, "mmdx_palette_bounds_args.reserved0 must be 0", "reserved0 + NULL operands")
        accepted(call(pbounds_args(None, None, 0, n=0)), "no instances: nothing to do, even on a host-only model")
        said(call(pbounds_args(pal, None, 0, pos_scale=0.0)), INVALID, "palettes / out_bounds is NULL", "NULL out_bounds + pos_scale")
        said(call(pbounds_args(pal, out, 0, pos_scale=0.0)), INVALID, "mmdx_palette_bounds_args.pos_scale must be finite and > 0", "pos_scale")
        said(call(pbounds_args(pal, pal + 8, 0)), INVALID, "palettes overlaps out_bounds", "overlap")
        said(call(pbounds_args(pal, out + 2, OUT)), INVALID, "device out_bounds must be 4-byte aligned", "alignment")
        said(call(pbounds_args(pal, out, 0)), NO_DEVICE, HOST_ONLY, "host-only model, a good call with host operands")
        said(call(pbounds_args(pal, out, PAL | OUT)), NO_DEVICE, HOST_ONLY, "host-only model, a good call with device flags")


def test_cull_bounds_on_a_host_only_model_bits_before_nulls_the_model_last(hip_lib):
    lib, h = hip_lib, HostArrays()
    view = make_cull_view(planes=[(0, 0, 1, 100)])
    vp = C.addressof(view)
    with DeformModel(model(), host_only=True) as dm:
        call = lambda a: lib.mmdx_cull_bounds(dm.h, C.byref(a))                       # noqa: E731
        b, ids, counts = h.ptr("bounds"), h.ptr("cull_ids"), h.ptr("cull_counts")
        said(lib.mmdx_cull_bounds(None, C.byref(cull_args(b, vp, ids, counts, size=4))), INVALID, "model / args is NULL", "NULL model + struct_size")
        said(lib.mmdx_cull_bounds(dm.h, None), INVALID, "model / args is NULL", "NULL args")
        said(call(cull_args(None, None, None, None, flags=2, size=4)), INVALID, "mmdx_cull_args.struct_size mismatch", "struct_size + rest")
        said(call(cull_args(None, None, None, None, flags=2)), INVALID, "unknown bits in mmdx_cull_args.flags",
             "unknown bits + NULL operands: the bits answer")
        said(call(cull_args(b, None, ids, counts, stride=1)), INVALID, "bounds / view / out_ids / out_counts is NULL", "NULL view + list_stride")
        said(call(cull_args(b, vp, ids, counts, stride=1)), INVALID, "mmdx_cull_args.list_stride is smaller than n_instances", "list_stride")
        said(call(cull_args(b + 2, vp, ids, counts)), INVALID, "device pointers of mmdx_cull_args must be 4-byte aligned", "alignment")
        bad_view = make_cull_view(planes=[(0, 0, 1, 100)], n_lods=5)
        said(call(cull_args(b, C.addressof(bad_view), ids, counts)), INVALID, "mmdx_cull_view.n_lods = 5 (1..4)", "a host view's n_lods")
        said(call(cull_args(b, vp, ids, counts)), NO_DEVICE, HOST_ONLY, "host-only model, a good call")


def test_instance_list_of_the_rig_form_header_then_placement_then_ids(hip_lib):
    """mmdx_skeleton_solve_select decides its list before it looks for a device: the list's own refusals in their order, each by a
    list that also violates everything behind it, and the call's own checks ahead of them (NULLs, then operand bits, then unknown
    bits -- a call that violates all three names the NULL)."""
    lib, h = hip_lib, HostArrays()
    rest, parent, level, flags = synth.make_skeleton(NB, 1)
    sk = vmd.Skeleton(rest, parent, level, flags)
    poses = np.zeros((NI, NB, 8), np.float32)
    dev = POSES | OUT

    def call(s, fl=dev, p=poses.ctypes.data):
        return lib.mmdx_skeleton_solve_select(sk.h, None, NI, p, None, fl, C.byref(s) if s is not None else None, h.ptr("placed"))

    far = np.array([1, 7, 9], np.uint32)
    worst = select(None, 3, size=4, flags=0x10, reserved0=1)
    said(call(worst, fl=0x80000000, p=None), INVALID, "NULL argument or n_instances == 0", "NULL poses + operand bits + unknown bits")
    said(call(worst, fl=0x80000000 | POSES), INVALID, SOLVE_SELECT_OPERANDS, "operand bits + unknown bits + a bad list")
    said(call(worst, fl=0x80000000 | dev), INVALID, "unknown flag bits", "unknown bits + a bad list")
    said(call(None), INVALID, "select is NULL (mmdx_skeleton_solve / _morphed solve every instance)", "NULL select")
    said(call(worst), INVALID, LIST_SIZE, "list: struct_size + flags + reserved0 + NULL ids")
    said(call(select(None, 3, flags=0x10, reserved0=1)), INVALID, LIST_BITS, "list: flags + reserved0 + NULL ids")
    said(call(select(None, 3, reserved0=1)), INVALID, LIST_RESERVED, "list: reserved0 + NULL ids")
    said(call(select(None, 3)), INVALID, LIST_NULL, "list: NULL ids")
    said(call(select(far.ctypes.data + 2, 3, on_device=True)), INVALID, LIST_ALIGN, "device list: alignment")
    said(call(select(far.ctypes.data, 3)), INVALID, "mmdx_instance_select.ids[1] = 7 is not below n_instances", "host list: ids[1] and ids[2] too large")
    two = np.array([2], np.uint32)
    said(call(select(far.ctypes.data, 3, count=two.ctypes.data)), INVALID, "mmdx_instance_select.ids[1] = 7 is not below n_instances",
         "host list: the count cuts ids[2] off, not ids[1]")
    sk.close()


# ---- on the GPU -----------------------------------------------------------------------------------------------------------------
class Crowd:
    """The operands of every call in host memory and in DeviceBuffers, and the calls over them: call(name, **which side)."""

    def __init__(self, dm, n=NI):
        self.dm, self.n, self.h = dm, n, HostArrays(n)
        self.d = {k: DeviceBuffer.from_numpy(a) for k, a in self.h.a.items()}
        self.view = make_cull_view(planes=[(0, 0, 1, 100)])

    def at(self, name, host=()):
        return self.h.ptr(name) if name in host else self.d[name].ptr

    def flags(self, host, pairs):
        f = 0
        for name, bit in pairs:
            f |= 0 if name in host else bit
        return f

    def deform(self, form, host=(), list_dev=True, sel=None, flags=None):
        lib = api.lib()
        f = self.flags(host, (("pal", PAL), ("w", WEIGHTS), ("out_a", OUT))) if flags is None else flags
        out_b = self.at("out_b", ("out_b",) if "out_a" in host else ())
        a = deform_args(self.at("w", host), self.at("pal", host), self.at("out_a", host), out_b, f, n=self.n)
        if form == "plain":
            return lib.mmdx_deform_batched(self.dm.h, C.byref(a))
        if form == "bounds":
            return lib.mmdx_deform_batched_bounds(self.dm.h, C.byref(a), self.at("bounds", ("bounds",) if "out_a" in host else ()))
        if sel is None:
            side = () if list_dev else ("ids", "count")
            sel = select(self.at("ids", side), NI, self.at("count", side), on_device=list_dev)
        return lib.mmdx_deform_batched_select(self.dm.h, C.byref(a), C.byref(sel), None)

    def place(self, host=()):
        a = place_args(self.at("pal", host), self.at("place", host), self.at("placed", host),
                       self.flags(host, (("pal", PAL), ("place", PLACE), ("placed", OUT))), n=self.n)
        return api.lib().mmdx_palette_place(self.dm.h, C.byref(a))

    def pbounds(self, host=()):
        a = pbounds_args(self.at("pal", host), self.at("bounds", host), self.flags(host, (("pal", PAL), ("bounds", OUT))), n=self.n)
        return api.lib().mmdx_palette_bounds(self.dm.h, C.byref(a))

    def cull(self, host=()):
        view = C.addressof(self.view)
        a = cull_args(self.d["bounds"].ptr, view, self.d["cull_ids"].ptr, self.d["cull_counts"].ptr, n=self.n, stride=self.n)
        return api.lib().mmdx_cull_bounds(self.dm.h, C.byref(a))

    def free(self):
        for b in self.d.values():
            b.free()


def on_another_thread(call):
    got = []
    t = threading.Thread(target=lambda: got.append((call(), api.lib().mmdx_last_error_string().decode())))
    t.start()
    t.join()
    return got[0]


@pytest.mark.gpu
def test_gpu_model_calls_while_recording(hip_lib):
    assert device_count() >= 1, "no HIP device visible: the GPU tests must run on the MI355X box"
    with DeformModel(model()) as dm:
        assert dm.ns > 0, "the model's morph must reach the kernels, or MMDX_WEIGHTS_ON_DEVICE would not matter"
        print("device_bytes", dm.info.device_bytes)
        c = Crowd(dm)
        every = [("deform_batched", lambda host=(): c.deform("plain", host), ("pal", "w", "out_a"), OPERANDS),
                 ("deform_batched_bounds", lambda host=(): c.deform("bounds", host), ("pal", "w", "out_a"), OPERANDS),
                 ("deform_batched_select", lambda host=(): c.deform("select", host), ("pal", "w", "out_a"), DEFORM_SELECT_OPERANDS),
                 ("palette_place", c.place, ("pal", "place", "placed"), PLACE_OPERANDS),
                 ("palette_bounds", c.pbounds, ("pal", "bounds"), PBOUNDS_OPERANDS),
                 ("cull_bounds", c.cull, (), None)]
        # outside a recording: the checks of the deform calls a host-only model never reaches, in their order
        said(c.deform("plain", flags=0x80000000 | PAL | OUT, host=("pal",)), INVALID, "unknown bits in mmdx_deform_args.flags",
             "deform: unknown bits answer ahead of operands")
        a = deform_args(None, None, None, None, 0x80000000 | PAL | WEIGHTS | OUT)
        said(hip_lib.mmdx_deform_batched(dm.h, C.byref(a)), INVALID, "unknown bits in mmdx_deform_args.flags", "deform: unknown bits + NULL operands")
        a = deform_args(None, None, None, None, PAL | WEIGHTS | OUT)
        worst = select(None, NI, size=4, flags=0x10, reserved0=1)
        said(hip_lib.mmdx_deform_batched_select(dm.h, C.byref(a), C.byref(worst), None), INVALID, "palettes / out_a / out_b is NULL",
             "select: NULL operands answer ahead of the list")
        ids = c.h.ptr("ids")
        for sel, text, what in ((worst, LIST_SIZE, "struct_size + flags + reserved0 + NULL ids"),
                                (select(None, NI, flags=0x10, reserved0=1), LIST_BITS, "flags + reserved0 + NULL ids"),
                                (select(None, NI, reserved0=1), LIST_RESERVED, "reserved0 + NULL ids"),
                                (select(None, NI), LIST_NULL, "NULL ids"),
                                (select(c.d["ids"].ptr + 2, NI, on_device=True), LIST_ALIGN, "device list: alignment"),
                                (select(c.d["ids"].ptr, NI), LIST_IN_DEVICE_MEMORY, "host-flagged list in device memory"),
                                (select(ids, NI, c.d["count"].ptr), LIST_IN_DEVICE_MEMORY, "host-flagged list, its count in device memory")):
            said(c.deform("select", sel=sel), INVALID, text, f"deform_select list: {what}")
        far = np.array([1, 7, 9], np.uint32)
        said(c.deform("select", sel=select(far.ctypes.data, 3)), INVALID, "mmdx_instance_select.ids[1] = 7 is not below n_instances",
             "deform_select list: ids[1] and ids[2] too large")
        #    ... and the operands check sits between the list's header and its placement
        said(c.deform("select", host=("pal",), sel=select(None, NI)), INVALID, LIST_NULL, "deform_select: NULL ids + host palettes")
        said(c.deform("select", host=("pal",), sel=select(c.d["ids"].ptr + 2, NI, on_device=True)), INVALID, DEFORM_SELECT_OPERANDS,
             "deform_select: host palettes + misaligned device list")
        # every call once outside a recording, host operands and device operands: sizes the scratch
        for name, call, operands, _ in every:
            if name != "deform_batched_select":                           # (device operands only, recording or not)
                accepted(call(host=operands), f"eager, host operands: {name}")
            accepted(call(), f"eager, device operands: {name}")
        accepted(c.deform("select", list_dev=False), "eager: deform_batched_select with a host list")
        dm.sync()
        rest, parent, level, flags = synth.make_skeleton(NB, 1)
        sk = vmd.Skeleton(rest, parent, level, flags)
        poses = DeviceBuffer.from_numpy(np.zeros((NI, NB, 8), np.float32))
        dm.graph_begin()
        for name, call, operands, text in every:
            for k in operands:
                said(call(host=(k,)), INVALID, text, f"recording, {k} on the host: {name}")
            accepted(call(), f"recording, device operands: {name}")
        accepted(c.cull(), "recording: cull_bounds with its view in host memory (read at the call)")
        said(c.deform("select", list_dev=False), INVALID, HOST_LIST, "recording: deform_batched_select with a host list")
        said(c.deform("select", sel=select(c.d["ids"].ptr, NI, c.d["count"].ptr)), INVALID, HOST_LIST,
             "recording: deform_batched_select, host-flagged list in device memory")
        st = hip_lib.mmdx_skeleton_solve_select(sk.h, dm.h, NI, poses.ptr, None, POSES | OUT,
                                                C.byref(select(c.d["ids"].ptr, NI, c.d["count"].ptr)), c.d["placed"].ptr)
        said(st, INVALID, HOST_LIST, "recording: skeleton_solve_select, host-flagged list in device memory")
        for name, call in (("palette_place", c.place), ("palette_bounds", c.pbounds), ("cull_bounds", c.cull)):
            st, msg = on_another_thread(call)
            print(f"second thread: {name}: status {st}: {msg}")
            assert st == INVALID and msg == OTHER_THREAD, (name, st, msg)
        dm.graph_end().close()                                            # closable after all these refusals
        dm.sync()
        sk.close()
        poses.free()
        c.free()


@pytest.mark.gpu
def test_gpu_morph_motion_eval_while_recording(hip_lib):
    assert device_count() >= 1, "no HIP device visible: the GPU tests must run on the MI355X box"
    lib, big = hip_lib, 16
    v = vmd.Vmd(vmd.write_vmd([], [("m", 0, 0.25), ("m", 20, 1.0)]))
    h, hb = HostArrays(), HostArrays(big)
    d = {k: DeviceBuffer.from_numpy(hb.a[k]) for k in ("frames", "times", "morphs")}
    with DeformModel(model()) as dm:
        for fn, clock in ((lib.mmdx_morph_motion_eval, "frames"), (lib.mmdx_morph_motion_eval_time, "times")):
            mm = v.bind_morphs(["m"])

            def call(host=(), n=NI, src=h):
                return fn(mm.h, dm.h, n, src.ptr(clock) if "clock" in host else d[clock].ptr, (0 if "clock" in host else FR) |
                          (0 if "out" in host else OUT), src.ptr("morphs") if "out" in host else d["morphs"].ptr)

            what = fn.__name__
            dm.graph_begin()
            said(call(host=("clock",)), INVALID, OPERANDS, f"{what}: first use, recording, host clock: the operands answer first")
            said(call(), INVALID, FIRST_USE, f"{what}: first use while recording")
            dm.graph_end().close()
            accepted(call(host=("clock", "out")), f"{what}: one plain call")
            dm.graph_begin()
            said(call(host=("clock",)), INVALID, OPERANDS, f"{what}: recording, host clock")
            said(call(host=("out",)), INVALID, OPERANDS, f"{what}: recording, host output")
            accepted(call(), f"{what}: recording, device operands")
            g = dm.graph_end()
            # the graph holds the motion's tables and scratch: more instances than any call before would have to grow them
            said(call(host=("clock",), n=big, src=hb), INVALID, "morph motion frame scratch" + WOULD_GROW, f"{what}: pinned, host clock")
            said(call(host=("out",), n=big, src=hb), INVALID, "morph motion output scratch" + WOULD_GROW, f"{what}: pinned, host output")
            accepted(call(host=("clock", "out")), f"{what}: pinned, the shape it was sized for")
            g.close()
            accepted(call(host=("clock", "out"), n=big, src=hb), f"{what}: the graph is gone, the scratch grows")
            dm.sync()
            mm.close()
    for b in d.values():
        b.free()
    v.close()

"""What the bone-track, skeleton, motion-set and cross-fade calls refuse while a graph is being recorded on a model's stream, and
what they accept.  Every text below is the library's own (csrc/rig_api.cpp), every refusal is status 1, and a refused call leaves
the recording closable.

Smallest shapes that reach every branch: 2 instances; a 3-bone parallel-FK skeleton; a 3-bone skeleton with one append bone,
which takes the ordered solver and so the two-launch form of the track + solve calls (both with bone morphs); one VMD with 2 bone
tracks and 1 morph track; a 2-clip set with both sides; every device operand a real DeviceBuffer.  Three states of the handles:
  1. none has run on the device: the all-device call is refused with the "... before" wording, host sides likewise;
  2. every call runs once outside a recording;
  3. recording again: a host operand, a host output or a host list is still refused, the all-device call is accepted, and a
     skeleton that never ran is refused next to a motion / set that did.
Nothing is replayed and nothing is compared numerically: tests/test_graph.py and the suites of the single calls do that."""
import ctypes as C

import numpy as np
import pytest

from simple_mmd_renderer_amd import _capi as api
from simple_mmd_renderer_amd import synth, vmd
from simple_mmd_renderer_amd.engine import DeformModel, DeviceBuffer, device_count

NI, NB = 2, 3
FR, OUT, POSES, WEIGHTS = vmd.FRAMES_ON_DEVICE, api.OUT_ON_DEVICE, vmd.POSES_ON_DEVICE, api.WEIGHTS_ON_DEVICE

OPERANDS = "while a graph is being recorded every operand must be in device memory"
MOTION = OPERANDS + " and the motion must have run on this device before"
SKELETON = OPERANDS + ", the skeleton must have run on this device before, and physics overrides (host lists) are not recordable"
MOTION_SKELETON = OPERANDS + " and the motion and the skeleton must have run on this device before"
SET = OPERANDS + " and the motion set must have run on this device before"
SET_SKELETON = OPERANDS + " and the motion set and the skeleton must have run on this device before"
SIZE_MOTION = "run the call once before recording: it sizes the motion's pose buffer"
SIZE_SET = "run the call once before recording: it sizes the motion set's pose buffer"
SELECT_SKELETON = "while a graph is being recorded the skeleton must have run on this device before"
HOST_LIST = "while a graph is being recorded the instance list must be in device memory (MMDX_SELECT_ON_DEVICE)"

OUTPUTS = ("out_poses", "palettes", "morphs")
HOST_IO = [(False, True, True), (True, False, True), (False, False, True)]    # host inputs, host output, both
HOST_IDS = [(True, True, False)]                                              # the select forms: a host list


def skeleton(append):
    rest, parent, level, flags = synth.make_skeleton(NB, 1)
    flags = flags.copy()
    if append:
        flags[2] |= 0x0100                                        # MMDX_BONE_APPEND_ROTATE: bone 2 inherits half of bone 1's rotation
    sk = vmd.Skeleton(rest, parent, level, flags, np.array([-1, -1, 1], np.int32), np.array([0, 0, 0.5], np.float32),
                      morphs=synth.make_bone_morphs(NB, 90))
    assert sk.info["solver"] == (vmd.SOLVER_SERIAL if append else vmd.SOLVER_PARALLEL_FK) and sk.info["n_bone_morph_entries"] > 0
    return sk


class Handles:
    """One binding of the VMD, the set over it, and the two skeletons: none of them has run on a device."""

    def __init__(self):
        names = ["b0", "b1", "b2"]
        self.v = vmd.Vmd(vmd.write_vmd(synth.make_bone_keys(names[:2], 3, keys_per=3, span=30), [("m", 0, 0.25), ("m", 20, 1.0)]))
        self.bm, self.mm = self.v.bind_bones(names), self.v.bind_morphs(["m"])
        self.set = vmd.MotionSet([self.bm, self.bm], [self.mm, self.mm])
        self.fk, self.ik = skeleton(False), skeleton(True)

    def close(self):
        for h in (self.fk, self.ik, self.set, self.bm, self.mm, self.v):
            h.close()


class Operands:
    """Every operand and output array twice, in host memory and in a DeviceBuffer."""

    def __init__(self, n_rates):
        self.host = dict(frames=np.array([3, 17], np.uint32), times=np.array([0.1, 0.5]), times_b=np.array([0.3, 0.0]),
                         clips=np.array([0, 1], np.uint32), clips_b=np.array([1, vmd.CLIP_NONE], np.uint32),
                         weights=np.array([0.25, 1.0], np.float32), poses=np.zeros((NI, NB, 8), np.float32),
                         rates=np.zeros((NI, n_rates), np.float32), ids=np.array([1, 0], np.uint32), count=np.array([2], np.uint32),
                         out_poses=np.zeros((NI, NB, 8), np.float32), palettes=np.zeros((NI, NB, 16), np.float32),
                         morphs=np.zeros((NI, 1), np.float32))
        self.host["poses"][..., 7] = 1.0
        self.dev = {k: DeviceBuffer.from_numpy(a) for k, a in self.host.items()}

    def at(self, inputs_dev, out_dev=True):
        """name -> address: the inputs on one side, the outputs on one side."""
        return {k: (self.dev[k].ptr if (out_dev if k in OUTPUTS else inputs_dev) else a.ctypes.data) for k, a in self.host.items()}

    def free(self):
        for b in self.dev.values():
            b.free()


def calls(h, ops, model, sk):
    """Every entry point, with skeleton `sk` where one is taken, as
    (name, call(inputs on device, output on device, list on device) -> status, the one-launch call's wording when nothing ran,
     its host variants, the wording of a two-launch call whose pose buffer was never sized, of its track half, of the solve)."""
    lib = api.lib()

    def flags(i, o):
        return (FR if i else 0) | (OUT if o else 0)

    def blend_args(p, i, o):
        return vmd.MotionBlendArgs(C.sizeof(vmd.MotionBlendArgs), NI, p["clips"], p["clips_b"], p["times"], p["times_b"], p["weights"],
                                   flags(i, o))

    def clock(fn, handles, key, out):                             # fn(handles..., model, n, clock, flags, out)
        return lambda i, o, l: fn(*handles, model.h, NI, ops.at(i, o)[key], flags(i, o), ops.at(i, o)[out])

    def set_clock(fn, handles, key, out):                         # fn(handles..., model, n, clips, clock, flags, out)
        return lambda i, o, l: fn(*handles, model.h, NI, ops.at(i, o)["clips"], ops.at(i, o)[key], flags(i, o), ops.at(i, o)[out])

    def blend(fn, handles, out):
        return lambda i, o, l: fn(*handles, model.h, C.byref(blend_args(ops.at(i, o), i, o)), ops.at(i, o)[out])

    def select(l):
        s = ops.at(l)
        return vmd.instance_select(s["ids"], NI, s["count"], on_device=l)

    def blend_select(fn, handles, out):                           # device operands only; the list on either side
        return lambda i, o, l: fn(*handles, model.h, C.byref(blend_args(ops.at(True), True, True)), C.byref(select(l)), ops.at(True)[out])

    def solve(i, o, l):
        p = ops.at(i, o)
        return lib.mmdx_skeleton_solve(sk.h, model.h, NI, p["poses"], (POSES if i else 0) | (OUT if o else 0), p["palettes"])

    def morphed(i, o, l):                                         # i == "rates": the poses on the device, the rates alone on the host
        w = i is True
        return lib.mmdx_skeleton_solve_morphed(sk.h, model.h, NI, ops.at(bool(i))["poses"], ops.at(w)["rates"],
                                               (POSES if i else 0) | (WEIGHTS if w else 0) | (OUT if o else 0), ops.at(i, o)["palettes"])

    def solve_select(i, o, l):
        p = ops.at(True)
        return lib.mmdx_skeleton_solve_select(sk.h, model.h, NI, p["poses"], None, POSES | OUT, C.byref(select(l)), p["palettes"])

    m, st, both = (h.bm.h,), (h.set.h,), (sk.h, h.set.h)
    return [
        ("bone_motion_eval", clock(lib.mmdx_bone_motion_eval, m, "frames", "out_poses"), MOTION, HOST_IO, None, None, None),
        ("bone_motion_eval_time", clock(lib.mmdx_bone_motion_eval_time, m, "times", "out_poses"), MOTION, HOST_IO, None, None, None),
        ("skeleton_solve", solve, SKELETON, HOST_IO, None, None, SKELETON),
        ("skeleton_solve_morphed", morphed, SKELETON, HOST_IO + [("rates", True, True)], None, None, SKELETON),
        ("skeleton_solve_select", solve_select, SELECT_SKELETON, HOST_IDS, None, None, SELECT_SKELETON),
        ("skeleton_solve_motion", clock(lib.mmdx_skeleton_solve_motion, (sk.h, h.bm.h), "frames", "palettes"), MOTION_SKELETON, HOST_IO,
         SIZE_MOTION, MOTION, SKELETON),
        ("skeleton_solve_motion_time", clock(lib.mmdx_skeleton_solve_motion_time, (sk.h, h.bm.h), "times", "palettes"), MOTION_SKELETON,
         HOST_IO, SIZE_MOTION, MOTION, SKELETON),
        ("motion_set_eval_bones", set_clock(lib.mmdx_motion_set_eval_bones, st, "frames", "out_poses"), SET, HOST_IO, None, None, None),
        ("motion_set_eval_bones_time", set_clock(lib.mmdx_motion_set_eval_bones_time, st, "times", "out_poses"), SET, HOST_IO, None, None,
         None),
        ("motion_set_eval_morphs", set_clock(lib.mmdx_motion_set_eval_morphs, st, "frames", "morphs"), SET, HOST_IO, None, None, None),
        ("motion_set_eval_morphs_time", set_clock(lib.mmdx_motion_set_eval_morphs_time, st, "times", "morphs"), SET, HOST_IO, None, None,
         None),
        ("skeleton_solve_motion_set", set_clock(lib.mmdx_skeleton_solve_motion_set, both, "frames", "palettes"), SET_SKELETON, HOST_IO,
         SIZE_SET, SET, SKELETON),
        ("skeleton_solve_motion_set_time", set_clock(lib.mmdx_skeleton_solve_motion_set_time, both, "times", "palettes"), SET_SKELETON,
         HOST_IO, SIZE_SET, SET, SKELETON),
        ("motion_set_blend_bones_time", blend(lib.mmdx_motion_set_blend_bones_time, st, "out_poses"), SET, HOST_IO, None, None, None),
        ("motion_set_blend_morphs_time", blend(lib.mmdx_motion_set_blend_morphs_time, st, "morphs"), SET, HOST_IO, None, None, None),
        ("skeleton_solve_motion_set_blend_time", blend(lib.mmdx_skeleton_solve_motion_set_blend_time, both, "palettes"), SET_SKELETON,
         HOST_IO, SIZE_SET, SET, SKELETON),
        ("motion_set_blend_bones_time_select", blend_select(lib.mmdx_motion_set_blend_bones_time_select, st, "out_poses"), SET, HOST_IDS,
         None, None, None),
        ("motion_set_blend_morphs_time_select", blend_select(lib.mmdx_motion_set_blend_morphs_time_select, st, "morphs"), SET, HOST_IDS,
         None, None, None),
        ("skeleton_solve_motion_set_blend_time_select", blend_select(lib.mmdx_skeleton_solve_motion_set_blend_time_select, both, "palettes"),
         SET_SKELETON, HOST_IDS, SIZE_SET, SET, SELECT_SKELETON),
    ]


def refused(call, args, wording, what):
    st = call(*args)
    msg = api.lib().mmdx_last_error_string().decode()
    print(f"{what} {args}: status {st}: {msg}")
    assert st == 1 and wording in msg and "record" in msg, (what, args, wording)


def accepted(call, what):
    st = call(True, True, True)
    assert st == 0, (what, st, api.lib().mmdx_last_error_string().decode())


@pytest.mark.gpu
def test_gpu_recording_refusals_and_acceptance_of_every_rig_call(hip_lib):
    assert device_count() >= 1, "no HIP device visible: the GPU tests must run on the MI355X box"
    h, spare = Handles(), Handles()                                # spare: its skeletons stay off the device throughout
    ops = Operands(h.fk.nm)
    with DeformModel(synth.make_model(120, 4, 2, 10, seed=1)) as dm:
        # (rig, row): every call on the FK skeleton, and on the append skeleton those that take a skeleton
        every = [("fk", row) for row in calls(h, ops, dm, h.fk)] + [("ik", row) for row in calls(h, ops, dm, h.ik) if row[6]]
        # 1. nothing has run on the device.  A one-launch call has one wording for a host side and for a handle that never ran; a
        #    two-launch call answers with its pose buffer before it looks at the operands; a host list is refused ahead of both.
        dm.graph_begin()
        for rig, (name, call, one, host, size, track, solver) in every:
            never = size if rig == "ik" and size else one
            refused(call, (True, True, True), never, f"never ran: {rig} {name}")
            for args in host:
                refused(call, args, never if args[2] else HOST_LIST, f"never ran: {rig} {name}")
        dm.graph_end().close()
        # 2. once outside a recording
        for rig, (name, call, *_) in every:
            accepted(call, f"eager: {rig} {name}")
        dm.sync()
        # 3. recording again.  The halves of a two-launch call answer for themselves: the track call for host inputs, and the solve for
        #    a host output, after the track call was recorded.
        dm.graph_begin()
        for rig, (name, call, one, host, size, track, solver) in every:
            for args in host:
                want = HOST_LIST if not args[2] else one if not (rig == "ik" and size) else track if not args[0] else solver
                refused(call, args, want, f"ran before: {rig} {name}")
            accepted(call, f"recorded: {rig} {name}")
        #    ... and next to a motion / set that ran, a skeleton that did not: the one-launch call refuses it itself; on the append
        #    skeleton the pose buffer is sized by now, the track call is recorded and the solve behind it refuses
        for rig, sk in (("fk", spare.fk), ("ik", spare.ik)):
            for name, call, one, host, size, track, solver in calls(h, ops, dm, sk):
                if solver:
                    refused(call, (True, True, True), solver if rig == "ik" and size else one, f"only the skeleton never ran: {rig} {name}")
        dm.graph_end().close()
        dm.sync()
    ops.free()
    for x in (h, spare):
        x.close()

"""VMD motion files: a writer for synthetic fixtures and the Python face of the C-ABI loader /
device evaluator (csrc/vmd.cpp + morph_track_eval_kernel).

File layout as the reference's reader consumes it (L/reader/vmd_reader_impl.inl:9-79,
L/reader/interprete/vmd_types.inl:17-37): 50-byte header, u32 count + 111-byte bone records,
u32 count + 23-byte morph records; names are Shift-JIS in 15-byte fields.
"""
from __future__ import annotations

import ctypes as C
import struct
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import _capi as api

MAGIC = b"Vocaloid Motion Data 0002"


def _name15(name: str) -> bytes:
    b = name.encode("shift_jis")
    if len(b) > 15:
        raise ValueError("VMD names are at most 15 bytes of Shift-JIS: %r" % name)
    return b + b"\0" * (15 - len(b))


def write_vmd(bone_keys: Sequence[tuple], morph_keys: Sequence[Tuple[str, int, float]],
              model_name: str = "synthetic") -> bytes:
    """bone_keys: (name, frame, (tx,ty,tz), (qx,qy,qz,qw), interpolation[64] or None);
    morph_keys: (name, frame, weight).  Records are written in the given order (a later record for
    the same (name, frame) wins, as in the reference)."""
    out = bytearray()
    out += MAGIC + b"\0" * (30 - len(MAGIC))
    mn = model_name.encode("shift_jis")[:20]
    out += mn + b"\0" * (20 - len(mn))
    out += struct.pack("<I", len(bone_keys))
    for name, frame, t, q, interp in bone_keys:
        out += _name15(name) + struct.pack("<I", frame) + struct.pack("<3f", *t) + struct.pack("<4f", *q)
        ip = bytes(interp) if interp is not None else bytes([20, 20, 0, 0, 20, 20, 20, 20, 107, 107, 107, 107,
                                                               107, 107, 107, 107] * 4)
        assert len(ip) == 64
        out += ip
    out += struct.pack("<I", len(morph_keys))
    for name, frame, w in morph_keys:
        out += _name15(name) + struct.pack("<I", frame) + np.float32(w).tobytes()
    out += struct.pack("<I", 0) * 3        # camera, light, self-shadow sections: empty
    return bytes(out)


class VmdInfo(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("n_bone_records", C.c_uint32), ("n_morph_records", C.c_uint32),
                ("n_bone_tracks", C.c_uint32), ("n_morph_tracks", C.c_uint32), ("n_bone_keys", C.c_uint32),
                ("n_morph_keys", C.c_uint32), ("max_frame", C.c_uint32), ("bytes_consumed", C.c_uint64)]


class VmdBoneKey(C.Structure):
    _fields_ = [("frame", C.c_uint32), ("translation", C.c_float * 3), ("rotation", C.c_float * 4),
                ("interpolation", C.c_int8 * 64)]


class Vmd:
    """A parsed VMD motion (mmdx_vmd_t)."""

    def __init__(self, source):
        lib = api.lib()
        self.h = C.c_void_p()
        if isinstance(source, (bytes, bytearray)):
            buf = (C.c_char * len(source)).from_buffer_copy(bytes(source))
            api.check(lib.mmdx_vmd_parse(buf, len(source), C.byref(self.h)))
        else:
            api.check(lib.mmdx_vmd_load_file(str(source).encode("utf-8"), C.byref(self.h)))
        info = VmdInfo()
        info.struct_size = C.sizeof(VmdInfo)
        api.check(lib.mmdx_vmd_get_info(self.h, C.byref(info)))
        self.info = {k: getattr(info, k) for k, _ in VmdInfo._fields_}

    def close(self):
        if getattr(self, "h", None):
            api.lib().mmdx_vmd_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _name(self, is_morph: int, i: int) -> str:
        buf = C.create_string_buffer(256)
        api.check(api.lib().mmdx_vmd_track_name(self.h, is_morph, i, buf, 256))
        return buf.value.decode("utf-8", "replace")

    @property
    def morph_track_names(self) -> List[str]:
        return [self._name(1, i) for i in range(self.info["n_morph_tracks"])]

    @property
    def bone_track_names(self) -> List[str]:
        return [self._name(0, i) for i in range(self.info["n_bone_tracks"])]

    def morph_track(self, i: int) -> Tuple[np.ndarray, np.ndarray]:
        fr, w, n = C.POINTER(C.c_uint32)(), C.POINTER(C.c_float)(), C.c_uint32()
        api.check(api.lib().mmdx_vmd_morph_track(self.h, i, C.byref(fr), C.byref(w), C.byref(n)))
        k = n.value
        return (np.ctypeslib.as_array(fr, (k,)).copy() if k else np.zeros(0, np.uint32),
                np.ctypeslib.as_array(w, (k,)).copy() if k else np.zeros(0, np.float32))

    def bone_track(self, i: int) -> List[dict]:
        keys, n = C.POINTER(VmdBoneKey)(), C.c_uint32()
        api.check(api.lib().mmdx_vmd_bone_track(self.h, i, C.byref(keys), C.byref(n)))
        return [dict(frame=keys[j].frame, translation=tuple(keys[j].translation), rotation=tuple(keys[j].rotation),
                     interpolation=bytes(bytearray(keys[j].interpolation))) for j in range(n.value)]

    def bind_morphs(self, morph_names: Sequence[str]) -> "MorphMotion":
        return MorphMotion(self, morph_names)

    def bind_bones(self, bone_names: Sequence[str]) -> "BoneMotion":
        return BoneMotion(self, bone_names)


class MorphMotion:
    """Morph tracks of a motion bound to a model's morph list; evaluated on the GPU."""

    def __init__(self, vmd: Vmd, morph_names: Sequence[str]):
        enc = [n.encode("utf-8") for n in morph_names]
        arr = (C.c_char_p * max(len(enc), 1))(*enc)
        self.h = C.c_void_p()
        api.check(api.lib().mmdx_vmd_bind_morphs(vmd.h, len(enc), arr, C.byref(self.h)))
        nm, mapped, keys = C.c_uint32(), C.c_uint32(), C.c_uint32()
        api.check(api.lib().mmdx_morph_motion_get_info(self.h, C.byref(nm), C.byref(mapped), C.byref(keys)))
        self.nm, self.n_mapped, self.n_keys = nm.value, mapped.value, keys.value

    def eval(self, frames, model=None) -> np.ndarray:
        """Host convenience: frames [NI] -> rates f32 [NI, NM] (device evaluation + D2H)."""
        fr = np.ascontiguousarray(frames, np.uint32).reshape(-1)
        out = np.empty((fr.size, self.nm), np.float32)
        api.check(api.lib().mmdx_morph_motion_eval(self.h, model.h if model is not None else None, fr.size,
                                                   fr.ctypes.data, 0, out.ctypes.data))
        return out

    def eval_device(self, n_instances: int, frames_ptr, out_ptr, model=None) -> None:
        """frames u32[NI] and out f32[NI][NM] resident in HBM; asynchronous on the model's stream."""
        api.check(api.lib().mmdx_morph_motion_eval(self.h, model.h if model is not None else None, n_instances,
                                                   frames_ptr, 1 | api.OUT_ON_DEVICE, out_ptr))

    def eval_time(self, times, model=None) -> np.ndarray:
        """Host convenience: times in seconds f64 [NI] -> rates f32 [NI, NM] (MotionPlayer::SeekTime's morph half)."""
        t = np.ascontiguousarray(times, np.float64).reshape(-1)
        out = np.empty((t.size, self.nm), np.float32)
        api.check(api.lib().mmdx_morph_motion_eval_time(self.h, model.h if model is not None else None, t.size,
                                                        t.ctypes.data, 0, out.ctypes.data))
        return out

    def eval_time_device(self, n_instances: int, times_ptr, out_ptr, model=None) -> None:
        """times f64[NI] (seconds) and out f32[NI][NM] resident in HBM; asynchronous on the model's stream."""
        api.check(api.lib().mmdx_morph_motion_eval_time(self.h, model.h if model is not None else None, n_instances,
                                                        times_ptr, TIMES_ON_DEVICE | api.OUT_ON_DEVICE, out_ptr))

    def close(self):
        if getattr(self, "h", None):
            api.lib().mmdx_morph_motion_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


FRAMES_ON_DEVICE = 1 << 0
TIMES_ON_DEVICE = FRAMES_ON_DEVICE       # the same bit for the *_time entry points
POSES_ON_DEVICE = 1 << 4
POSE_FLOATS = 8


class BoneMotion:
    """Bone tracks of a motion bound to a model's bone list; local poses are evaluated on the GPU
    (Motion::GetBonePose for every (instance, bone): t.xyz, 0, q.xyzw)."""

    def __init__(self, vmd: Vmd, bone_names: Sequence[str]):
        enc = [n.encode("utf-8") for n in bone_names]
        arr = (C.c_char_p * max(len(enc), 1))(*enc)
        self.h = C.c_void_p()
        api.check(api.lib().mmdx_vmd_bind_bones(vmd.h, len(enc), arr, C.byref(self.h)))
        self._read_info()

    def _read_info(self):
        nb, mapped, keys, curves = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_uint32()
        api.check(api.lib().mmdx_bone_motion_get_info(self.h, C.byref(nb), C.byref(mapped), C.byref(keys),
                                                      C.byref(curves)))
        self.nb, self.n_mapped, self.n_keys, self.n_curves = nb.value, mapped.value, keys.value, curves.value

    def in_place(self, bone: int, axes: int) -> "BoneMotion":
        """A copy of this motion in which the translation of every key of `bone` is +0 on `axes` (api.ROOT_X | ROOT_Y | ROOT_Z;
        mmdx_bone_motion_in_place): the motion with its root motion taken out, for a crowd whose placements carry it
        (Animator.root_motion).  Everything else is the same, byte for byte."""
        out = BoneMotion.__new__(BoneMotion)
        out.h = C.c_void_p()
        api.check(api.lib().mmdx_bone_motion_in_place(self.h, bone, axes, C.byref(out.h)))
        out._read_info()
        return out

    def in_place_turn(self, bone: int, axes: int) -> "BoneMotion":
        """in_place, and every key of `bone` also gets the rotation {+0,+0,+0,1} (mmdx_bone_motion_in_place_turn): the track evaluates
        to the identity at every time, for a crowd whose placements carry the turning as well (Animator.root_turn)."""
        out = BoneMotion.__new__(BoneMotion)
        out.h = C.c_void_p()
        api.check(api.lib().mmdx_bone_motion_in_place_turn(self.h, bone, axes, C.byref(out.h)))
        out._read_info()
        return out

    def keys(self) -> Dict[str, np.ndarray]:
        """Copies of the host key tables (mmdx_bone_motion_get_keys, for tests): key_off u32 [NB+1], key_frame u32 [K], key_tr
        f32 [K, 4], key_rot f32 [K, 4], key_curve u32 [K, 4], lut f32 [n_curves, 32]."""
        k = api.BoneMotionKeys(C.sizeof(api.BoneMotionKeys))
        api.check(api.lib().mmdx_bone_motion_get_keys(self.h, C.byref(k)))

        def take(p, shape):
            return np.ctypeslib.as_array(p, shape).copy() if int(np.prod(shape)) else np.zeros(shape, p._type_)
        return dict(key_off=take(k.key_off, (k.n_bones + 1,)), key_frame=take(k.key_frame, (k.n_keys,)),
                    key_tr=take(k.key_tr, (k.n_keys, 4)), key_rot=take(k.key_rot, (k.n_keys, 4)),
                    key_curve=take(k.key_curve, (k.n_keys, 4)), lut=take(k.lut, (k.n_curves, 32)))

    def eval(self, frames, model=None) -> np.ndarray:
        """Host convenience: frames [NI] -> poses f32 [NI, NB, 8] (device evaluation + D2H)."""
        fr = np.ascontiguousarray(frames, np.uint32).reshape(-1)
        out = np.empty((fr.size, self.nb, POSE_FLOATS), np.float32)
        api.check(api.lib().mmdx_bone_motion_eval(self.h, model.h if model is not None else None, fr.size,
                                                  fr.ctypes.data, 0, out.ctypes.data))
        return out

    def eval_device(self, n_instances: int, frames_ptr, out_ptr, model=None) -> None:
        """frames u32[NI] and out f32[NI][NB][8] resident in HBM; asynchronous on the model's stream."""
        api.check(api.lib().mmdx_bone_motion_eval(self.h, model.h if model is not None else None, n_instances,
                                                  frames_ptr, FRAMES_ON_DEVICE | api.OUT_ON_DEVICE, out_ptr))

    def eval_time(self, times, model=None) -> np.ndarray:
        """Host convenience: times in seconds f64 [NI] -> poses f32 [NI, NB, 8] (Motion::GetBonePose(name, double time))."""
        t = np.ascontiguousarray(times, np.float64).reshape(-1)
        out = np.empty((t.size, self.nb, POSE_FLOATS), np.float32)
        api.check(api.lib().mmdx_bone_motion_eval_time(self.h, model.h if model is not None else None, t.size,
                                                       t.ctypes.data, 0, out.ctypes.data))
        return out

    def eval_time_device(self, n_instances: int, times_ptr, out_ptr, model=None) -> None:
        """times f64[NI] (seconds) and out f32[NI][NB][8] resident in HBM; asynchronous on the model's stream."""
        api.check(api.lib().mmdx_bone_motion_eval_time(self.h, model.h if model is not None else None, n_instances,
                                                       times_ptr, TIMES_ON_DEVICE | api.OUT_ON_DEVICE, out_ptr))

    def close(self):
        if getattr(self, "h", None):
            api.lib().mmdx_bone_motion_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


CLIP_NONE = 0xFFFFFFFF                   # MMDX_CLIP_NONE: the instance plays nothing (rest pose, all rates 0)


class MotionSetInfo(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("n_clips", C.c_uint32), ("n_bones", C.c_uint32), ("n_morphs", C.c_uint32),
                ("n_bone_keys", C.c_uint32), ("n_morph_keys", C.c_uint32), ("n_curves", C.c_uint32)]


class MotionBlendArgs(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("n_instances", C.c_uint32), ("clips_a", C.c_void_p), ("clips_b", C.c_void_p),
                ("times_a", C.c_void_p), ("times_b", C.c_void_p), ("weights", C.c_void_p), ("flags", C.c_uint32)]


def blend_args_host(clips_a, times_a, clips_b, times_b, weights):
    """mmdx_motion_blend_args over host arrays -> (args, the arrays it points into: keep them alive over the call)."""
    keep = [np.ascontiguousarray(clips_a, np.uint32).reshape(-1), np.ascontiguousarray(clips_b, np.uint32).reshape(-1),
            np.ascontiguousarray(times_a, np.float64).reshape(-1), np.ascontiguousarray(times_b, np.float64).reshape(-1),
            np.ascontiguousarray(weights, np.float32).reshape(-1)]
    if len({a.size for a in keep}) != 1:
        raise ValueError("one clip a, time a, clip b, time b and weight per instance")
    return MotionBlendArgs(C.sizeof(MotionBlendArgs), keep[0].size, *[a.ctypes.data for a in keep], 0), keep


def blend_args_device(n_instances, clips_a_ptr, times_a_ptr, clips_b_ptr, times_b_ptr, weights_ptr):
    """mmdx_motion_blend_args over five device arrays, the output on the device as well."""
    return MotionBlendArgs(C.sizeof(MotionBlendArgs), n_instances, clips_a_ptr, clips_b_ptr, times_a_ptr, times_b_ptr, weights_ptr,
                           TIMES_ON_DEVICE | api.OUT_ON_DEVICE)


def instance_select(ids_ptr, n_ids: int, count_ptr=None, on_device=True) -> "api.InstanceSelect":
    """mmdx_instance_select over a u32 list (capacity n_ids, the first *count_ptr in use; None = all) in device or host memory."""
    s = api.InstanceSelect()
    s.struct_size = C.sizeof(api.InstanceSelect)
    s.flags = api.SELECT_ON_DEVICE if on_device else 0
    s.ids, s.count, s.n_ids = ids_ptr, count_ptr, n_ids
    return s


# ---- layers: the masked blend of two evaluated pose or rate arrays (mmdx_pose_blend / mmdx_rate_blend) -----------------------
MASK_NONE = api.MASK_NONE                # MMDX_MASK_NONE: this instance blends every item at its full weight


def _blend_rows_host(fn, a, b, weights, masks, mask_ids, model, item_floats):
    a = np.ascontiguousarray(a, np.float32)
    b = np.ascontiguousarray(b, np.float32)
    if a.shape != b.shape or a.ndim != (3 if item_floats > 1 else 2) or (item_floats > 1 and a.shape[2] != item_floats):
        raise ValueError("a and b must have one shape: [NI, items, 8] for poses, [NI, items] for rates")
    ni, items = a.shape[0], a.shape[1]
    w = np.ascontiguousarray(weights, np.float32).reshape(-1)
    if w.size != ni:
        raise ValueError("one weight per instance")
    keep = [a, b, w]
    args = api.RowBlendArgs(C.sizeof(api.RowBlendArgs), 0, ni, items, a.ctypes.data, b.ctypes.data, w.ctypes.data, None, None, 0, 0, None)
    if mask_ids is not None:
        ids = np.ascontiguousarray(mask_ids, np.uint32).reshape(-1)
        if ids.size != ni:
            raise ValueError("one mask id per instance")
        m = np.ascontiguousarray(masks if masks is not None else np.zeros((0, items)), np.float32).reshape(-1, items)
        keep += [ids, m]
        args.mask_ids, args.masks, args.n_masks = ids.ctypes.data, m.ctypes.data if m.size else None, m.shape[0]
    out = np.empty_like(a)
    args.out = out.ctypes.data
    api.check(fn(model.h if model is not None else None, C.byref(args), None))
    return out


def blend_poses(a, b, weights, masks=None, mask_ids=None, model=None) -> np.ndarray:
    """Host convenience (mmdx_pose_blend; `model` is required: it supplies the device and stream): poses a, b f32 [NI, items, 8],
    weights [NI], masks f32 [n_masks, items] and mask_ids u32 [NI] (MASK_NONE = no mask; None = nobody has one) -> poses f32
    [NI, items, 8]: per item the cross-fade's blend at weights[i] * masks[mask_ids[i]][item]."""
    return _blend_rows_host(api.lib().mmdx_pose_blend, a, b, weights, masks, mask_ids, model, POSE_FLOATS)


def blend_rates(a, b, weights, masks=None, mask_ids=None, model=None) -> np.ndarray:
    """The same for morph rates (mmdx_rate_blend): a, b f32 [NI, items] -> f32 [NI, items]."""
    return _blend_rows_host(api.lib().mmdx_rate_blend, a, b, weights, masks, mask_ids, model, 1)


def _blend_rows_device(fn, n_instances, row_items, a_ptr, b_ptr, weights_ptr, out_ptr, masks_ptr, n_masks, mask_ids_ptr, model, select):
    args = api.RowBlendArgs(C.sizeof(api.RowBlendArgs),
                            api.BLEND_A_ON_DEVICE | api.BLEND_B_ON_DEVICE | api.BLEND_PARAMS_ON_DEVICE | api.OUT_ON_DEVICE,
                            n_instances, row_items, a_ptr, b_ptr, weights_ptr, mask_ids_ptr, masks_ptr, n_masks, 0, out_ptr)
    api.check(fn(model.h if model is not None else None, C.byref(args), C.byref(select) if select is not None else None))


def blend_poses_device(n_instances: int, row_items: int, a_ptr, b_ptr, weights_ptr, out_ptr, masks_ptr=None, n_masks: int = 0,
                       mask_ids_ptr=None, model=None, select=None) -> None:
    """a, b, out f32[NI][row_items][8] (out may be a or b), weights f32[NI], mask_ids u32[NI] (or None) and masks
    f32[n_masks][row_items] resident in HBM; asynchronous on the model's stream.  select: an instance_select(...) -- only the listed
    instances are blended, every other row of out keeps its bytes."""
    _blend_rows_device(api.lib().mmdx_pose_blend, n_instances, row_items, a_ptr, b_ptr, weights_ptr, out_ptr, masks_ptr, n_masks,
                       mask_ids_ptr, model, select)


def blend_rates_device(n_instances: int, row_items: int, a_ptr, b_ptr, weights_ptr, out_ptr, masks_ptr=None, n_masks: int = 0,
                       mask_ids_ptr=None, model=None, select=None) -> None:
    """The same for morph rates: a, b, out f32[NI][row_items]."""
    _blend_rows_device(api.lib().mmdx_rate_blend, n_instances, row_items, a_ptr, b_ptr, weights_ptr, out_ptr, masks_ptr, n_masks,
                       mask_ids_ptr, model, select)


# ---- additive layers: a clip's offset from its reference pose, added per bone / per morph (mmdx_pose_add / mmdx_rate_add) -----
REF_NONE = api.REF_NONE                  # MMDX_REF_NONE: this instance's B rows already are differences


def _add_rows_host(fn, a, b, weights, masks, mask_ids, refs, ref_ids, model, item_floats):
    a = np.ascontiguousarray(a, np.float32)
    b = np.ascontiguousarray(b, np.float32)
    if a.shape != b.shape or a.ndim != (3 if item_floats > 1 else 2) or (item_floats > 1 and a.shape[2] != item_floats):
        raise ValueError("a and b must have one shape: [NI, items, 8] for poses, [NI, items] for rates")
    ni, items = a.shape[0], a.shape[1]
    w = np.ascontiguousarray(weights, np.float32).reshape(-1)
    if w.size != ni:
        raise ValueError("one weight per instance")
    keep = [a, b, w]
    args = api.RowAddArgs(C.sizeof(api.RowAddArgs), 0, ni, items, a.ctypes.data, b.ctypes.data, w.ctypes.data, None, None, 0, 0, None,
                          None, None, 0, 0)
    if mask_ids is not None:
        ids = np.ascontiguousarray(mask_ids, np.uint32).reshape(-1)
        if ids.size != ni:
            raise ValueError("one mask id per instance")
        m = np.ascontiguousarray(masks if masks is not None else np.zeros((0, items)), np.float32).reshape(-1, items)
        keep += [ids, m]
        args.mask_ids, args.masks, args.n_masks = ids.ctypes.data, m.ctypes.data if m.size else None, m.shape[0]
    if ref_ids is not None:
        rids = np.ascontiguousarray(ref_ids, np.uint32).reshape(-1)
        if rids.size != ni:
            raise ValueError("one reference id per instance")
        r = np.ascontiguousarray(refs if refs is not None else np.zeros((0,) + a.shape[1:]), np.float32)
        if r.shape[1:] != a.shape[1:]:
            raise ValueError("refs must be [n_refs, items, 8] for poses, [n_refs, items] for rates")
        keep += [rids, r]
        args.ref_ids, args.refs, args.n_refs = rids.ctypes.data, r.ctypes.data if r.size else None, r.shape[0]
    out = np.empty_like(a)
    args.out = out.ctypes.data
    api.check(fn(model.h if model is not None else None, C.byref(args), None))
    return out


def add_poses(a, b, weights, masks=None, mask_ids=None, refs=None, ref_ids=None, model=None) -> np.ndarray:
    """Host convenience (mmdx_pose_add; `model` is required: it supplies the device and stream): base poses a and layer poses b f32
    [NI, items, 8], weights [NI], masks / mask_ids as blend_poses, refs f32 [n_refs, items, 8] and ref_ids u32 [NI] (REF_NONE = b
    already is a difference; None = nobody has a reference) -> poses f32 [NI, items, 8]: per item a with b's difference from its
    reference row applied at weights[i] * masks[mask_ids[i]][item], the way a bone morph is applied."""
    return _add_rows_host(api.lib().mmdx_pose_add, a, b, weights, masks, mask_ids, refs, ref_ids, model, POSE_FLOATS)


def add_rates(a, b, weights, masks=None, mask_ids=None, refs=None, ref_ids=None, model=None) -> np.ndarray:
    """The same for morph rates (mmdx_rate_add): a, b f32 [NI, items], refs f32 [n_refs, items] -> a + (b - ref) * e, f32 [NI, items]."""
    return _add_rows_host(api.lib().mmdx_rate_add, a, b, weights, masks, mask_ids, refs, ref_ids, model, 1)


def _add_rows_device(fn, n_instances, row_items, a_ptr, b_ptr, weights_ptr, out_ptr, masks_ptr, n_masks, mask_ids_ptr, refs_ptr, n_refs,
                     ref_ids_ptr, model, select):
    args = api.RowAddArgs(C.sizeof(api.RowAddArgs),
                          api.BLEND_A_ON_DEVICE | api.BLEND_B_ON_DEVICE | api.BLEND_PARAMS_ON_DEVICE | api.OUT_ON_DEVICE,
                          n_instances, row_items, a_ptr, b_ptr, weights_ptr, mask_ids_ptr, masks_ptr, n_masks, 0, out_ptr,
                          ref_ids_ptr, refs_ptr, n_refs, 0)
    api.check(fn(model.h if model is not None else None, C.byref(args), C.byref(select) if select is not None else None))


def add_poses_device(n_instances: int, row_items: int, a_ptr, b_ptr, weights_ptr, out_ptr, masks_ptr=None, n_masks: int = 0,
                     mask_ids_ptr=None, refs_ptr=None, n_refs: int = 0, ref_ids_ptr=None, model=None, select=None) -> None:
    """a, b, out f32[NI][row_items][8] (out may be a or b), weights f32[NI], mask_ids u32[NI] (or None), masks f32[n_masks][row_items],
    ref_ids u32[NI] (or None) and refs f32[n_refs][row_items][8] resident in HBM; asynchronous on the model's stream.  refs is what
    MotionSet.eval_bones_time_device writes for clips 0 .. n_refs - 1 at time 0.  select: an instance_select(...) -- only the listed
    instances are layered, every other row of out keeps its bytes."""
    _add_rows_device(api.lib().mmdx_pose_add, n_instances, row_items, a_ptr, b_ptr, weights_ptr, out_ptr, masks_ptr, n_masks,
                     mask_ids_ptr, refs_ptr, n_refs, ref_ids_ptr, model, select)


def add_rates_device(n_instances: int, row_items: int, a_ptr, b_ptr, weights_ptr, out_ptr, masks_ptr=None, n_masks: int = 0,
                     mask_ids_ptr=None, refs_ptr=None, n_refs: int = 0, ref_ids_ptr=None, model=None, select=None) -> None:
    """The same for morph rates: a, b, out f32[NI][row_items], refs f32[n_refs][row_items]."""
    _add_rows_device(api.lib().mmdx_rate_add, n_instances, row_items, a_ptr, b_ptr, weights_ptr, out_ptr, masks_ptr, n_masks,
                     mask_ids_ptr, refs_ptr, n_refs, ref_ids_ptr, model, select)


class MotionSet:
    """A bank of clips bound to one model (mmdx_motion_set_t): every instance of a crowd plays its own clip, clips[i], at its own
    frame or time.  bone_motions / morph_motions: sequences of BoneMotion / MorphMotion, one per clip, at least one of the two;
    their tables are copied, so the motions (and their Vmd) may be closed afterwards."""

    def __init__(self, bone_motions: Optional[Sequence["BoneMotion"]] = None,
                 morph_motions: Optional[Sequence["MorphMotion"]] = None):
        n = len(bone_motions) if bone_motions is not None else len(morph_motions) if morph_motions is not None else 0
        if bone_motions is not None and morph_motions is not None and len(bone_motions) != len(morph_motions):
            raise ValueError("bone_motions and morph_motions must hold one motion per clip each")

        def handles(ms):
            return (C.c_void_p * max(n, 1))(*[m.h for m in ms]) if ms is not None else None
        self.h = C.c_void_p()
        api.check(api.lib().mmdx_motion_set_create(n, handles(bone_motions), handles(morph_motions), C.byref(self.h)))
        info = MotionSetInfo()
        info.struct_size = C.sizeof(MotionSetInfo)
        api.check(api.lib().mmdx_motion_set_get_info(self.h, C.byref(info)))
        self.info = {k: getattr(info, k) for k, _ in MotionSetInfo._fields_}
        self.n_clips, self.nb, self.nm = info.n_clips, info.n_bones, info.n_morphs

    def _host(self, fn, clips, clock, dtype, row_shape, model):
        c = np.ascontiguousarray(clips, np.uint32).reshape(-1)
        t = np.ascontiguousarray(clock, dtype).reshape(-1)
        if c.size != t.size:
            raise ValueError("one clip index per instance")
        out = np.empty((c.size,) + row_shape, np.float32)
        api.check(fn(self.h, model.h if model is not None else None, c.size, c.ctypes.data, t.ctypes.data, 0, out.ctypes.data))
        return out

    def eval_bones(self, clips, frames, model=None) -> np.ndarray:
        """Host convenience: clip ids [NI], frames [NI] -> poses f32 [NI, NB, 8] (device evaluation + D2H)."""
        return self._host(api.lib().mmdx_motion_set_eval_bones, clips, frames, np.uint32, (self.nb, POSE_FLOATS), model)

    def eval_bones_time(self, clips, times, model=None) -> np.ndarray:
        """Host convenience: clip ids [NI], times in seconds f64 [NI] -> poses f32 [NI, NB, 8]."""
        return self._host(api.lib().mmdx_motion_set_eval_bones_time, clips, times, np.float64, (self.nb, POSE_FLOATS), model)

    def eval_morphs(self, clips, frames, model=None) -> np.ndarray:
        """Host convenience: clip ids [NI], frames [NI] -> rates f32 [NI, NM]."""
        return self._host(api.lib().mmdx_motion_set_eval_morphs, clips, frames, np.uint32, (self.nm,), model)

    def eval_morphs_time(self, clips, times, model=None) -> np.ndarray:
        """Host convenience: clip ids [NI], times in seconds f64 [NI] -> rates f32 [NI, NM]."""
        return self._host(api.lib().mmdx_motion_set_eval_morphs_time, clips, times, np.float64, (self.nm,), model)

    def _device(self, fn, n_instances, clips_ptr, clock_ptr, out_ptr, model):
        api.check(fn(self.h, model.h if model is not None else None, n_instances, clips_ptr, clock_ptr,
                     FRAMES_ON_DEVICE | api.OUT_ON_DEVICE, out_ptr))

    def eval_bones_device(self, n_instances: int, clips_ptr, frames_ptr, out_ptr, model=None) -> None:
        """clips u32[NI], frames u32[NI] and out f32[NI][NB][8] resident in HBM; asynchronous on the model's stream."""
        self._device(api.lib().mmdx_motion_set_eval_bones, n_instances, clips_ptr, frames_ptr, out_ptr, model)

    def eval_bones_time_device(self, n_instances: int, clips_ptr, times_ptr, out_ptr, model=None) -> None:
        """clips u32[NI], times f64[NI] (seconds) and out f32[NI][NB][8] resident in HBM."""
        self._device(api.lib().mmdx_motion_set_eval_bones_time, n_instances, clips_ptr, times_ptr, out_ptr, model)

    def eval_morphs_device(self, n_instances: int, clips_ptr, frames_ptr, out_ptr, model=None) -> None:
        """clips u32[NI], frames u32[NI] and out f32[NI][NM] resident in HBM."""
        self._device(api.lib().mmdx_motion_set_eval_morphs, n_instances, clips_ptr, frames_ptr, out_ptr, model)

    def eval_morphs_time_device(self, n_instances: int, clips_ptr, times_ptr, out_ptr, model=None) -> None:
        """clips u32[NI], times f64[NI] (seconds) and out f32[NI][NM] resident in HBM."""
        self._device(api.lib().mmdx_motion_set_eval_morphs_time, n_instances, clips_ptr, times_ptr, out_ptr, model)

    # -- cross-fade between two clips, per instance (mmdx_motion_set_blend_*_time) --------------------------------------
    def _blend_host(self, fn, clips_a, times_a, clips_b, times_b, weights, row_shape, model):
        args, keep = blend_args_host(clips_a, times_a, clips_b, times_b, weights)
        out = np.empty((args.n_instances,) + row_shape, np.float32)
        api.check(fn(self.h, model.h if model is not None else None, C.byref(args), out.ctypes.data))
        return out

    def blend_bones_time(self, clips_a, times_a, clips_b, times_b, weights, model=None) -> np.ndarray:
        """Host convenience: per instance clip a at time a, clip b at time b (seconds) and the weight of b -> poses f32
        [NI, NB, 8]: A below 1e-7, B above 1 - 1e-7, else lerp of the translations and NLerp of the rotations."""
        return self._blend_host(api.lib().mmdx_motion_set_blend_bones_time, clips_a, times_a, clips_b, times_b, weights,
                                (self.nb, POSE_FLOATS), model)

    def blend_morphs_time(self, clips_a, times_a, clips_b, times_b, weights, model=None) -> np.ndarray:
        """Host convenience: the same for morph rates -> f32 [NI, NM]."""
        return self._blend_host(api.lib().mmdx_motion_set_blend_morphs_time, clips_a, times_a, clips_b, times_b, weights,
                                (self.nm,), model)

    def blend_bones_time_device(self, n_instances: int, clips_a_ptr, times_a_ptr, clips_b_ptr, times_b_ptr, weights_ptr, out_ptr,
                                model=None) -> None:
        """clips u32[NI] x 2, times f64[NI] x 2, weights f32[NI] and out f32[NI][NB][8] resident in HBM; asynchronous."""
        args = blend_args_device(n_instances, clips_a_ptr, times_a_ptr, clips_b_ptr, times_b_ptr, weights_ptr)
        api.check(api.lib().mmdx_motion_set_blend_bones_time(self.h, model.h if model is not None else None, C.byref(args), out_ptr))

    def blend_morphs_time_device(self, n_instances: int, clips_a_ptr, times_a_ptr, clips_b_ptr, times_b_ptr, weights_ptr, out_ptr,
                                 model=None) -> None:
        """The same for morph rates: out f32[NI][NM] resident in HBM."""
        args = blend_args_device(n_instances, clips_a_ptr, times_a_ptr, clips_b_ptr, times_b_ptr, weights_ptr)
        api.check(api.lib().mmdx_motion_set_blend_morphs_time(self.h, model.h if model is not None else None, C.byref(args), out_ptr))

    # -- the cross-fade for a listed subset of the crowd (mmdx_motion_set_blend_*_time_select) ---------------------------
    def blend_bones_time_select_device(self, n_instances: int, clips_a_ptr, times_a_ptr, clips_b_ptr, times_b_ptr, weights_ptr,
                                       out_ptr, ids_ptr, n_ids: int, count_ptr=None, model=None, select_on_device=True) -> None:
        """blend_bones_time_device for the instances in the u32 list at ids_ptr only (capacity n_ids, the first *count_ptr in use;
        count_ptr None = all n_ids): the operand arrays and out f32[NI][NB][8] keep [n_instances] rows, every row that is not
        listed keeps its bytes.  List and count in device memory (asynchronous) or, with select_on_device=False, in host memory
        (the call returns when its work is done)."""
        args = blend_args_device(n_instances, clips_a_ptr, times_a_ptr, clips_b_ptr, times_b_ptr, weights_ptr)
        s = instance_select(ids_ptr, n_ids, count_ptr, select_on_device)
        api.check(api.lib().mmdx_motion_set_blend_bones_time_select(self.h, model.h if model is not None else None, C.byref(args),
                                                                    C.byref(s), out_ptr))

    def blend_morphs_time_select_device(self, n_instances: int, clips_a_ptr, times_a_ptr, clips_b_ptr, times_b_ptr, weights_ptr,
                                        out_ptr, ids_ptr, n_ids: int, count_ptr=None, model=None, select_on_device=True) -> None:
        """The same for morph rates: out f32[NI][NM] resident in HBM."""
        args = blend_args_device(n_instances, clips_a_ptr, times_a_ptr, clips_b_ptr, times_b_ptr, weights_ptr)
        s = instance_select(ids_ptr, n_ids, count_ptr, select_on_device)
        api.check(api.lib().mmdx_motion_set_blend_morphs_time_select(self.h, model.h if model is not None else None, C.byref(args),
                                                                     C.byref(s), out_ptr))

    def clip_frames(self) -> np.ndarray:
        """u32 [n_clips]: the largest key frame of every clip over the sides the set has (Motion::GetLength of those tracks);
        a clip's length in seconds is frames / 30.0."""
        out = np.zeros(self.n_clips, np.uint32)
        api.check(api.lib().mmdx_motion_set_clip_frames(self.h, out.ctypes.data))
        return out

    def close(self):
        if getattr(self, "h", None):
            api.lib().mmdx_motion_set_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---- the crowd animator (mmdx_animator_*): clocks, loops and cross-fades advanced on the device ---------------------------
ANIM_NO_REQUEST = 0xFFFFFFFE             # MMDX_ANIM_NO_REQUEST: no pending request in req_clip
ANIM_LOOP, ANIM_HOLD, ANIM_THEN = 0, 1, 2
ANIM_DT_ON_DEVICE = 1 << 10              # mmdx_animator_advance: dt is a device pointer, read when the kernel runs


class AnimatorClip(C.Structure):
    _fields_ = [("length", C.c_double), ("mode", C.c_uint32), ("next", C.c_uint32), ("fade", C.c_float), ("reserved0", C.c_uint32)]


class AnimatorDesc(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("n_instances", C.c_uint32), ("clips", C.c_void_p), ("n_clips", C.c_uint32),
                ("reserved0", C.c_uint32)]


class AnimatorInfo(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("n_instances", C.c_uint32), ("n_clips", C.c_uint32), ("device_ordinal", C.c_int32)]


# the eleven state arrays in the order of mmdx_animator_arrays, with their element types
ANIMATOR_ARRAYS = (("clips_a", np.uint32), ("clips_b", np.uint32), ("times_a", np.float64), ("times_b", np.float64),
                   ("weights", np.float32), ("speed", np.float32), ("fade_rate", np.float32), ("req_clip", np.uint32),
                   ("req_fade", np.float32), ("req_time", np.float64), ("loops", np.uint32))


class AnimatorArrays(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("n_instances", C.c_uint32)] + [(k, C.c_void_p) for k, _ in ANIMATOR_ARRAYS]


class Animator:
    """The playback state of every instance of a crowd, in device memory (mmdx_animator_t): advance() steps all clocks, loops,
    fades and pending requests with one launch, and operands() is what the three blend calls take.
    clips: None (every clip loops over its own length) or one (length, mode, next, fade) per clip of the set; length <= 0 = the
    clip's own."""

    def __init__(self, motion_set: "MotionSet", n_instances: int, clips=None):
        desc = AnimatorDesc(C.sizeof(AnimatorDesc), n_instances, None, 0, 0)
        if clips is not None:
            table = (AnimatorClip * max(len(clips), 1))(*[AnimatorClip(float(l), int(m), int(n), float(f), 0) for l, m, n, f in clips])
            desc.clips, desc.n_clips = C.addressof(table), len(clips)
        self.h = C.c_void_p()
        api.check(api.lib().mmdx_animator_create(motion_set.h, C.byref(desc), C.byref(self.h)))
        self.ni, self.n_clips = n_instances, motion_set.n_clips

    def clip_table(self) -> List[tuple]:
        """The table as resolved: (length in seconds, mode, next, fade) per clip."""
        info = AnimatorInfo(C.sizeof(AnimatorInfo))
        table = (AnimatorClip * max(self.n_clips, 1))()
        api.check(api.lib().mmdx_animator_get_info(self.h, C.byref(info), table))
        return [(table[c].length, table[c].mode, table[c].next, table[c].fade) for c in range(self.n_clips)]

    def advance(self, dt: float, model=None) -> None:
        """One step of `dt` seconds for every instance (a recorded graph freezes this dt)."""
        api.check(api.lib().mmdx_animator_advance(self.h, model.h if model is not None else None, C.byref(C.c_double(dt)), 0))

    def advance_device_dt(self, dt_ptr, model=None) -> None:
        """The same with dt a device double, read when the kernel runs: a replayed graph rewrites 8 bytes."""
        api.check(api.lib().mmdx_animator_advance(self.h, model.h if model is not None else None, dt_ptr, ANIM_DT_ON_DEVICE))

    def root_motion(self, motion_set: "MotionSet", root_bone: int, axes: int, placements_ptr, dt: Optional[float] = None, dt_ptr=None,
                    model=None) -> None:
        """Add to placements f32[NI][8] (device memory, the pose form of mmdx_palette_place) what the playing clips of `motion_set`
        move bone `root_bone` by during the step advance() is ABOUT to take, rotated by each placement's heading: call it before
        advance with the same step -- dt, a host value, or dt_ptr, a device double read when the kernel runs.  axes: api.ROOT_X |
        ROOT_Y | ROOT_Z.  Only placements[i][0..2] are written."""
        if (dt is None) == (dt_ptr is None):
            raise ValueError("give one of dt and dt_ptr")
        host = C.c_double(dt) if dt is not None else None
        args = api.RootMotionArgs(C.sizeof(api.RootMotionArgs), 0 if dt is not None else ANIM_DT_ON_DEVICE, root_bone, axes,
                                  C.addressof(host) if dt is not None else dt_ptr, placements_ptr)
        api.check(api.lib().mmdx_animator_root_motion(self.h, motion_set.h, model.h if model is not None else None, C.byref(args)))

    def root_turn(self, motion_set: "MotionSet", root_bone: int, axes: int, placements_ptr, dt: Optional[float] = None, dt_ptr=None,
                  model=None, normalize: bool = False) -> None:
        """root_motion for clips whose root also rotates (mmdx_animator_root_motion_turn): the displacement is taken in the root's
        own frame at the start of the step, and each placement's heading [4..7] is multiplied by the root's rotation delta --
        normalised afterwards with normalize=True (api.ROOT_NORMALIZE).  placements[i][0..2] and [4..7] are written."""
        if (dt is None) == (dt_ptr is None):
            raise ValueError("give one of dt and dt_ptr")
        host = C.c_double(dt) if dt is not None else None
        flags = (0 if dt is not None else ANIM_DT_ON_DEVICE) | (api.ROOT_NORMALIZE if normalize else 0)
        args = api.RootTurnArgs(C.sizeof(api.RootTurnArgs), flags, root_bone, axes, C.addressof(host) if dt is not None else dt_ptr,
                                placements_ptr)
        api.check(api.lib().mmdx_animator_root_motion_turn(self.h, motion_set.h, model.h if model is not None else None, C.byref(args)))

    def step(self, motion_set: "MotionSet", root_bone: int, axes: int, placements_ptr, dt: Optional[float] = None, dt_ptr=None,
             model=None, turn: bool = False, normalize: bool = False) -> None:
        """root_motion -- root_turn with turn=True, where normalize applies -- then advance, with one step: the order the header
        requires, in one call."""
        if turn:
            self.root_turn(motion_set, root_bone, axes, placements_ptr, dt, dt_ptr, model, normalize)
        elif normalize:
            raise ValueError("normalize needs turn=True")
        else:
            self.root_motion(motion_set, root_bone, axes, placements_ptr, dt, dt_ptr, model)
        if dt is not None:
            self.advance(dt, model)
        else:
            self.advance_device_dt(dt_ptr, model)

    def events(self, event_set: "EventSet", out_fired_ptr, dt: Optional[float] = None, dt_ptr=None, lists=None, levels_ptr=None,
               dominant: bool = False, model=None) -> None:
        """mmdx_animator_events: out_fired u32[NI] (device memory) receives, per instance, the channels of the markers of `event_set`
        that the step advance() is ABOUT to take passes -- call it before advance with the same step, dt or dt_ptr as in
        root_motion.  lists: None, or (masks, list_stride, out_ids_ptr, out_counts_ptr) -- up to four channel masks; list l, at
        out_ids + l * list_stride words, receives in ascending order the instances whose mask meets masks[l] (and, with levels_ptr,
        mmdx_cull_bounds' out_levels, are not culled), out_counts u32[4] the lengths.  dominant: only the heavier side of a
        cross-fade fires (EVENTS_DOMINANT_SIDE).  The animator's arrays are not written."""
        if (dt is None) == (dt_ptr is None):
            raise ValueError("give one of dt and dt_ptr")
        host = C.c_double(dt) if dt is not None else None
        flags = (0 if dt is not None else ANIM_DT_ON_DEVICE) | (api.EVENTS_DOMINANT_SIDE if dominant else 0)
        args = EventsArgs(C.sizeof(EventsArgs), flags, C.addressof(host) if dt is not None else dt_ptr, out_fired_ptr)
        if lists is not None:
            masks, args.list_stride, args.out_ids, args.out_counts = lists
            if len(masks) > api.EVENTS_MAX_LISTS:
                raise ValueError("at most %d lists" % api.EVENTS_MAX_LISTS)
            args.n_lists = len(masks)
            for l, m in enumerate(masks):
                args.list_mask[l] = int(m)
        args.levels = levels_ptr
        api.check(api.lib().mmdx_animator_events(self.h, event_set.h, model.h if model is not None else None, C.byref(args)))

    def request(self, ids, clips, fades=None, start_times=None, model=None) -> None:
        """Host lists: instance ids[j] fades (fades[j] seconds, default 0 = at once) to clips[j] started at start_times[j]."""
        i, c = np.ascontiguousarray(ids, np.uint32).reshape(-1), np.ascontiguousarray(clips, np.uint32).reshape(-1)
        f = None if fades is None else np.ascontiguousarray(fades, np.float32).reshape(-1)
        t = None if start_times is None else np.ascontiguousarray(start_times, np.float64).reshape(-1)
        if any(x is not None and x.size != i.size for x in (c, f, t)):
            raise ValueError("one clip (and fade, start time) per listed instance")
        api.check(api.lib().mmdx_animator_request(self.h, model.h if model is not None else None, i.size, i.ctypes.data, c.ctypes.data,
                                                  f.ctypes.data if f is not None else None, t.ctypes.data if t is not None else None, 0))

    def request_device(self, n: int, ids_ptr, clips_ptr, fades_ptr=None, start_times_ptr=None, model=None) -> None:
        """The same with the lists in device memory (recordable); an id >= n_instances is skipped on the device."""
        api.check(api.lib().mmdx_animator_request(self.h, model.h if model is not None else None, n, ids_ptr, clips_ptr, fades_ptr,
                                                  start_times_ptr, TIMES_ON_DEVICE))

    def set_state(self, model=None, **arrays) -> None:
        """Overwrite the named arrays (clips_a=..., speed=..., ...: ANIMATOR_ARRAYS), [n_instances] each; the others keep their bytes."""
        s = AnimatorArrays(C.sizeof(AnimatorArrays), self.ni)
        keep = []
        types = dict(ANIMATOR_ARRAYS)
        for k, v in arrays.items():
            a = np.ascontiguousarray(v, types[k]).reshape(-1)
            if a.size != self.ni:
                raise ValueError(f"{k}: one value per instance")
            keep.append(a)
            setattr(s, k, a.ctypes.data)
        api.check(api.lib().mmdx_animator_set_state(self.h, model.h if model is not None else None, C.byref(s)))

    def get_state(self, model=None, names=None) -> Dict[str, np.ndarray]:
        """The named arrays (default: all eleven) as numpy arrays."""
        s = AnimatorArrays(C.sizeof(AnimatorArrays), self.ni)
        out = {k: np.zeros(self.ni, t) for k, t in ANIMATOR_ARRAYS if names is None or k in names}
        for k, a in out.items():
            setattr(s, k, a.ctypes.data)
        api.check(api.lib().mmdx_animator_get_state(self.h, model.h if model is not None else None, C.byref(s)))
        return out

    def operands(self) -> MotionBlendArgs:
        """mmdx_motion_blend_args over the animator's own device arrays, ready for the three blend calls."""
        a = MotionBlendArgs()
        api.check(api.lib().mmdx_animator_operands(self.h, C.byref(a)))
        return a

    def operand_ptrs(self) -> tuple:
        """The same five device addresses in the order the *_blend_time_device methods take them: clips a, times a, clips b,
        times b, weights."""
        a = self.operands()
        return a.clips_a, a.times_a, a.clips_b, a.times_b, a.weights

    def device_arrays(self) -> Dict[str, int]:
        """Device address of every state array (for an adopter's own kernels)."""
        s = AnimatorArrays(C.sizeof(AnimatorArrays), self.ni)
        api.check(api.lib().mmdx_animator_device_arrays(self.h, C.byref(s)))
        return {k: getattr(s, k) for k, _ in ANIMATOR_ARRAYS}

    def close(self):
        if getattr(self, "h", None):
            api.lib().mmdx_animator_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


EventMarker, EventSetDesc, EventsArgs = api.EventMarker, api.EventSetDesc, api.EventsArgs


class EventSet:
    """The markers of an animator's clips (mmdx_event_set_t): markers = (time seconds, clip, channel < 32) in any order; the set keeps
    them sorted by (clip, time) and copies what it needs of the animator, which may be closed afterwards."""

    def __init__(self, animator: "Animator", markers):
        rows = [(float(t), int(c), int(ch)) for t, c, ch in markers]
        table = (EventMarker * max(len(rows), 1))(*[EventMarker(*r) for r in rows])
        desc = EventSetDesc(C.sizeof(EventSetDesc), len(rows), C.addressof(table) if rows else None)
        self.h = C.c_void_p()
        api.check(api.lib().mmdx_event_set_create(animator.h, C.byref(desc), C.byref(self.h)))
        self.n_markers = len(rows)

    def info(self) -> dict:
        i = api.EventSetInfo(C.sizeof(api.EventSetInfo))
        api.check(api.lib().mmdx_event_set_get_info(self.h, C.byref(i)))
        return dict(n_markers=i.n_markers, n_clips=i.n_clips, device_ordinal=i.device_ordinal)

    def close(self):
        if getattr(self, "h", None):
            api.lib().mmdx_event_set_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class SkeletonDesc(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("n_bones", C.c_uint32), ("rest_position", C.c_void_p),
                ("parent", C.c_void_p), ("transform_level", C.c_void_p), ("flags", C.c_void_p),
                ("append_parent", C.c_void_p), ("append_ratio", C.c_void_p),
                ("ik_target", C.c_void_p), ("ik_loop_count", C.c_void_p), ("ik_angle_limit", C.c_void_p),
                ("ik_link_offset", C.c_void_p), ("ik_link_bone", C.c_void_p), ("ik_link_limited", C.c_void_p),
                ("ik_link_lo", C.c_void_p), ("ik_link_hi", C.c_void_p),
                ("n_morphs", C.c_uint32), ("create_flags", C.c_uint32), ("morph_type", C.c_void_p),
                ("morph_offset", C.c_void_p), ("morph_index", C.c_void_p), ("morph_value", C.c_void_p),
                ("morph_rotation", C.c_void_p)]


class SkeletonInfo(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("n_bones", C.c_uint32), ("n_pre_physics", C.c_uint32),
                ("n_post_physics", C.c_uint32), ("max_chain", C.c_uint32), ("solver", C.c_uint32),
                ("n_ik_bones", C.c_uint32), ("n_ik_links", C.c_uint32), ("n_append_bones", C.c_uint32),
                ("n_bone_morph_entries", C.c_uint32), ("n_solve_rounds", C.c_uint32),
                ("n_ik_rounds_16_lanes", C.c_uint32)]


SOLVER_PARALLEL_FK, SOLVER_SERIAL = 0, 1
SKELETON_PHYSICS_SEAM = 1
OVERRIDES_ON_DEVICE = 1 << 5


class PhysicsOverrides(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("n_bones", C.c_uint32), ("bone", C.c_void_p), ("strict", C.c_void_p),
                ("skinning", C.c_void_p)]


class Skeleton:
    """A model's bone hierarchy compiled for the device bone solve (local poses -> float[16] palettes,
    Poser::UpdateBoneTransform + UpdateBoneSkinningMatrix in the reference's evaluation order).
    ik = dict(target, loop, angle, link_off, link_bone, link_limited, link_lo, link_hi) as produced by
    synth.make_ik_rig / the PMX loader; None for a rig without IK."""

    def __init__(self, rest_position, parent, transform_level=None, flags=None, append_parent=None,
                 append_ratio=None, ik=None, morphs=None, physics_seam=False):
        """morphs = dict(type i32[NM], offset u32[NM+1], index u32[E], value f32[E,3], rotation f32[E,4] or None):
        the model's morph table; its group and bone morphs feed mmdx_skeleton_solve_morphed."""
        rest = np.ascontiguousarray(rest_position, np.float32).reshape(-1, 3)
        nb = rest.shape[0]

        def arr(a, dt, shape=None):
            if a is None:
                return None
            a = np.ascontiguousarray(a, dt)
            return a.reshape(shape) if shape is not None else a
        keep = [rest, arr(parent, np.int32, nb), arr(transform_level, np.int32, nb), arr(flags, np.uint16, nb),
                arr(append_parent, np.int32, nb), arr(append_ratio, np.float32, nb)]
        if ik is not None:
            keep += [arr(ik["target"], np.int32, nb), arr(ik["loop"], np.int32, nb), arr(ik["angle"], np.float32, nb),
                     arr(ik["link_off"], np.uint32, nb + 1), arr(ik["link_bone"], np.int32), arr(ik["link_limited"], np.uint8),
                     arr(ik["link_lo"], np.float32), arr(ik["link_hi"], np.float32)]
        else:
            keep += [None] * 8
        nm = 0
        if morphs is not None:
            nm = int(np.asarray(morphs["type"]).size)
            mk = [arr(morphs["type"], np.int32, nm), arr(morphs["offset"], np.uint32, nm + 1), arr(morphs["index"], np.uint32),
                  arr(morphs["value"], np.float32), arr(morphs.get("rotation"), np.float32)]
        else:
            mk = [None] * 5
        ptr = lambda a: a.ctypes.data if a is not None else None          # noqa: E731
        d = SkeletonDesc(C.sizeof(SkeletonDesc), nb, *[ptr(a) for a in keep], nm, SKELETON_PHYSICS_SEAM if physics_seam else 0,
                         *[ptr(a) for a in mk])
        self._keep = keep + mk
        self.rest_position = rest                # f32 [NB, 3]: what engine.SocketSet.from_skeleton builds its desc from
        self.parent = keep[1]                    # i32 [NB]: what engine.chains_below walks
        self.nm = nm
        self.h = C.c_void_p()
        api.check(api.lib().mmdx_skeleton_create(C.byref(d), C.byref(self.h)))
        info = SkeletonInfo()
        info.struct_size = C.sizeof(SkeletonInfo)
        api.check(api.lib().mmdx_skeleton_get_info(self.h, C.byref(info)))
        self.info = {k: getattr(info, k) for k, _ in SkeletonInfo._fields_}
        self.nb = nb

    def last_solve_shape(self) -> dict:
        """mmdx_debug_last_solve_shape: what the last solve of this skeleton launched -- solver ('none' | 'ordered' |
        'parallel_fk') and, of the ordered solver, nested / dense / select, workgroups, lds, segments (ordered-segment launches)
        and coop_launches (ik_coop launches).  Tests prove with it which compilation of the ordered kernel they ran."""
        s = api.DebugSolveShape()
        s.struct_size = C.sizeof(api.DebugSolveShape)
        api.check(api.lib().mmdx_debug_last_solve_shape(self.h, C.byref(s)))
        d = {k: int(getattr(s, k)) for k, _ in api.DebugSolveShape._fields_ if k not in ("struct_size", "reserved0")}
        d["solver"] = api.DEBUG_SOLVERS[d["solver"]]
        return d

    def subtree_mask(self, roots, inside: float = 1.0, outside: float = 0.0) -> np.ndarray:
        """A mask row for blend_poses from the hierarchy (mmdx_skeleton_subtree_mask, host only): f32 [NB] holding `inside` for
        every bone that is one of `roots` or has one among its ancestors, `outside` for the rest."""
        r = np.ascontiguousarray(roots, np.uint32).reshape(-1)
        out = np.empty(self.nb, np.float32)
        api.check(api.lib().mmdx_skeleton_subtree_mask(self.h, r.size, r.ctypes.data if r.size else None, inside, outside,
                                                       out.ctypes.data))
        return out

    def solve(self, poses, model=None, morph_weights=None) -> np.ndarray:
        """Host convenience: poses f32 [NI, NB, 8] (+ morph rates [NI, NM] or shared [NM]) -> palettes
        f32 [NI, NB, 16]."""
        p = np.ascontiguousarray(poses, np.float32).reshape(-1, self.nb, POSE_FLOATS)
        out = np.empty((p.shape[0], self.nb, 16), np.float32)
        if morph_weights is None:
            api.check(api.lib().mmdx_skeleton_solve(self.h, model.h if model is not None else None, p.shape[0],
                                                    p.ctypes.data, 0, out.ctypes.data))
        else:
            w = np.ascontiguousarray(morph_weights, np.float32)
            flags = api.WEIGHTS_SHARED if w.ndim == 1 else 0
            assert w.shape[-1] == self.nm and (w.ndim == 1 or w.shape[0] == p.shape[0])
            api.check(api.lib().mmdx_skeleton_solve_morphed(self.h, model.h if model is not None else None, p.shape[0],
                                                            p.ctypes.data, w.ctypes.data, flags, out.ctypes.data))
        return out

    # -- the physics seam: PrePhysicsPosing | the reactor's writes | PostPhysicsPosing (main.cpp:1801-1810) ------------
    def solve_pre(self, poses, model=None, morph_weights=None) -> np.ndarray:
        """Reset + bone morphs + the pre-physics bone list -> palettes [NI, NB, 16] (rows of post-physics bones are
        unspecified until solve_post)."""
        p = np.ascontiguousarray(poses, np.float32).reshape(-1, self.nb, POSE_FLOATS)
        self._seam_out = np.empty((p.shape[0], self.nb, 16), np.float32)
        w, flags = None, 0
        if morph_weights is not None:
            w = np.ascontiguousarray(morph_weights, np.float32)
            flags = api.WEIGHTS_SHARED if w.ndim == 1 else 0
        api.check(api.lib().mmdx_skeleton_solve_pre(self.h, model.h if model is not None else None, p.shape[0],
                                                    p.ctypes.data, w.ctypes.data if w is not None else None, flags,
                                                    self._seam_out.ctypes.data))
        return self._seam_out.copy()

    def solve_post(self, bones, strict, skinning, model=None) -> np.ndarray:
        """The reactor's writes (skinning [NI, K, 16] for bones [K]; Fix where strict [K]) then the post-physics list
        -> the complete palettes [NI, NB, 16]."""
        b = np.ascontiguousarray(bones, np.int32).reshape(-1)
        k = b.size
        st = np.ascontiguousarray(strict, np.uint8).reshape(k)
        xf = np.ascontiguousarray(skinning, np.float32)
        xf = xf.reshape(-1, k, 16) if k else xf.reshape(xf.shape[0], 0, 16)
        ni = xf.shape[0]
        if getattr(self, "_seam_out", None) is None or self._seam_out.shape[0] != ni:
            self._seam_out = np.empty((ni, self.nb, 16), np.float32)     # the library rejects the call
        ov = PhysicsOverrides(C.sizeof(PhysicsOverrides), k, b.ctypes.data if k else None, st.ctypes.data if k else None,
                              xf.ctypes.data if k else None)
        api.check(api.lib().mmdx_skeleton_solve_post(self.h, model.h if model is not None else None, ni, C.byref(ov), 0,
                                                     self._seam_out.ctypes.data))
        return self._seam_out.copy()

    # -- bone tracks -> palettes in one call (one launch on parallel-FK skeletons: the poses stay in LDS) -------------
    def solve_motion(self, motion: "BoneMotion", frames, model=None) -> np.ndarray:
        """Host convenience: frame numbers [NI] -> palettes f32 [NI, NB, 16] (= solve(motion.eval(frames)))."""
        f = np.ascontiguousarray(frames, np.uint32).reshape(-1)
        out = np.empty((f.size, self.nb, 16), np.float32)
        api.check(api.lib().mmdx_skeleton_solve_motion(self.h, motion.h, model.h if model is not None else None, f.size,
                                                       f.ctypes.data, 0, out.ctypes.data))
        return out

    def solve_motion_device(self, motion: "BoneMotion", n_instances: int, frames_ptr, out_ptr, model=None) -> None:
        """Frame numbers and palettes resident in HBM; asynchronous on the model's stream."""
        api.check(api.lib().mmdx_skeleton_solve_motion(self.h, motion.h, model.h if model is not None else None, n_instances,
                                                       frames_ptr, FRAMES_ON_DEVICE | api.OUT_ON_DEVICE, out_ptr))

    def solve_motion_time(self, motion: "BoneMotion", times, model=None) -> np.ndarray:
        """Host convenience: times in seconds f64 [NI] -> palettes f32 [NI, NB, 16] (= solve(motion.eval_time(times)))."""
        t = np.ascontiguousarray(times, np.float64).reshape(-1)
        out = np.empty((t.size, self.nb, 16), np.float32)
        api.check(api.lib().mmdx_skeleton_solve_motion_time(self.h, motion.h, model.h if model is not None else None, t.size,
                                                            t.ctypes.data, 0, out.ctypes.data))
        return out

    def solve_motion_time_device(self, motion: "BoneMotion", n_instances: int, times_ptr, out_ptr, model=None) -> None:
        """Times (f64 seconds) and palettes resident in HBM; asynchronous on the model's stream."""
        api.check(api.lib().mmdx_skeleton_solve_motion_time(self.h, motion.h, model.h if model is not None else None, n_instances,
                                                            times_ptr, TIMES_ON_DEVICE | api.OUT_ON_DEVICE, out_ptr))

    # -- the same from a motion set: every instance its own clip -----------------------------------------------------
    def _solve_set(self, fn, motion_set, clips, clock, dtype, model):
        c = np.ascontiguousarray(clips, np.uint32).reshape(-1)
        t = np.ascontiguousarray(clock, dtype).reshape(-1)
        if c.size != t.size:
            raise ValueError("one clip index per instance")
        out = np.empty((c.size, self.nb, 16), np.float32)
        api.check(fn(self.h, motion_set.h, model.h if model is not None else None, c.size, c.ctypes.data, t.ctypes.data, 0,
                     out.ctypes.data))
        return out

    def solve_motion_set(self, motion_set: "MotionSet", clips, frames, model=None) -> np.ndarray:
        """Host convenience: clip ids [NI], frame numbers [NI] -> palettes f32 [NI, NB, 16]."""
        return self._solve_set(api.lib().mmdx_skeleton_solve_motion_set, motion_set, clips, frames, np.uint32, model)

    def solve_motion_set_time(self, motion_set: "MotionSet", clips, times, model=None) -> np.ndarray:
        """Host convenience: clip ids [NI], times in seconds f64 [NI] -> palettes f32 [NI, NB, 16]."""
        return self._solve_set(api.lib().mmdx_skeleton_solve_motion_set_time, motion_set, clips, times, np.float64, model)

    def solve_motion_set_device(self, motion_set: "MotionSet", n_instances: int, clips_ptr, frames_ptr, out_ptr, model=None) -> None:
        """Clip ids, frame numbers and palettes resident in HBM; asynchronous on the model's stream."""
        api.check(api.lib().mmdx_skeleton_solve_motion_set(self.h, motion_set.h, model.h if model is not None else None, n_instances,
                                                           clips_ptr, frames_ptr, FRAMES_ON_DEVICE | api.OUT_ON_DEVICE, out_ptr))

    def solve_motion_set_time_device(self, motion_set: "MotionSet", n_instances: int, clips_ptr, times_ptr, out_ptr,
                                     model=None) -> None:
        """Clip ids, times (f64 seconds) and palettes resident in HBM; asynchronous on the model's stream."""
        api.check(api.lib().mmdx_skeleton_solve_motion_set_time(self.h, motion_set.h, model.h if model is not None else None,
                                                                n_instances, clips_ptr, times_ptr,
                                                                TIMES_ON_DEVICE | api.OUT_ON_DEVICE, out_ptr))

    def solve_motion_set_blend_time(self, motion_set: "MotionSet", clips_a, times_a, clips_b, times_b, weights, model=None) -> np.ndarray:
        """Host convenience: the cross-fade of MotionSet.blend_bones_time solved -> palettes f32 [NI, NB, 16]."""
        args, keep = blend_args_host(clips_a, times_a, clips_b, times_b, weights)
        out = np.empty((args.n_instances, self.nb, 16), np.float32)
        api.check(api.lib().mmdx_skeleton_solve_motion_set_blend_time(self.h, motion_set.h, model.h if model is not None else None,
                                                                      C.byref(args), out.ctypes.data))
        return out

    def solve_motion_set_blend_time_device(self, motion_set: "MotionSet", n_instances: int, clips_a_ptr, times_a_ptr, clips_b_ptr,
                                           times_b_ptr, weights_ptr, out_ptr, model=None) -> None:
        """All five operand arrays and the palettes resident in HBM; asynchronous on the model's stream."""
        args = blend_args_device(n_instances, clips_a_ptr, times_a_ptr, clips_b_ptr, times_b_ptr, weights_ptr)
        api.check(api.lib().mmdx_skeleton_solve_motion_set_blend_time(self.h, motion_set.h, model.h if model is not None else None,
                                                                      C.byref(args), out_ptr))

    def solve_device(self, n_instances: int, poses_ptr, out_ptr, model=None, weights_ptr=None, shared=False) -> None:
        """poses, palettes (and morph rates) resident in HBM; asynchronous on the model's stream."""
        flags = POSES_ON_DEVICE | api.OUT_ON_DEVICE | (api.WEIGHTS_ON_DEVICE if weights_ptr else 0) | \
            (api.WEIGHTS_SHARED if shared else 0)
        api.check(api.lib().mmdx_skeleton_solve_morphed(self.h, model.h if model is not None else None, n_instances,
                                                        poses_ptr, weights_ptr, flags, out_ptr))

    # -- the solve for a listed subset of the crowd (mmdx_skeleton_solve_select) --------------------------------------
    def solve_select_device(self, n_instances: int, poses_ptr, out_ptr, ids_ptr, n_ids: int, count_ptr=None, model=None,
                            weights_ptr=None, shared=False, select_on_device=True) -> None:
        """poses, palettes (and morph rates) resident in HBM, [n_instances] rows each; only the instances in the u32 list at
        ids_ptr (capacity n_ids, the first *count_ptr in use; count_ptr None = all n_ids) are solved, every other palette row
        keeps its bytes.  List and count in device memory (asynchronous on the model's stream) or, with select_on_device=False,
        in host memory (the call returns when its work is done)."""
        flags = POSES_ON_DEVICE | api.OUT_ON_DEVICE | (api.WEIGHTS_ON_DEVICE if weights_ptr else 0) | \
            (api.WEIGHTS_SHARED if shared else 0)
        s = api.InstanceSelect()
        s.struct_size = C.sizeof(api.InstanceSelect)
        s.flags = api.SELECT_ON_DEVICE if select_on_device else 0
        s.ids, s.count, s.n_ids = ids_ptr, count_ptr, n_ids
        api.check(api.lib().mmdx_skeleton_solve_select(self.h, model.h if model is not None else None, n_instances, poses_ptr,
                                                       weights_ptr, flags, C.byref(s), out_ptr))

    def solve_select(self, poses, ids, count=None, model=None, morph_weights=None, out=None) -> np.ndarray:
        """Host convenience: uploads poses [NI, NB, 8] (+ rates [NI, NM] or shared [NM]), the id list and `out` (the palettes
        [NI, NB, 16] as they stand before the call; zeros when None), solves the first `count` (None = all) listed instances
        and downloads the WHOLE palette array, so the rows the call must not touch can be looked at."""
        from .engine import DeviceBuffer
        p = np.ascontiguousarray(poses, np.float32).reshape(-1, self.nb, POSE_FLOATS)
        ni = p.shape[0]
        ids = np.ascontiguousarray(ids, np.uint32).reshape(-1)
        before = np.zeros((ni, self.nb, 16), np.float32) if out is None else np.ascontiguousarray(out, np.float32)
        assert before.shape == (ni, self.nb, 16)
        bufs = [DeviceBuffer.from_numpy(p), DeviceBuffer.from_numpy(before), DeviceBuffer(max(ids.nbytes, 4))]
        d_pose, d_out, d_ids = bufs
        if ids.size:
            d_ids.upload(ids)
        d_cnt = d_w = None
        if count is not None:
            d_cnt = DeviceBuffer.from_numpy(np.array([count], np.uint32))
            bufs.append(d_cnt)
        shared = False
        if morph_weights is not None:
            w = np.ascontiguousarray(morph_weights, np.float32)
            shared = w.ndim == 1
            assert w.shape[-1] == self.nm and (shared or w.shape[0] == ni)
            d_w = DeviceBuffer.from_numpy(w)
            bufs.append(d_w)
        try:
            self.solve_select_device(ni, d_pose.ptr, d_out.ptr, d_ids.ptr, ids.size, d_cnt.ptr if d_cnt else None, model,
                                     d_w.ptr if d_w else None, shared)
            api.check(api.lib().mmdx_sync(model.h) if model is not None else api.lib().mmdx_device_synchronize())
            return d_out.download((ni, self.nb, 16), np.float32)
        finally:
            for b in bufs:
                b.free()

    # -- tracks and solve for a listed subset of the crowd (mmdx_skeleton_solve_motion_set_blend_time_select) ----------------
    def solve_motion_set_blend_time_select_device(self, motion_set: "MotionSet", n_instances: int, clips_a_ptr, times_a_ptr,
                                                  clips_b_ptr, times_b_ptr, weights_ptr, out_ptr, ids_ptr, n_ids: int, count_ptr=None,
                                                  model=None, select_on_device=True) -> None:
        """solve_motion_set_blend_time_device for the instances in the u32 list at ids_ptr only (capacity n_ids, the first
        *count_ptr in use; count_ptr None = all n_ids); every palette row that is not listed keeps its bytes.  List and count in
        device memory (asynchronous) or, with select_on_device=False, in host memory (the call returns when its work is done)."""
        args = blend_args_device(n_instances, clips_a_ptr, times_a_ptr, clips_b_ptr, times_b_ptr, weights_ptr)
        s = instance_select(ids_ptr, n_ids, count_ptr, select_on_device)
        api.check(api.lib().mmdx_skeleton_solve_motion_set_blend_time_select(self.h, motion_set.h, model.h if model is not None else None,
                                                                             C.byref(args), C.byref(s), out_ptr))

    def solve_motion_set_blend_time_select(self, motion_set: "MotionSet", clips_a, times_a, clips_b, times_b, weights, ids, count=None,
                                           model=None, out=None) -> np.ndarray:
        """Host convenience in the style of solve_select: uploads the five operand arrays [NI], the id list and `out` (the palettes
        [NI, NB, 16] as they stand before the call; zeros when None), evaluates and solves the first `count` (None = all) listed
        instances and downloads the WHOLE palette array."""
        from .engine import DeviceBuffer
        args, keep = blend_args_host(clips_a, times_a, clips_b, times_b, weights)
        ca, cb, ta, tb, w = keep
        ni = args.n_instances
        ids = np.ascontiguousarray(ids, np.uint32).reshape(-1)
        before = np.zeros((ni, self.nb, 16), np.float32) if out is None else np.ascontiguousarray(out, np.float32)
        assert before.shape == (ni, self.nb, 16)
        bufs = [DeviceBuffer.from_numpy(a) for a in (ca, ta, cb, tb, w)] + [DeviceBuffer.from_numpy(before), DeviceBuffer(max(ids.nbytes, 4))]
        d_out, d_ids = bufs[5], bufs[6]
        if ids.size:
            d_ids.upload(ids)
        d_cnt = None
        if count is not None:
            d_cnt = DeviceBuffer.from_numpy(np.array([count], np.uint32))
            bufs.append(d_cnt)
        try:
            self.solve_motion_set_blend_time_select_device(motion_set, ni, *[b.ptr for b in bufs[:5]], d_out.ptr, d_ids.ptr, ids.size,
                                                           d_cnt.ptr if d_cnt else None, model)
            api.check(api.lib().mmdx_sync(model.h) if model is not None else api.lib().mmdx_device_synchronize())
            return d_out.download((ni, self.nb, 16), np.float32)
        finally:
            for b in bufs:
                b.free()

    def close(self):
        if getattr(self, "h", None):
            api.lib().mmdx_skeleton_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

"""Host-side Python front-end of the C ABI (include/mmdx.h): model handles, device buffers and the
deform calls.  Thin by design -- every number is produced by libmmdx.so on the GPU.

`Poser` mirrors the slice of the reference's `mmd::Poser` that sits on the hot path
(L/motion/poser.inl:17-43): SetMorphPose / ResetPosing / Deform / pose_image, plus the palette
injection the reference performs through PhysicsReactor::GetPoserBoneImage
(L/motion/physics.inl:32-40) and the viewer's UpdateDeformedVertices (main.cpp:821-863).
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Tuple

import numpy as np

from . import _capi as api
from .synth import FlatModel

_f32p = C.POINTER(C.c_float)
_i32p = C.POINTER(C.c_int32)
_u32p = C.POINTER(C.c_uint32)


def _c(a, dt):
    return np.ascontiguousarray(a, dtype=dt)


def _ptr(a, t):
    return a.ctypes.data_as(t) if a is not None and a.size else None


def device_count() -> int:
    n = C.c_int32(0)
    st = api.lib().mmdx_device_count(C.byref(n))
    return int(n.value) if st == api.OK else 0


def device_select(ordinal: int) -> None:
    api.check(api.lib().mmdx_device_select(ordinal))


def device_name(ordinal: int = 0) -> str:
    buf = C.create_string_buffer(256)
    api.check(api.lib().mmdx_device_name(ordinal, buf, 256))
    return buf.value.decode()


def device_synchronize() -> None:
    api.check(api.lib().mmdx_device_synchronize())


def planes_from_matrix(m, depth_zero_to_one: bool = False) -> np.ndarray:
    """mmdx_cull_planes_from_matrix: the six frustum planes (left, right, bottom, top, near, far; f32 [6,4], not normalised) of a
    column-major clip-space transform m (16 floats, element (r, c) at m[c*4+r], as HandmadeMath and OpenGL store it)."""
    m = _c(m, np.float32).reshape(16)
    out = np.empty((6, 4), np.float32)
    api.check(api.lib().mmdx_cull_planes_from_matrix(_ptr(m, _f32p), 1 if depth_zero_to_one else 0, _ptr(out, _f32p)))
    return out


def make_cull_view(planes=(), eye=(0.0, 0.0, 0.0), lod_distance=(), margin: float = 0.0, n_planes=None, n_lods=None) -> api.CullView:
    """An mmdx_cull_view from arrays: planes [n,4] (a,b,c,d), the eye, up to 3 ascending LOD distances (n_lods = their number + 1).
    n_planes / n_lods override the counts as written into the structure (device views are not validated)."""
    v = api.CullView()
    pl = _c(planes, np.float32).reshape(-1, 4)
    assert pl.shape[0] <= api.CULL_MAX_PLANES and len(lod_distance) <= api.CULL_MAX_LODS - 1
    for p in range(pl.shape[0]):
        for k in range(4):
            v.planes[p][k] = pl[p, k]
    v.n_planes = pl.shape[0] if n_planes is None else n_planes
    v.n_lods = len(lod_distance) + 1 if n_lods is None else n_lods
    for k in range(3):
        v.eye[k] = eye[k]
    v.margin = margin
    for k, d in enumerate(lod_distance):
        v.lod_distance[k] = d
    return v


class DeviceBuffer:
    """A hipMalloc'ed range owned through the C ABI's memory helpers."""

    def __init__(self, nbytes: int):
        self.nbytes = int(nbytes)
        p = C.c_void_p()
        api.check(api.lib().mmdx_device_malloc(C.byref(p), self.nbytes))
        self.ptr = p.value

    @classmethod
    def adopt(cls, ptr: int, nbytes: int) -> "DeviceBuffer":
        """Wrap a device range allocated by the library (freed with mmdx_device_free like any other)."""
        b = cls.__new__(cls)
        b.nbytes, b.ptr = int(nbytes), int(ptr)
        return b

    @classmethod
    def from_numpy(cls, a: np.ndarray) -> "DeviceBuffer":
        a = np.ascontiguousarray(a)
        b = cls(a.nbytes)
        b.upload(a)
        return b

    def upload(self, a: np.ndarray, offset: int = 0) -> None:
        a = np.ascontiguousarray(a)
        assert offset + a.nbytes <= self.nbytes
        api.check(api.lib().mmdx_memcpy_h2d(self.ptr + offset, a.ctypes.data, a.nbytes))

    def download(self, shape, dtype, offset: int = 0) -> np.ndarray:
        out = np.empty(shape, dtype)
        assert offset + out.nbytes <= self.nbytes
        api.check(api.lib().mmdx_memcpy_d2h(out.ctypes.data, self.ptr + offset, out.nbytes))
        return out

    def memset(self, value: int = 0) -> None:
        api.check(api.lib().mmdx_device_memset(self.ptr, value, self.nbytes))

    def free(self) -> None:
        if self.ptr:
            api.lib().mmdx_device_free(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class PinnedArray:
    """A numpy view of page-locked host memory (mmdx_host_malloc): frame buffers that cross PCIe by DMA."""

    def __init__(self, shape, dtype):
        self.shape, self.dtype = tuple(shape), np.dtype(dtype)
        nbytes = int(np.prod(self.shape)) * self.dtype.itemsize
        p = C.c_void_p()
        api.check(api.lib().mmdx_host_malloc(C.byref(p), nbytes))
        self.ptr = p.value
        buf = (C.c_char * max(nbytes, 1)).from_address(self.ptr)
        self.array = np.frombuffer(buf, dtype=self.dtype, count=int(np.prod(self.shape))).reshape(self.shape)

    def free(self) -> None:
        if self.ptr:
            self.array = None
            api.lib().mmdx_host_free(self.ptr)
            self.ptr = None


class Graph:
    """mmdx_graph_t: a recorded sequence of library calls on one model's stream, replayed with one submission."""

    def __init__(self, handle):
        self.h = handle

    def launch(self) -> None:
        api.check(api.lib().mmdx_graph_launch(self.h))

    def close(self) -> None:
        if self.h:
            api.lib().mmdx_graph_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DeformModel:
    """mmdx_model_t: the model compiled to the kernels' HBM layout, resident on one GPU."""

    def __init__(self, flat: FlatModel, normalize: bool = True, f16_positions: bool = False,
                 host_only: bool = False, fast_math: bool = False, tile_order: bool = False):
        """fast_math: MMDX_CREATE_FAST_MATH -- contracted multiply-adds, results within the stated tolerance of the
        reference's instead of bit-identical (include/mmdx.h).  tile_order: MMDX_CREATE_TILE_ORDER -- outputs in the
        engine's vertex order (vertex_order() gives the permutation), same values."""
        self.flat = flat
        self.f16 = bool(f16_positions)
        self._keep = dict(
            positions=_c(flat.positions, np.float32), normals=_c(flat.normals, np.float32),
            uvs=_c(flat.uvs, np.float32), skin_type=_c(flat.skin_type, np.int32),
            bone_ids=_c(flat.bone_ids, np.int32), bone_weights=_c(flat.bone_weights, np.float32),
            sdef=_c(flat.sdef, np.float32) if flat.sdef is not None else None,
            bone_parent=_c(flat.bone_parent, np.int32), morph_type=_c(flat.morph_type, np.int32),
            morph_offset=_c(flat.morph_off, np.uint32), morph_index=_c(flat.morph_index, np.uint32),
            morph_value=_c(flat.morph_value, np.float32))
        k = self._keep
        d = api.ModelDesc()
        d.struct_size = C.sizeof(api.ModelDesc)
        d.flags = ((api.CREATE_NORMALIZE if normalize else 0) |
                   (api.CREATE_F16_POSITIONS if f16_positions else 0) |
                   (api.CREATE_HOST_ONLY if host_only else 0) |
                   (api.CREATE_FAST_MATH if fast_math else 0) |
                   (api.CREATE_TILE_ORDER if tile_order else 0))
        d.n_vertices, d.n_bones, d.n_morphs = flat.nv, flat.nb, flat.nm
        d.positions = _ptr(k["positions"], _f32p)
        d.normals = _ptr(k["normals"], _f32p)
        d.uvs = _ptr(k["uvs"], _f32p)
        d.skin_type = _ptr(k["skin_type"], _i32p)
        d.bone_ids = _ptr(k["bone_ids"], _i32p)
        d.bone_weights = _ptr(k["bone_weights"], _f32p)
        d.sdef_params = _ptr(k["sdef"], _f32p) if k["sdef"] is not None else None
        d.bone_parent = _ptr(k["bone_parent"], _i32p)
        d.morph_type = _ptr(k["morph_type"], _i32p)
        d.morph_offset = _ptr(k["morph_offset"], _u32p)
        d.morph_index = _ptr(k["morph_index"], _u32p)
        d.morph_value = _ptr(k["morph_value"], _f32p)
        h = C.c_void_p()
        api.check(api.lib().mmdx_model_create(C.byref(d), C.byref(h)))
        self.h = h
        self._keep = None  # borrowed only for the duration of the call
        self.info = self._get_info()
        self.nv, self.nb, self.nm, self.ns = (self.info.n_vertices, self.info.n_bones,
                                              self.info.n_morphs, self.info.n_slots)

    # -- lifetime -----------------------------------------------------------------------------
    def close(self) -> None:
        if getattr(self, "h", None):
            api.lib().mmdx_model_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # -- queries ------------------------------------------------------------------------------
    def _get_info(self) -> api.ModelInfo:
        info = api.ModelInfo()
        info.struct_size = C.sizeof(api.ModelInfo)
        api.check(api.lib().mmdx_model_get_info(self.h, C.byref(info)))
        return info

    def get_skin(self) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        t = np.empty(self.nv, np.int32)
        ids = np.empty((self.nv, 4), np.int32)
        w = np.empty((self.nv, 4), np.float32)
        api.check(api.lib().mmdx_model_get_skin(self.h, _ptr(t, _i32p), _ptr(ids, _i32p), _ptr(w, _f32p)))
        return t, ids, w

    def vertex_order(self) -> Tuple[np.ndarray, np.ndarray]:
        """(engine_to_original, original_to_engine): position e of a tile-order model's outputs holds file vertex
        engine_to_original[e]."""
        e2o, o2e = np.empty(self.nv, np.uint32), np.empty(self.nv, np.uint32)
        u32p = C.POINTER(C.c_uint32)
        api.check(api.lib().mmdx_model_get_vertex_order(self.h, _ptr(e2o, u32p), _ptr(o2e, u32p)))
        return e2o, o2e

    def slot_weights(self, rates) -> np.ndarray:
        rates = _c(rates, np.float32)
        assert rates.shape == (self.nm,)
        out = np.zeros(max(self.ns, 1), np.float32)
        api.check(api.lib().mmdx_model_slot_weights(self.h, _ptr(rates, _f32p), _ptr(out, _f32p)))
        return out[:self.ns]

    # -- the hot path -------------------------------------------------------------------------
    def deform(self, rates, palette) -> Tuple[np.ndarray, np.ndarray]:
        """mmdx_deform: one instance, host in / host out -> pose_image (pos, nrm) f32 [NV,3]."""
        rates = _c(rates, np.float32).reshape(-1)
        pal = _c(palette, np.float32).reshape(-1)
        assert rates.size == self.nm and pal.size == self.nb * 16
        pos = np.empty((self.nv, 3), np.float32)
        nrm = np.empty((self.nv, 3), np.float32)
        api.check(api.lib().mmdx_deform(self.h, _ptr(rates, _f32p), _ptr(pal, _f32p),
                                        _ptr(pos, _f32p), _ptr(nrm, _f32p)))
        return pos, nrm

    def deform_vertex32(self, rates, palette, pos_scale: float = 0.1) -> np.ndarray:
        rates = _c(rates, np.float32).reshape(-1)
        pal = _c(palette, np.float32).reshape(-1)
        assert rates.size == self.nm and pal.size == self.nb * 16
        out = np.empty((self.nv, 8), np.float32)
        api.check(api.lib().mmdx_deform_vertex32(self.h, _ptr(rates, _f32p), _ptr(pal, _f32p),
                                                 C.c_float(pos_scale), out.ctypes.data))
        return out

    def output_pitch(self, layout: int) -> int:
        """mmdx_model_output_pitch: the smallest instance pitch >= NV (in vertices) that starts every instance of `layout` on a
        16-byte boundary -- what alloc_outputs(..., pitch=) and deform_batched*(..., pitch=) take."""
        p = C.c_uint32(0)
        api.check(api.lib().mmdx_model_output_pitch(self.h, layout, C.byref(p)))
        return p.value

    def out_sizes(self, layout: int, ni: int, pitch: int = 0) -> Tuple[int, int]:
        """Bytes of the two output arrays of `ni` instances, [ni][pitch] vertices when a pitch is given, else [ni][NV]."""
        nvi = ni * (pitch or self.nv)
        if layout == api.OUT_SOA:
            return nvi * 12, nvi * 12
        if layout == api.OUT_VERTEX32:
            return nvi * 32, 0
        return nvi * 6, nvi * 12

    def alloc_outputs(self, layout: int, ni: int, max_tries: int = 16, pitch: int = 0):
        """The crowd's output arrays through mmdx_crowd_output_alloc (placement-aware on MI355X); with a pitch through
        mmdx_crowd_output_alloc_pitched ([ni][pitch] vertices, for calls with the same pitch).
        Returns (a, b or None, info dict); info["store_flags"] is the MMDX_OUT_STORES_* hint to OR into the flags of the crowd
        calls that write these arrays (the library itself remembers nothing about them)."""
        class _Info(C.Structure):
            _fields_ = [("struct_size", C.c_uint32), ("tries", C.c_uint32), ("probed", C.c_uint32),
                        ("store_GBs", C.c_float), ("fill_GBs", C.c_float), ("store_flags", C.c_uint32)]
        info = _Info()
        info.struct_size = C.sizeof(_Info)
        pa, pb = C.c_void_p(), C.c_void_p()
        if pitch:
            api.check(api.lib().mmdx_crowd_output_alloc_pitched(self.h, ni, layout, pitch, max_tries, C.byref(pa), C.byref(pb),
                                                                C.byref(info)))
        else:
            api.check(api.lib().mmdx_crowd_output_alloc(self.h, ni, layout, max_tries, C.byref(pa), C.byref(pb),
                                                        C.byref(info)))
        sa, sb = self.out_sizes(layout, ni, pitch)
        a = DeviceBuffer.adopt(pa.value, sa)
        b = DeviceBuffer.adopt(pb.value, sb) if pb.value else None
        return a, b, {"tries": info.tries, "probed": bool(info.probed), "store_GBs": info.store_GBs,
                      "fill_GBs": info.fill_GBs, "store_flags": int(info.store_flags)}

    def deform_batched_raw(self, ni: int, weights_ptr, palettes_ptr, out_a_ptr, out_b_ptr, layout: int,
                           flags: int, pos_scale: float = 1.0, pitch: int = 0, bounds_ptr=None, select_ptr=None,
                           select_count_ptr=None, n_select=None, select_on_device: bool = True) -> None:
        """pitch: instance pitch of the outputs in vertices (MMDX_OUT_PITCHED); 0 = dense [ni][NV].
        bounds_ptr: f32 [ni][6] {min xyz, max xyz} of every instance's written positions (mmdx_deform_batched_bounds), where the
        outputs live: a device pointer with OUT_ON_DEVICE, else a host pointer.
        n_select (not None): mmdx_deform_batched_select -- only the instances listed in the u32 array at select_ptr (capacity
        n_select; the first *select_count_ptr of them when a count is given) are deformed, everything else keeps its bytes;
        device operands only.  select_on_device: the list and the count are device pointers (else host pointers)."""
        a = api.DeformArgs()
        a.struct_size = C.sizeof(api.DeformArgs)
        if pitch:
            flags |= api.OUT_PITCHED
            a.out_instance_pitch = pitch
        a.flags, a.n_instances, a.out_layout = flags, ni, layout
        a.morph_weights, a.palettes = weights_ptr, palettes_ptr
        a.out_a, a.out_b = out_a_ptr, out_b_ptr
        a.pos_scale = pos_scale
        if n_select is not None:
            s = api.InstanceSelect()
            s.struct_size = C.sizeof(api.InstanceSelect)
            s.flags = api.SELECT_ON_DEVICE if select_on_device else 0
            s.ids, s.count, s.n_ids = select_ptr, select_count_ptr, n_select
            api.check(api.lib().mmdx_deform_batched_select(self.h, C.byref(a), C.byref(s), bounds_ptr))
        elif bounds_ptr is None:
            api.check(api.lib().mmdx_deform_batched(self.h, C.byref(a)))
        else:
            api.check(api.lib().mmdx_deform_batched_bounds(self.h, C.byref(a), bounds_ptr))

    def deform_batched(self, weights, palettes, layout: int = api.OUT_SOA, shared_weights: bool = False,
                       pos_scale: float = 1.0, pitch: int = 0, bounds: bool = False):
        """Host arrays in, host arrays out (copies + sync inside the call).
        weights [NI,NM] (or [NM] with shared_weights); palettes [NI,NB,16].  pitch: the call writes [NI][pitch]-vertex host
        arrays (MMDX_OUT_PITCHED); the [:, :NV] views of them are returned.  bounds: one more result, f32 [NI,6] = {min x,
        min y, min z, max x, max y, max z} of each instance's positions as written (mmdx_deform_batched_bounds)."""
        pal = _c(palettes, np.float32).reshape(-1, self.nb, 16)
        ni = pal.shape[0]
        w = _c(weights, np.float32)
        if self.nm:
            w = w.reshape(self.nm) if shared_weights else w.reshape(ni, self.nm)
        flags = api.WEIGHTS_SHARED if shared_weights else 0
        rows = pitch or self.nv
        if layout == api.OUT_SOA:
            oa = np.empty((ni, rows, 3), np.float32)
            ob = np.empty((ni, rows, 3), np.float32)
        elif layout == api.OUT_VERTEX32:
            oa = np.empty((ni, rows, 8), np.float32)
            ob = None
        else:
            oa = np.empty((ni, rows, 3), np.float16)
            ob = np.empty((ni, rows, 3), np.float32)
        bnd = np.empty((ni, 6), np.float32) if bounds else None
        self.deform_batched_raw(ni, w.ctypes.data if w.size else None, pal.ctypes.data, oa.ctypes.data,
                                ob.ctypes.data if ob is not None else None, layout, flags, pos_scale, pitch,
                                bnd.ctypes.data if bounds else None)
        if pitch:
            oa = oa[:, :self.nv]
            ob = ob[:, :self.nv] if ob is not None else None
        out = (oa, ob) if ob is not None else (oa,)
        return out + (bnd,) if bounds else (out if ob is not None else oa)

    def deform_batched_select(self, ni: int, ids, weights_ptr, palettes_ptr, out_a_ptr, out_b_ptr, layout: int, flags: int,
                              pos_scale: float = 1.0, pitch: int = 0, bounds_ptr=None, count=None) -> None:
        """mmdx_deform_batched_select with the list in host memory: `ids` (any integer sequence, converted to u32) names the
        instances of the `ni`-instance device arrays to deform, `count` (optional) how many leading ids are in use.  Every other
        operand is a device pointer as in deform_batched_raw; returns when the work has completed."""
        ids = np.ascontiguousarray(ids, dtype=np.uint32).reshape(-1)
        cnt = C.c_uint32(count) if count is not None else None
        self.deform_batched_raw(ni, weights_ptr, palettes_ptr, out_a_ptr, out_b_ptr, layout, flags, pos_scale, pitch, bounds_ptr,
                                select_ptr=ids.ctypes.data if ids.size else None,
                                select_count_ptr=C.addressof(cnt) if cnt is not None else None, n_select=int(ids.size),
                                select_on_device=False)

    def cull_bounds(self, bounds_buf, view, ni: int, ids_buf, counts_buf, levels_buf=None, list_stride=None) -> None:
        """mmdx_cull_bounds: the boxes in bounds_buf (device f32 [ni][6], as mmdx_deform_batched_bounds writes them) against the
        planes and LOD distances of `view` -- an api.CullView (host memory, validated, passed by value) or a DeviceBuffer holding
        one (read when the kernel runs: a recorded call reads it afresh at every replay).  List l (visible instances of level l in
        ascending order) goes to ids_buf at u32 offset l * list_stride (default ni), its length to counts_buf[l] (u32 [4]); these
        are what deform_batched_raw takes as select_ptr / select_count_ptr.  levels_buf (optional, u32 [ni]): every instance's
        level or api.CULLED.  Buffers are DeviceBuffers (or raw device addresses).  Asynchronous on the model's stream."""
        dev = lambda b: getattr(b, "ptr", b)
        a = api.CullArgs()
        a.struct_size = C.sizeof(api.CullArgs)
        a.n_instances = ni
        a.list_stride = ni if list_stride is None else list_stride
        a.bounds, a.out_ids, a.out_counts, a.out_levels = dev(bounds_buf), dev(ids_buf), dev(counts_buf), dev(levels_buf)
        if isinstance(view, api.CullView):
            a.flags, a.view = 0, C.addressof(view)
        else:
            a.flags, a.view = api.CULL_VIEW_ON_DEVICE, dev(view)
        api.check(api.lib().mmdx_cull_bounds(self.h, C.byref(a)))

    def place_palettes(self, n_instances: int, palettes_ptr, placements_ptr, out_ptr, flags: int) -> None:
        """mmdx_palette_place, the raw form: out[i][b] = palettes[i][b] * W[i] for the n_instances x NB skinning matrices at
        palettes_ptr, W[i] from the 8-float pose {tx, ty, tz, 0, qx, qy, qz, qw} (or, with api.PLACE_MATRIX, the 16-float matrix)
        at placements_ptr + i.  flags: api.PALETTE_ON_DEVICE | api.PLACE_ON_DEVICE | api.OUT_ON_DEVICE say which of the three
        addresses are device memory (the others are host memory, copied inside the call) | api.PLACE_MATRIX.  out_ptr may equal
        palettes_ptr.  With all three on the device the call is asynchronous on the model's stream and records into a graph."""
        a = api.PlaceArgs()
        a.struct_size = C.sizeof(api.PlaceArgs)
        a.flags, a.n_instances = flags, n_instances
        a.palettes, a.placements, a.out_palettes = palettes_ptr, placements_ptr, out_ptr
        api.check(api.lib().mmdx_palette_place(self.h, C.byref(a)))

    def place(self, palettes, placements) -> np.ndarray:
        """Host arrays in, host array out (copies + sync inside the call): palettes [NI,NB,16] and placements [NI,8] (poses) or
        [NI,16] / [NI,4,4] (matrices, translation in elements 12..14) -> the placed palettes [NI,NB,16]."""
        pal = _c(palettes, np.float32).reshape(-1, self.nb, 16)
        ni = pal.shape[0]
        pl = _c(placements, np.float32).reshape(ni, -1)
        if pl.shape[1] not in (api.POSE_FLOATS, 16):
            raise ValueError("placements must be [NI,8] poses or [NI,16] matrices")
        out = np.empty_like(pal)
        self.place_palettes(ni, pal.ctypes.data, pl.ctypes.data, out.ctypes.data, api.PLACE_MATRIX if pl.shape[1] == 16 else 0)
        return out

    def bone_boxes(self) -> dict:
        """mmdx_model_get_bone_boxes: the table mmdx_palette_bounds transforms -- bones u32 [n], boxes f32 [n,9] (lo xyz, hi xyz of
        the base positions of the vertices the bone moves, reach xyz of their morph offsets), and the scalars eps, weight_sum_dev,
        max_vertex_entries, n_nonconvex.  Works on host-only models."""
        info = api.BoneBoxInfo()
        info.struct_size = C.sizeof(api.BoneBoxInfo)
        api.check(api.lib().mmdx_model_get_bone_boxes(self.h, C.byref(info), None, None))
        bones, boxes = np.empty(info.n_boxes, np.uint32), np.empty((info.n_boxes, 9), np.float32)
        api.check(api.lib().mmdx_model_get_bone_boxes(self.h, C.byref(info), _ptr(bones, _u32p), _ptr(boxes, _f32p)))
        return dict(bones=bones, boxes=boxes, n_boxes=int(info.n_boxes), n_nonconvex=int(info.n_nonconvex),
                    max_vertex_entries=int(info.max_vertex_entries), eps=np.float32(info.eps),
                    weight_sum_dev=np.float32(info.weight_sum_dev))

    def palette_bounds_raw(self, n_instances: int, palettes_ptr, bounds_ptr, flags: int, pos_scale: float = 1.0,
                           morph_scale: float = 1.0) -> None:
        """mmdx_palette_bounds, the raw form: bounds_ptr[i] = {min xyz, max xyz} of a box that contains every position a deform of
        instance i from the palettes at palettes_ptr with this pos_scale writes, as long as no slot weight exceeds morph_scale.
        flags: api.PALETTE_ON_DEVICE | api.OUT_ON_DEVICE say which of the two addresses are device memory.  With both on the device
        the call is asynchronous on the model's stream and records into a graph."""
        a = api.PaletteBoundsArgs()
        a.struct_size = C.sizeof(api.PaletteBoundsArgs)
        a.flags, a.n_instances = flags, n_instances
        a.palettes, a.out_bounds = palettes_ptr, bounds_ptr
        a.pos_scale, a.morph_scale = pos_scale, morph_scale
        api.check(api.lib().mmdx_palette_bounds(self.h, C.byref(a)))

    def palette_bounds(self, palettes, pos_scale: float = 1.0, morph_scale: float = 1.0) -> np.ndarray:
        """Host array in, host array out (copies + sync inside the call): palettes [NI,NB,16] -> boxes f32 [NI,6]."""
        pal = _c(palettes, np.float32).reshape(-1, self.nb, 16)
        out = np.empty((pal.shape[0], 6), np.float32)
        self.palette_bounds_raw(pal.shape[0], pal.ctypes.data, out.ctypes.data, 0, pos_scale, morph_scale)
        return out

    def set_stream(self, stream) -> None:
        """mmdx_model_set_stream: every later call of this model (and of the motion / rig calls that take it) is enqueued on the
        caller's hipStream_t `stream` (an address, or a ctypes.c_void_p), behind everything the model enqueued before; None goes
        back to the handle's own stream.  Refused while a graph is being recorded and for a stream of another device.  The stream
        must outlive its use: switch away from it (and destroy the graphs recorded on it) before destroying it."""
        api.check(api.lib().mmdx_model_set_stream(self.h, getattr(stream, "value", stream)))

    def sync(self) -> None:
        api.check(api.lib().mmdx_sync(self.h))

    def morph_pass_stats(self) -> Tuple[int, int, int]:
        """(launches that walked the morph table, launches that found the rates unchanged on the device and skipped the walk,
        calls whose host-side comparison skipped the launch) of this model's shared morph passes."""
        w, d, h = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
        api.check(api.lib().mmdx_debug_morph_pass_stats(self.h, C.byref(w), C.byref(d), C.byref(h)))
        return w.value, d.value, h.value

    def last_store_policy(self) -> str:
        """Store flavour the kernel of the last crowd call ran with: 'nt' (cached, non-temporal) or 'sc1 nt' (write-through)."""
        wt = C.c_int32(0)
        api.check(api.lib().mmdx_debug_last_store_policy(self.h, C.byref(wt)))
        return "sc1 nt" if wt.value else "nt"

    def last_launch_shape(self) -> dict:
        """mmdx_debug_last_launch_shape: what the last deform call of this model launched -- kernel ('none' | 'deform' | 'pack' |
        'frame' | 'cull': then group = instances per chunk, ngroups = chunks, select = the form), threads, group (instances per workgroup), ngroups, lds, morph (kMorph*), layout, and the 0 / 1 fields f16,
        tile_order, bounds, select, write_through, interleave, sel_interleave."""
        s = api.DebugLaunchShape()
        s.struct_size = C.sizeof(api.DebugLaunchShape)
        api.check(api.lib().mmdx_debug_last_launch_shape(self.h, C.byref(s)))
        d = {name: int(getattr(s, name)) for name, _ in api.DebugLaunchShape._fields_ if name not in ("struct_size", "reserved0")}
        d["kernel"] = api.DEBUG_KERNELS[d["kernel"]]
        return d

    def timer_start(self) -> None:
        api.check(api.lib().mmdx_timer_start(self.h))

    def timer_stop(self) -> float:
        ms = C.c_float(0)
        api.check(api.lib().mmdx_timer_stop(self.h, C.byref(ms)))
        return float(ms.value)

    # -- HIP-graph replay of the device work of a frame ----------------------------------------------
    def graph_begin(self) -> None:
        api.check(api.lib().mmdx_graph_begin(self.h))

    def graph_end(self) -> "Graph":
        g = C.c_void_p()
        api.check(api.lib().mmdx_graph_end(self.h, C.byref(g)))
        return Graph(g)

    def profile_enable(self, on, every: int = 1) -> None:
        """Events around the morph kernels and the skinning kernel of every call, or of every `every`-th call."""
        api.check(api.lib().mmdx_profile_enable(self.h, max(int(every), 1) if on else 0))

    def profile_collect(self) -> Tuple[int, float, float]:
        """(calls, skin kernel ms total, morph pass ms total) since profile_enable / last collect."""
        n, s, m = C.c_uint32(0), C.c_float(0), C.c_float(0)
        api.check(api.lib().mmdx_profile_collect(self.h, C.byref(n), C.byref(s), C.byref(m)))
        return int(n.value), float(s.value), float(m.value)


class SocketSet:
    """mmdx_socket_set_t: chosen bones of a model whose frames mmdx_palette_sockets reads out of a crowd's palettes, on the device.
    Socket s of instance i is O[s] * G[s] * palettes[i][bones[s]] (G: the identity with row 4 = the bone's rest position; O: the
    socket's optional local offset), 16 floats in libmmd's v[0..15] order; on placed palettes that is the bone's world frame.

    bones: indices into the model's bones [NS].  rest_position: f32 [NS,3], the rest position of bones[s].  offsets: None, [NS,8]
    poses {tx,ty,tz,_,qx,qy,qz,qw} or [NS,16] / [NS,4,4] matrices.  has_offset: None (every socket has one when offsets is given) or
    bool [NS]."""

    def __init__(self, model: "DeformModel", bones, rest_position, offsets=None, has_offset=None):
        bone = np.ascontiguousarray(bones, np.uint32).reshape(-1)
        ns = bone.size
        rest = _c(rest_position, np.float32).reshape(ns, 3)
        d = api.SocketSetDesc()
        d.struct_size = C.sizeof(api.SocketSetDesc)
        d.n_sockets = ns
        d.bone, d.rest_position = bone.ctypes.data, rest.ctypes.data
        keep = [bone, rest]
        if offsets is not None:
            off = _c(offsets, np.float32).reshape(ns, -1)
            if off.shape[1] not in (api.POSE_FLOATS, 16):
                raise ValueError("offsets must be [NS,8] poses or [NS,16] matrices")
            d.flags = api.SOCKET_OFFSET_MATRIX if off.shape[1] == 16 else 0
            d.offset = off.ctypes.data
            keep.append(off)
            if has_offset is not None:
                has = np.ascontiguousarray(has_offset).astype(np.uint8).reshape(ns)
                d.has_offset = has.ctypes.data
                keep.append(has)
        elif has_offset is not None:
            raise ValueError("has_offset without offsets")
        self.h = C.c_void_p()
        api.check(api.lib().mmdx_socket_set_create(model.h, C.byref(d), C.byref(self.h)))      # copies the arrays
        info = api.SocketSetInfo()
        info.struct_size = C.sizeof(api.SocketSetInfo)
        api.check(api.lib().mmdx_socket_set_get_info(self.h, C.byref(info)))
        self.info = {k: int(getattr(info, k)) for k, _ in api.SocketSetInfo._fields_}
        self.ns, self.nb = ns, self.info["n_bones"]

    @classmethod
    def from_pmx(cls, model: "DeformModel", pmx_model, bones, offsets=None, has_offset=None) -> "SocketSet":
        """From a loaded .pmx (pmx.PmxModel, the arrays of mmdx_pmx_get_arrays): bones are indices or bone names."""
        idx = [pmx_model.bone_names.index(b) if isinstance(b, str) else int(b) for b in bones]
        return cls(model, idx, np.asarray(pmx_model.flat.bone_pos, np.float32)[idx], offsets, has_offset)

    @classmethod
    def from_skeleton(cls, model: "DeformModel", skeleton, bones, offsets=None, has_offset=None) -> "SocketSet":
        """From a vmd.Skeleton's rest positions and bone indices."""
        idx = np.asarray(bones, np.int64).reshape(-1)
        return cls(model, idx, skeleton.rest_position[idx], offsets, has_offset)

    def sockets_raw(self, n_instances: int, palettes_ptr, out_ptr, flags: int, select=None) -> None:
        """mmdx_palette_sockets, the raw form.  flags: api.PALETTE_ON_DEVICE | api.OUT_ON_DEVICE say which of the two addresses
        are device memory; select: an api.InstanceSelect (vmd.instance_select) or None = every instance."""
        a = api.SocketsArgs()
        a.struct_size = C.sizeof(api.SocketsArgs)
        a.flags, a.n_instances = flags, n_instances
        a.palettes, a.out_sockets = palettes_ptr, out_ptr
        if select is not None:
            a.select = C.pointer(select)
        api.check(api.lib().mmdx_palette_sockets(self.h, C.byref(a)))

    def sockets(self, palettes_dev, out_dev, select=None, n_instances=None) -> None:
        """Device palettes [NI][NB][16] in, device socket matrices [NS][NI][16] out (socket-major: slab s is an [NI][16] placement
        array for DeformModel.place_palettes(..., api.PLACE_MATRIX) of another model's crowd).  Asynchronous on the model's stream
        and recordable.  palettes_dev / out_dev: DeviceBuffers or raw addresses; n_instances defaults to what palettes_dev holds."""
        if n_instances is None:
            n_instances = palettes_dev.nbytes // (self.nb * 64)
        dev = lambda b: getattr(b, "ptr", b)                     # noqa: E731
        self.sockets_raw(n_instances, dev(palettes_dev), dev(out_dev), api.PALETTE_ON_DEVICE | api.OUT_ON_DEVICE, select)

    def sockets_host(self, palettes) -> np.ndarray:
        """Host array in, host array out (copies + sync inside the call): palettes [NI,NB,16] -> socket matrices [NS,NI,16]."""
        pal = _c(palettes, np.float32).reshape(-1, self.nb, 16)
        out = np.empty((self.ns, pal.shape[0], 16), np.float32)
        self.sockets_raw(pal.shape[0], pal.ctypes.data, out.ctypes.data, 0)
        return out

    def close(self) -> None:
        if getattr(self, "h", None):
            api.lib().mmdx_socket_set_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def chains_below(skeleton, roots) -> list:
    """Walk the hierarchy below each bone of `roots` into chains for SpringSet: a chain starts at a root and follows single-child
    runs (a bone with exactly one child continues, any other count ends the chain), cut at 32 joints.  skeleton: anything with
    .parent (i32 [NB], -1 = none), e.g. a vmd.Skeleton.  -> a list of lists of bone indices, one per root, the root side first."""
    parent = np.asarray(skeleton.parent, np.int64).reshape(-1)
    children = {}
    for b, p in enumerate(parent.tolist()):
        children.setdefault(p, []).append(b)
    out = []
    for r in roots:
        chain = [int(r)]
        while len(children.get(chain[-1], [])) == 1 and len(chain) < api.SPRING_MAX_JOINTS:
            chain.append(children[chain[-1]][0])
        out.append(chain)
    return out


class SpringSet:
    """mmdx_spring_set_t: chains of bones of a skeleton that swing behind their parents (hair, skirts, ribbons), per crowd instance,
    on the device.  step() advances every chain of every (listed) instance by dt in one launch and rewrites the chains' rows of a
    device palette array [NI][NB][16] in place: after DeformModel.place_palettes the simulation is in world space, before it in
    model space.  include/mmdx.h states the arithmetic.

    chains: lists of bone indices, the root side first, each bone the skeleton child of the one before it; the first bone's parent
    is the chain's anchor.  params: [n_chains,4] stiffness, drag, gravity scale, radius (or one row for all).  colliders: (bones
    [NC], spheres [NC,4] rest-space centre xyz + radius).  tails: None (the defaults) or [n_joints,3]."""

    def __init__(self, skeleton, chains, params, max_instances: int, gravity=(0.0, -9.8, 0.0), colliders=None, tails=None):
        chains = [np.ascontiguousarray(c, np.uint32).reshape(-1) for c in chains]
        off = np.zeros(len(chains) + 1, np.uint32)
        off[1:] = np.cumsum([c.size for c in chains])
        bones = np.ascontiguousarray(np.concatenate(chains) if chains else np.zeros(0), np.uint32)
        prm = np.ascontiguousarray(np.broadcast_to(_c(params, np.float32).reshape(-1, 4), (len(chains), 4)), np.float32)
        d = api.SpringSetDesc()
        d.struct_size = C.sizeof(api.SpringSetDesc)
        d.n_chains, d.max_instances = len(chains), max_instances
        d.chain_offset, d.joint_bone, d.chain_params = off.ctypes.data, bones.ctypes.data, prm.ctypes.data
        d.gravity[:] = [float(g) for g in gravity]
        keep = [off, bones, prm]
        if tails is not None:
            t = _c(tails, np.float32).reshape(bones.size, 3)
            d.joint_tail = t.ctypes.data
            keep.append(t)
        if colliders is not None and len(colliders[0]):
            cb = np.ascontiguousarray(colliders[0], np.uint32).reshape(-1)
            cs = _c(colliders[1], np.float32).reshape(cb.size, 4)
            d.n_colliders, d.collider_bone, d.collider_sphere = cb.size, cb.ctypes.data, cs.ctypes.data
            keep += [cb, cs]
        self.h = C.c_void_p()
        api.check(api.lib().mmdx_spring_set_create(skeleton.h, C.byref(d), C.byref(self.h)))      # copies the arrays
        i = self.info()
        self.n_joints, self.nb, self.max_instances = i["n_joints"], i["n_bones"], i["max_instances"]

    @classmethod
    def from_skeleton(cls, skeleton, roots, params, max_instances: int, **kw) -> "SpringSet":
        """Chains found by chains_below(skeleton, roots)."""
        return cls(skeleton, chains_below(skeleton, roots), params, max_instances, **kw)

    def info(self) -> dict:
        i = api.SpringSetInfo(C.sizeof(api.SpringSetInfo))
        api.check(api.lib().mmdx_spring_set_get_info(self.h, C.byref(i)))
        return {k: int(getattr(i, k)) for k, _ in api.SpringSetInfo._fields_ if k not in ("struct_size", "reserved0")}

    def step_raw(self, n_instances: int, palettes_ptr, dt_ptr, flags: int, select=None, model=None) -> None:
        """mmdx_spring_step, the raw form: dt_ptr is the address of one float, host memory unless flags has SPRING_DT_ON_DEVICE."""
        a = api.SpringArgs()
        a.struct_size = C.sizeof(api.SpringArgs)
        a.flags, a.n_instances = flags, n_instances
        a.palettes, a.dt = palettes_ptr, dt_ptr
        if select is not None:
            a.select = C.pointer(select)
        api.check(api.lib().mmdx_spring_step(self.h, model.h if model is not None else None, C.byref(a)))

    def step(self, palettes_dev, dt=None, dt_ptr=None, n_instances=None, select=None, model=None, reset: bool = False) -> None:
        """One step on device palettes (a DeviceBuffer or a raw address), in place, asynchronous on the model's stream and recordable
        with dt_ptr (a device float) and a device list.  dt: a host float; exactly one of dt / dt_ptr."""
        if (dt is None) == (dt_ptr is None):
            raise ValueError("exactly one of dt and dt_ptr")
        if n_instances is None:
            n_instances = palettes_dev.nbytes // (self.nb * 64)
        flags = api.PALETTE_ON_DEVICE | (api.SPRING_RESET if reset else 0)
        host = C.c_float(dt if dt is not None else 0.0)
        if dt_ptr is not None:
            flags |= api.SPRING_DT_ON_DEVICE
        self.step_raw(n_instances, getattr(palettes_dev, "ptr", palettes_dev), dt_ptr if dt_ptr is not None else C.addressof(host), flags,
                      select, model)

    def reset(self, palettes_dev, n_instances=None, select=None, model=None) -> None:
        """Every joint of the (listed) instances back to the rigid continuation of its parent: a step with MMDX_SPRING_RESET, dt = 0."""
        self.step(palettes_dev, dt=0.0, n_instances=n_instances, select=select, model=model, reset=True)

    def state(self, n_instances=None, model=None) -> np.ndarray:
        """mmdx_spring_get_state: f32 [n_instances, n_joints, 6] = current tail xyz, previous tail xyz (NaN before the first step)."""
        n = self.max_instances if n_instances is None else n_instances
        out = np.empty((n, self.n_joints, 6), np.float32)
        api.check(api.lib().mmdx_spring_get_state(self.h, model.h if model is not None else None, n, out.ctypes.data))
        return out

    def set_state(self, state, model=None) -> None:
        """mmdx_spring_set_state: f32 [n, n_joints, 6] for the first n instances."""
        s = _c(state, np.float32).reshape(-1, self.n_joints, 6)
        api.check(api.lib().mmdx_spring_set_state(self.h, model.h if model is not None else None, s.shape[0], s.ctypes.data))

    def close(self) -> None:
        if getattr(self, "h", None):
            api.lib().mmdx_spring_set_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class AimSet:
    """mmdx_aim_set_t: look-at for a crowd.  aim() turns the link bones of every aim of every (listed) instance towards the
    instance's target, in one launch, and rewrites the rows of the links' subtrees of a device palette array [NI][NB][16] in place:
    after DeformModel.place_palettes the targets are world points, before it model-space points.  It runs before SpringSet.step (hair
    anchors on the head row).  include/mmdx.h states the arithmetic.

    aims: a list of dicts {links: bone indices, the root side first, each a strict skeleton ancestor of the next; eye_bone (default:
    the last link); eye_point [3] rest-space (default: the eye bone's rest position); forward [3] rest-space (default (0, 0, -1));
    shares: per link in [0, 1] (default 1); cos_limits: per link in [-1, 1] (default -1, no limit)}."""

    def __init__(self, skeleton, aims):
        links = [np.ascontiguousarray(a["links"], np.uint32).reshape(-1) for a in aims]
        off = np.zeros(len(aims) + 1, np.uint32)
        off[1:] = np.cumsum([k.size for k in links])
        bones = np.ascontiguousarray(np.concatenate(links) if links else np.zeros(0), np.uint32)
        prm = np.ones((bones.size, 2), np.float32)
        prm[:, 1] = -1.0
        eye = np.zeros(len(aims), np.uint32)
        point, fwd = np.zeros((len(aims), 3), np.float32), np.zeros((len(aims), 3), np.float32)
        for k, a in enumerate(aims):
            lo, hi = int(off[k]), int(off[k + 1])
            if "shares" in a:
                prm[lo:hi, 0] = np.asarray(a["shares"], np.float32).reshape(-1)
            if "cos_limits" in a:
                prm[lo:hi, 1] = np.asarray(a["cos_limits"], np.float32).reshape(-1)
            eye[k] = a.get("eye_bone", links[k][-1] if links[k].size else 0)
            point[k] = a["eye_point"] if "eye_point" in a else np.asarray(skeleton.rest_position, np.float32).reshape(-1, 3)[eye[k]]
            fwd[k] = a.get("forward", (0.0, 0.0, -1.0))
        d = api.AimSetDesc()
        d.struct_size = C.sizeof(api.AimSetDesc)
        d.n_aims = len(aims)
        d.link_offset, d.link_bone, d.link_params = off.ctypes.data, bones.ctypes.data, prm.ctypes.data
        d.eye_bone, d.eye_point, d.forward = eye.ctypes.data, point.ctypes.data, fwd.ctypes.data
        self.h = C.c_void_p()
        api.check(api.lib().mmdx_aim_set_create(skeleton.h, C.byref(d), C.byref(self.h)))      # copies the arrays
        self.nb = self.info()["n_bones"]

    def info(self) -> dict:
        i = api.AimSetInfo(C.sizeof(api.AimSetInfo))
        api.check(api.lib().mmdx_aim_set_get_info(self.h, C.byref(i)))
        return {k: int(getattr(i, k)) for k, _ in api.AimSetInfo._fields_ if k != "struct_size"}

    def aim_raw(self, n_instances: int, palettes_ptr, targets_ptr, stride: int, flags: int, select=None, model=None) -> None:
        """mmdx_palette_aim, the raw form: targets_ptr is host memory unless flags has AIM_TARGETS_ON_DEVICE."""
        a = api.AimArgs()
        a.struct_size = C.sizeof(api.AimArgs)
        a.flags, a.n_instances, a.target_stride = flags, n_instances, stride
        a.palettes, a.targets = palettes_ptr, targets_ptr
        if select is not None:
            a.select = C.pointer(select)
        api.check(api.lib().mmdx_palette_aim(self.h, model.h if model is not None else None, C.byref(a)))

    def aim(self, model, palettes_dev, targets, stride: int = 4, select=None, n_instances=None) -> None:
        """Device palettes (a DeviceBuffer or a raw address) in place, asynchronous on the model's stream and recordable with device
        targets and a device list.  targets: a DeviceBuffer or a raw device address ({x, y, z, weight} every `stride` floats; stride 0:
        one target for everyone; stride 16 and the address of a mmdx_palette_sockets slab + 48 bytes: the slab's translations), or a
        numpy array [NI,4] / [4] in host memory (copied, and the call returns when the work is done)."""
        if n_instances is None:
            n_instances = palettes_dev.nbytes // (self.nb * 64)
        pal = getattr(palettes_dev, "ptr", palettes_dev)
        if isinstance(targets, np.ndarray):
            t = _c(targets, np.float32)
            stride = 0 if t.size == 4 else t.size // max(n_instances, 1)
            self.aim_raw(n_instances, pal, t.ctypes.data, stride, api.PALETTE_ON_DEVICE, select, model)
        else:
            self.aim_raw(n_instances, pal, getattr(targets, "ptr", targets), stride,
                         api.PALETTE_ON_DEVICE | api.AIM_TARGETS_ON_DEVICE, select, model)

    def close(self) -> None:
        if getattr(self, "h", None):
            api.lib().mmdx_aim_set_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class ReachSet:
    """mmdx_reach_set_t: two-bone IK for a crowd.  reach() puts the tip of every reach of every (listed) instance on the instance's
    target, in one launch, and rewrites the rows of the limbs' subtrees of a device palette array [NI][NB][16] in place: after
    DeformModel.place_palettes the targets are world points, before it model-space points.  It runs after AimSet.aim (an aimed spine
    carries the arms) and before SpringSet.step (sleeves anchor on the rows it rewrites).  include/mmdx.h states the arithmetic.

    reaches: a list of dicts {bones: (a, b, c), each a strict skeleton ancestor of the next; tip_point [3] rest-space (default: the
    rest position of c); pole [3] rest-space (default (0, 0, -1)); max_extension in (0, 1] (default 1); keep_end_rotation (default
    False): solve for the pivot of c and translate its subtree, so a planted foot keeps its orientation}."""

    def __init__(self, skeleton, reaches):
        n = len(reaches)
        bones = np.zeros((n, 3), np.uint32)
        tip, pole = np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32)
        ext, flags = np.ones(n, np.float32), np.zeros(n, np.uint32)
        for k, r in enumerate(reaches):
            bones[k] = np.asarray(r["bones"], np.uint32).reshape(3)
            tip[k] = r["tip_point"] if "tip_point" in r else np.asarray(skeleton.rest_position, np.float32).reshape(-1, 3)[bones[k, 2]]
            pole[k] = r.get("pole", (0.0, 0.0, -1.0))
            ext[k] = r.get("max_extension", 1.0)
            flags[k] = r.get("flags", api.REACH_KEEP_END_ROTATION if r.get("keep_end_rotation") else 0)
        d = api.ReachSetDesc()
        d.struct_size = C.sizeof(api.ReachSetDesc)
        d.n_reaches = n
        d.bones, d.tip_point, d.pole = bones.ctypes.data, tip.ctypes.data, pole.ctypes.data
        d.max_extension, d.flags = ext.ctypes.data, flags.ctypes.data
        self.h = C.c_void_p()
        api.check(api.lib().mmdx_reach_set_create(skeleton.h, C.byref(d), C.byref(self.h)))      # copies the arrays
        self.nb = self.info()["n_bones"]

    def info(self) -> dict:
        i = api.ReachSetInfo(C.sizeof(api.ReachSetInfo))
        api.check(api.lib().mmdx_reach_set_get_info(self.h, C.byref(i)))
        return {k: int(getattr(i, k)) for k, _ in api.ReachSetInfo._fields_ if k not in ("struct_size", "reserved0")}

    def reach_raw(self, n_instances: int, palettes_ptr, targets_ptr, stride: int, flags: int, select=None, model=None) -> None:
        """mmdx_palette_reach, the raw form: targets_ptr is host memory unless flags has REACH_TARGETS_ON_DEVICE."""
        a = api.ReachArgs()
        a.struct_size = C.sizeof(api.ReachArgs)
        a.flags, a.n_instances, a.target_stride = flags, n_instances, stride
        a.palettes, a.targets = palettes_ptr, targets_ptr
        if select is not None:
            a.select = C.pointer(select)
        api.check(api.lib().mmdx_palette_reach(self.h, model.h if model is not None else None, C.byref(a)))

    def reach(self, model, palettes_dev, targets, stride: int = 4, select=None, n_instances=None) -> None:
        """Device palettes (a DeviceBuffer or a raw address) in place, asynchronous on the model's stream and recordable with device
        targets and a device list.  targets: a DeviceBuffer or a raw device address ({x, y, z, weight} every `stride` floats; stride 0:
        one target for everyone; stride 16 and the address of a mmdx_palette_sockets slab + 48 bytes: the slab's translations), or a
        numpy array [NI,4] / [4] in host memory (copied, and the call returns when the work is done)."""
        if n_instances is None:
            n_instances = palettes_dev.nbytes // (self.nb * 64)
        pal = getattr(palettes_dev, "ptr", palettes_dev)
        if isinstance(targets, np.ndarray):
            t = _c(targets, np.float32)
            stride = 0 if t.size == 4 else t.size // max(n_instances, 1)
            self.reach_raw(n_instances, pal, t.ctypes.data, stride, api.PALETTE_ON_DEVICE, select, model)
        else:
            self.reach_raw(n_instances, pal, getattr(targets, "ptr", targets), stride,
                           api.PALETTE_ON_DEVICE | api.REACH_TARGETS_ON_DEVICE, select, model)

    def close(self) -> None:
        if getattr(self, "h", None):
            api.lib().mmdx_reach_set_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class Ground:
    """mmdx_ground_t: a regular height field in device memory.  place() puts every (listed) placement on it (only placements[i][1]
    is written), after root motion and before DeformModel.place_palettes; targets() turns the feet's world positions (a
    SocketSet.sockets output) into reach targets that keep each foot's animated height over the ground under that foot, one slab
    [NI][4] per foot for that foot's ReachSet (keep_end_rotation), and writes a hip drop that the NEXT frame's place() reads.
    include/mmdx.h states the arithmetic.

    heights: [nz][nx] floats; origin = (x, z) of heights[0][0]; cell = (x, z) distance between samples."""

    def __init__(self, heights, origin=(0.0, 0.0), cell=(1.0, 1.0)):
        h = _c(heights, np.float32)
        d = api.GroundDesc()
        d.struct_size = C.sizeof(api.GroundDesc)
        d.nz, d.nx = (h.shape if h.ndim == 2 else (0, 0))
        d.origin_x, d.origin_z = origin
        d.cell_x, d.cell_z = cell
        d.heights = h.ctypes.data
        self.h = C.c_void_p()
        api.check(api.lib().mmdx_ground_create(C.byref(d), C.byref(self.h)))      # copies the heights

    def info(self) -> dict:
        i = api.GroundInfo(C.sizeof(api.GroundInfo))
        api.check(api.lib().mmdx_ground_get_info(self.h, C.byref(i)))
        return {k: getattr(i, k) for k, _ in api.GroundInfo._fields_ if k not in ("struct_size", "reserved0")}

    def place(self, model, placements_dev, n_instances: int, drop=None, y_offset: float = 0.0, select=None, flags: int = 0) -> None:
        """mmdx_ground_place: device placements [NI][8] (a DeviceBuffer or a raw address) in place, asynchronous on the model's
        stream and recordable; drop: a DeviceBuffer / raw device address [NI] or None."""
        a = api.GroundPlaceArgs()
        a.struct_size = C.sizeof(api.GroundPlaceArgs)
        a.flags, a.n_instances, a.y_offset = flags, n_instances, y_offset
        a.placements = getattr(placements_dev, "ptr", placements_dev)
        a.drop = getattr(drop, "ptr", drop)
        if select is not None:
            a.select = C.pointer(select)
        api.check(api.lib().mmdx_ground_place(self.h, model.h if model is not None else None, C.byref(a)))

    def targets(self, model, placements_dev, points, out_targets, n_instances: int, n_feet: int, point_stride: int = 16,
                slab_stride=None, out_drop=None, max_step: float = 1.0, max_drop: float = 1.0, select=None, flags: int = 0) -> None:
        """mmdx_ground_targets: every operand a DeviceBuffer or a raw device address.  points: foot f of instance i at
        f*slab_stride + i*point_stride floats (the defaults and the address of a sockets output + 48 bytes: its translations);
        out_targets [NF][NI][4]; out_drop [NI] or None."""
        a = api.GroundTargetsArgs()
        a.struct_size = C.sizeof(api.GroundTargetsArgs)
        a.flags, a.n_instances, a.n_feet = flags, n_instances, n_feet
        a.placements = getattr(placements_dev, "ptr", placements_dev)
        a.points = getattr(points, "ptr", points)
        a.point_stride = point_stride
        a.slab_stride = n_instances * point_stride if slab_stride is None else slab_stride
        a.out_targets = getattr(out_targets, "ptr", out_targets)
        a.out_drop = getattr(out_drop, "ptr", out_drop)
        a.max_step, a.max_drop = max_step, max_drop
        if select is not None:
            a.select = C.pointer(select)
        api.check(api.lib().mmdx_ground_targets(self.h, model.h if model is not None else None, C.byref(a)))

    def close(self) -> None:
        if getattr(self, "h", None):
            api.lib().mmdx_ground_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class PoseImage:
    def __init__(self, nv: int):
        self.coordinates = np.zeros((nv, 3), np.float32)
        self.normals = np.zeros((nv, 3), np.float32)


class Poser:
    """The hot-path slice of mmd::Poser, GPU-backed.  The host keeps doing what the reference's
    frame() does upstream (motion seek, bone solve, physics) and hands over morph rates and the
    finished bone palette; Deform() then fills pose_image exactly as Poser::Deform() would."""

    def __init__(self, model: FlatModel, normalize: bool = True):
        self.model = model
        self._dm = DeformModel(model, normalize=normalize)
        self.pose_image = PoseImage(model.nv)
        self._rates = np.zeros(model.nm, np.float32)
        self._palette = np.tile(np.eye(4, dtype=np.float32).reshape(16), (model.nb, 1))
        # the reference's constructor ends with ResetPosing(); Deform()  (poser_impl.inl:126-127)
        self.Deform()

    def ResetPosing(self) -> None:
        self._rates[:] = 0.0

    def SetMorphPose(self, index: int, weight: float) -> None:
        self._rates[index] = np.float32(weight)

    def SetSkinningMatrix(self, bone: int, matrix16) -> None:
        self._palette[bone] = np.asarray(matrix16, np.float32).reshape(16)

    def SetSkinningMatrices(self, palette) -> None:
        self._palette[:] = np.asarray(palette, np.float32).reshape(self.model.nb, 16)

    def Deform(self) -> None:
        pos, nrm = self._dm.deform(self._rates, self._palette)
        self.pose_image.coordinates, self.pose_image.normals = pos, nrm

    def UpdateDeformedVertices(self, pos_scale: float = 0.1) -> np.ndarray:
        """Deform + repack in one pass on the GPU: the viewer's 32-byte vertex stream."""
        return self._dm.deform_vertex32(self._rates, self._palette, pos_scale)

    def close(self) -> None:
        self._dm.close()

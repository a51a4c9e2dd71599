"""ctypes declarations for the C ABI in include/mmdx.h (libmmdx.so, built in-tree by build.py).

This is the ONLY compute backend: if the HIP library is missing or no GPU is usable the package
raises -- there is no CPU or eager fallback to silently pass tests on.
"""
from __future__ import annotations

import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MMDX_LIB") or os.path.join(HERE, "libmmdx.so")   # MMDX_LIB: A/B of builds (tools/)

OK = 0
ABI_VERSION = 3          # include/mmdx.h MMDX_ABI_VERSION
ERR_NAMES = {1: "INVALID_ARGUMENT", 2: "BAD_INDEX", 3: "NO_DEVICE", 4: "HIP", 5: "OUT_OF_MEMORY",
             6: "UNSUPPORTED"}

CREATE_NORMALIZE, CREATE_HOST_ONLY, CREATE_F16_POSITIONS, CREATE_FAST_MATH, CREATE_TILE_ORDER = 1, 2, 4, 8, 16
OUT_SOA, OUT_VERTEX32, OUT_SOA_POS16 = 0, 1, 2
PALETTE_ON_DEVICE, WEIGHTS_ON_DEVICE, OUT_ON_DEVICE, WEIGHTS_SHARED, MORPH_UNCHANGED = 1, 2, 4, 8, 16
OUT_STORES_WRITE_THROUGH, OUT_STORES_CACHED = 32, 64
OUT_PITCHED = 128        # mmdx_deform_args.out_instance_pitch is read: instance i of the outputs starts at vertex i * pitch
SELECT_ON_DEVICE = 1     # mmdx_instance_select.flags: ids and count are device pointers
CULL_MAX_PLANES, CULL_MAX_LODS, CULLED = 16, 4, 0xFFFFFFFF      # mmdx_cull_view / mmdx_cull_bounds
CULL_VIEW_ON_DEVICE = 1  # mmdx_cull_args.flags: view is a device pointer, read when the kernel runs
PLACE_ON_DEVICE, PLACE_MATRIX = 256, 512     # mmdx_place_args.flags (with PALETTE_ON_DEVICE / OUT_ON_DEVICE): placements is a device
#                                              pointer; placements[i] is a 16-float matrix instead of an 8-float pose
POSE_FLOATS = 8          # MMDX_POSE_FLOATS: translation xyz, 0, quaternion xyzw
MASK_NONE = 0xFFFFFFFF   # MMDX_MASK_NONE: no mask, every item's mask value is 1.0f (mmdx_pose_blend / mmdx_rate_blend)
BLEND_A_ON_DEVICE, BLEND_B_ON_DEVICE, BLEND_PARAMS_ON_DEVICE = 1 << 11, 1 << 12, 1 << 13   # mmdx_row_blend_args.flags (with OUT_ON_DEVICE):
#                                              a, b, and {weights, mask_ids, masks} are device pointers
REF_NONE = 0xFFFFFFFF    # MMDX_REF_NONE: no reference row, B already is a difference (mmdx_pose_add / mmdx_rate_add)

_f32p = C.POINTER(C.c_float)
_i32p = C.POINTER(C.c_int32)
_u32p = C.POINTER(C.c_uint32)


class ModelDesc(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("flags", C.c_uint32),
                ("n_vertices", C.c_uint32), ("n_bones", C.c_uint32), ("n_morphs", C.c_uint32),
                ("reserved0", C.c_uint32),
                ("positions", _f32p), ("normals", _f32p), ("uvs", _f32p),
                ("skin_type", _i32p), ("bone_ids", _i32p), ("bone_weights", _f32p),
                ("sdef_params", _f32p), ("bone_parent", _i32p),
                ("morph_type", _i32p), ("morph_offset", _u32p), ("morph_index", _u32p),
                ("morph_value", _f32p)]


class DeformArgs(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("flags", C.c_uint32),
                ("n_instances", C.c_uint32), ("out_layout", C.c_uint32),
                ("morph_weights", C.c_void_p), ("palettes", C.c_void_p),
                ("out_a", C.c_void_p), ("out_b", C.c_void_p),
                ("pos_scale", C.c_float), ("out_instance_pitch", C.c_uint32)]


class InstanceSelect(C.Structure):
    """mmdx_instance_select: which instances a mmdx_deform_batched_select call deforms."""
    _fields_ = [("struct_size", C.c_uint32), ("flags", C.c_uint32),
                ("ids", C.c_void_p), ("count", C.c_void_p),
                ("n_ids", C.c_uint32), ("reserved0", C.c_uint32)]


class CullView(C.Structure):
    """mmdx_cull_view: planes, eye and LOD distances of one mmdx_cull_bounds call (host or device memory)."""
    _fields_ = [("planes", (C.c_float * 4) * CULL_MAX_PLANES), ("n_planes", C.c_uint32), ("n_lods", C.c_uint32),
                ("eye", C.c_float * 3), ("margin", C.c_float), ("lod_distance", C.c_float * (CULL_MAX_LODS - 1)),
                ("reserved0", C.c_uint32)]


class CullArgs(C.Structure):
    """mmdx_cull_args: bounds in, instance lists / counts / levels out (all device memory)."""
    _fields_ = [("struct_size", C.c_uint32), ("flags", C.c_uint32), ("n_instances", C.c_uint32), ("list_stride", C.c_uint32),
                ("bounds", C.c_void_p), ("view", C.c_void_p), ("out_ids", C.c_void_p), ("out_counts", C.c_void_p),
                ("out_levels", C.c_void_p)]


class PlaceArgs(C.Structure):
    """mmdx_place_args: palettes x per-instance world matrices (mmdx_palette_place)."""
    _fields_ = [("struct_size", C.c_uint32), ("flags", C.c_uint32), ("n_instances", C.c_uint32), ("reserved0", C.c_uint32),
                ("palettes", C.c_void_p), ("placements", C.c_void_p), ("out_palettes", C.c_void_p)]


SOCKET_OFFSET_MATRIX = 1    # mmdx_socket_set_desc.flags: offsets are [NS][16] matrices (else [NS][8] poses)


class SocketSetDesc(C.Structure):
    """mmdx_socket_set_desc: the bones, their rest positions and the local offsets of a socket set (mmdx_socket_set_create)."""
    _fields_ = [("struct_size", C.c_uint32), ("flags", C.c_uint32), ("n_sockets", C.c_uint32), ("reserved0", C.c_uint32),
                ("bone", C.c_void_p), ("rest_position", C.c_void_p), ("offset", C.c_void_p), ("has_offset", C.c_void_p)]


class SocketSetInfo(C.Structure):
    """mmdx_socket_set_info (mmdx_socket_set_get_info)."""
    _fields_ = [("struct_size", C.c_uint32), ("n_sockets", C.c_uint32), ("n_offsets", C.c_uint32), ("n_bones", C.c_uint32),
                ("device_ordinal", C.c_int32), ("reserved0", C.c_uint32)]


class SocketsArgs(C.Structure):
    """mmdx_sockets_args: palettes in, [NS][NI][16] socket matrices out (mmdx_palette_sockets)."""
    _fields_ = [("struct_size", C.c_uint32), ("flags", C.c_uint32), ("n_instances", C.c_uint32), ("reserved0", C.c_uint32),
                ("palettes", C.c_void_p), ("out_sockets", C.c_void_p), ("select", C.POINTER(InstanceSelect))]


class RowBlendArgs(C.Structure):
    """mmdx_row_blend_args: two pose or rate arrays, a weight and a mask row per instance (mmdx_pose_blend / mmdx_rate_blend)."""
    _fields_ = [("struct_size", C.c_uint32), ("flags", C.c_uint32), ("n_instances", C.c_uint32), ("row_items", C.c_uint32),
                ("a", C.c_void_p), ("b", C.c_void_p), ("weights", C.c_void_p), ("mask_ids", C.c_void_p), ("masks", C.c_void_p),
                ("n_masks", C.c_uint32), ("reserved0", C.c_uint32), ("out", C.c_void_p)]


class RowAddArgs(C.Structure):
    """mmdx_row_add_args: mmdx_row_blend_args plus the reference rows of an additive layer (mmdx_pose_add / mmdx_rate_add)."""
    _fields_ = RowBlendArgs._fields_ + [("ref_ids", C.c_void_p), ("refs", C.c_void_p), ("n_refs", C.c_uint32), ("reserved1", C.c_uint32)]


ROOT_X, ROOT_Y, ROOT_Z = 1, 2, 4          # MMDX_ROOT_*: the axes of mmdx_animator_root_motion / mmdx_bone_motion_in_place


class RootMotionArgs(C.Structure):
    """mmdx_root_motion_args: the root bone, the axes, the step and the placements of mmdx_animator_root_motion."""
    _fields_ = [("struct_size", C.c_uint32), ("flags", C.c_uint32), ("root_bone", C.c_uint32), ("axes", C.c_uint32),
                ("dt", C.c_void_p), ("placements", C.c_void_p)]


ROOT_NORMALIZE = 1 << 14                  # MMDX_ROOT_NORMALIZE: mmdx_animator_root_motion_turn normalises the heading it wrote


class RootTurnArgs(C.Structure):
    """mmdx_root_turn_args: mmdx_root_motion_args' fields, its own type, for mmdx_animator_root_motion_turn."""
    _fields_ = list(RootMotionArgs._fields_)


EVENTS_DOMINANT_SIDE = 1 << 15            # MMDX_EVENTS_DOMINANT_SIDE: mmdx_animator_events lets only the heavier side of a fade fire
EVENTS_MAX_LISTS = 4                      # MMDX_EVENTS_MAX_LISTS


class EventMarker(C.Structure):
    """mmdx_event_marker: a time in a clip and the channel (< 32) it fires."""
    _fields_ = [("time", C.c_double), ("clip", C.c_uint32), ("channel", C.c_uint32)]


class EventSetDesc(C.Structure):
    """mmdx_event_set_desc: the markers of mmdx_event_set_create, host memory, any order."""
    _fields_ = [("struct_size", C.c_uint32), ("n_markers", C.c_uint32), ("markers", C.c_void_p)]


class EventSetInfo(C.Structure):
    """mmdx_event_set_info (mmdx_event_set_get_info)."""
    _fields_ = [("struct_size", C.c_uint32), ("n_markers", C.c_uint32), ("n_clips", C.c_uint32), ("device_ordinal", C.c_int32)]


class EventsArgs(C.Structure):
    """mmdx_events_args: the step, the per-instance masks and the instance lists of mmdx_animator_events (all outputs device memory)."""
    _fields_ = [("struct_size", C.c_uint32), ("flags", C.c_uint32), ("dt", C.c_void_p), ("out_fired", C.c_void_p),
                ("n_lists", C.c_uint32), ("list_stride", C.c_uint32), ("list_mask", C.c_uint32 * EVENTS_MAX_LISTS),
                ("levels", C.c_void_p), ("out_ids", C.c_void_p), ("out_counts", C.c_void_p)]


SPRING_RESET, SPRING_DT_ON_DEVICE = 1 << 16, 1 << 17     # MMDX_SPRING_*: mmdx_spring_args.flags (with PALETTE_ON_DEVICE, required)
SPRING_MAX_JOINTS, SPRING_MAX_COLLIDERS = 32, 16          # MMDX_SPRING_MAX_*


class SpringSetDesc(C.Structure):
    """mmdx_spring_set_desc: chains of bones, their parameters, the colliders and gravity of a spring set (mmdx_spring_set_create)."""
    _fields_ = [("struct_size", C.c_uint32), ("n_chains", C.c_uint32), ("n_colliders", C.c_uint32), ("max_instances", C.c_uint32),
                ("chain_offset", C.c_void_p), ("joint_bone", C.c_void_p), ("joint_tail", C.c_void_p), ("chain_params", C.c_void_p),
                ("collider_bone", C.c_void_p), ("collider_sphere", C.c_void_p), ("gravity", C.c_float * 3), ("reserved0", C.c_uint32)]


class SpringSetInfo(C.Structure):
    """mmdx_spring_set_info (mmdx_spring_set_get_info)."""
    _fields_ = [("struct_size", C.c_uint32), ("n_chains", C.c_uint32), ("n_joints", C.c_uint32), ("n_colliders", C.c_uint32),
                ("max_instances", C.c_uint32), ("n_bones", C.c_uint32), ("device_ordinal", C.c_int32), ("reserved0", C.c_uint32)]


class SpringArgs(C.Structure):
    """mmdx_spring_args: device palettes rewritten in place, the step and the instance list of mmdx_spring_step."""
    _fields_ = [("struct_size", C.c_uint32), ("flags", C.c_uint32), ("n_instances", C.c_uint32), ("reserved0", C.c_uint32),
                ("palettes", C.c_void_p), ("dt", C.c_void_p), ("select", C.POINTER(InstanceSelect))]


AIM_TARGETS_ON_DEVICE = 1 << 18                           # MMDX_AIM_TARGETS_ON_DEVICE: mmdx_aim_args.flags (with PALETTE_ON_DEVICE, required)
AIM_MAX_AIMS, AIM_MAX_LINKS = 16, 4                       # MMDX_AIM_MAX_*


class AimSetDesc(C.Structure):
    """mmdx_aim_set_desc: the link bones, their shares and limits, and the eye of every aim of an aim set (mmdx_aim_set_create)."""
    _fields_ = [("struct_size", C.c_uint32), ("n_aims", C.c_uint32), ("link_offset", C.c_void_p), ("link_bone", C.c_void_p),
                ("link_params", C.c_void_p), ("eye_bone", C.c_void_p), ("eye_point", C.c_void_p), ("forward", C.c_void_p),
                ("reserved0", C.c_uint32)]


class AimSetInfo(C.Structure):
    """mmdx_aim_set_info (mmdx_aim_set_get_info)."""
    _fields_ = [("struct_size", C.c_uint32), ("n_aims", C.c_uint32), ("n_links", C.c_uint32), ("n_subtree_rows", C.c_uint32),
                ("n_bones", C.c_uint32), ("device_ordinal", C.c_int32)]


class AimArgs(C.Structure):
    """mmdx_aim_args: device palettes rewritten in place, the targets and the instance list of mmdx_palette_aim."""
    _fields_ = [("struct_size", C.c_uint32), ("flags", C.c_uint32), ("n_instances", C.c_uint32), ("target_stride", C.c_uint32),
                ("palettes", C.c_void_p), ("targets", C.c_void_p), ("select", C.POINTER(InstanceSelect))]


REACH_TARGETS_ON_DEVICE = 1 << 19                         # MMDX_REACH_TARGETS_ON_DEVICE: mmdx_reach_args.flags (with PALETTE_ON_DEVICE, required)
REACH_MAX_REACHES = 16                                    # MMDX_REACH_MAX_REACHES
REACH_KEEP_END_ROTATION = 1                               # MMDX_REACH_KEEP_END_ROTATION: mmdx_reach_set_desc.flags[r]


class ReachSetDesc(C.Structure):
    """mmdx_reach_set_desc: the three bones, the tip point, the pole, the extension and the flags of every reach of a reach set
    (mmdx_reach_set_create)."""
    _fields_ = [("struct_size", C.c_uint32), ("n_reaches", C.c_uint32), ("bones", C.c_void_p), ("tip_point", C.c_void_p),
                ("pole", C.c_void_p), ("max_extension", C.c_void_p), ("flags", C.c_void_p), ("reserved0", C.c_uint32)]


class ReachSetInfo(C.Structure):
    """mmdx_reach_set_info (mmdx_reach_set_get_info)."""
    _fields_ = [("struct_size", C.c_uint32), ("n_reaches", C.c_uint32), ("n_subtree_rows", C.c_uint32), ("n_bones", C.c_uint32),
                ("device_ordinal", C.c_int32), ("reserved0", C.c_uint32)]


class ReachArgs(C.Structure):
    """mmdx_reach_args: device palettes rewritten in place, the targets and the instance list of mmdx_palette_reach."""
    _fields_ = [("struct_size", C.c_uint32), ("flags", C.c_uint32), ("n_instances", C.c_uint32), ("target_stride", C.c_uint32),
                ("palettes", C.c_void_p), ("targets", C.c_void_p), ("select", C.POINTER(InstanceSelect))]


class BoneMotionKeys(C.Structure):
    """mmdx_bone_motion_keys: the host key tables of a bound bone motion (mmdx_bone_motion_get_keys)."""
    _fields_ = [("struct_size", C.c_uint32), ("n_bones", C.c_uint32), ("n_keys", C.c_uint32), ("n_curves", C.c_uint32),
                ("key_off", _u32p), ("key_frame", _u32p), ("key_tr", _f32p), ("key_rot", _f32p), ("key_curve", _u32p), ("lut", _f32p)]


class BoneBoxInfo(C.Structure):
    """mmdx_bone_box_info: the scalars of a model's bone-box table (mmdx_model_get_bone_boxes)."""
    _fields_ = [("struct_size", C.c_uint32), ("n_boxes", C.c_uint32), ("n_nonconvex", C.c_uint32), ("max_vertex_entries", C.c_uint32),
                ("eps", C.c_float), ("weight_sum_dev", C.c_float), ("reserved0", C.c_uint32 * 2)]


class PaletteBoundsArgs(C.Structure):
    """mmdx_palette_bounds_args: palettes in, one conservative box per instance out (mmdx_palette_bounds)."""
    _fields_ = [("struct_size", C.c_uint32), ("flags", C.c_uint32), ("n_instances", C.c_uint32), ("reserved0", C.c_uint32),
                ("palettes", C.c_void_p), ("out_bounds", C.c_void_p), ("pos_scale", C.c_float), ("morph_scale", C.c_float)]


class ModelInfo(C.Structure):
    _fields_ = [("struct_size", C.c_uint32),
                ("n_vertices", C.c_uint32), ("n_bones", C.c_uint32), ("n_morphs", C.c_uint32),
                ("n_slots", C.c_uint32), ("n_entries", C.c_uint32), ("n_entries_padded", C.c_uint32),
                ("n_tiles", C.c_uint32), ("tile_vertices", C.c_uint32),
                ("n_bdef1", C.c_uint32), ("n_bdef2", C.c_uint32), ("n_bdef4", C.c_uint32),
                ("max_tile_bones", C.c_uint32),
                ("device_bytes", C.c_uint64),
                ("device_ordinal", C.c_uint32), ("flags", C.c_uint32), ("reserved0", C.c_uint32)]


class DebugLaunchShape(C.Structure):
    """mmdx_debug_launch_shape (include/mmdx_bench.h): the shape of a model's last deform launch."""
    _fields_ = [("struct_size", C.c_uint32), ("kernel", C.c_uint32), ("threads", C.c_uint32), ("group", C.c_uint32),
                ("ngroups", C.c_uint32), ("lds", C.c_uint32), ("morph", C.c_uint32), ("layout", C.c_uint32),
                ("f16", C.c_uint32), ("tile_order", C.c_uint32), ("bounds", C.c_uint32), ("select", C.c_uint32),
                ("write_through", C.c_uint32), ("interleave", C.c_uint32), ("sel_interleave", C.c_uint32),
                ("reserved0", C.c_uint32)]


GROUND_MAX_FEET = 8                                       # MMDX_GROUND_MAX_FEET
GROUND_H_ERROR = 6e-7                                     # MMDX_GROUND_H_ERROR


class GroundDesc(C.Structure):
    """mmdx_ground_desc: a regular height field, heights [nz][nx] in host memory (mmdx_ground_create copies them)."""
    _fields_ = [("struct_size", C.c_uint32), ("flags", C.c_uint32), ("nx", C.c_uint32), ("nz", C.c_uint32),
                ("origin_x", C.c_float), ("origin_z", C.c_float), ("cell_x", C.c_float), ("cell_z", C.c_float),
                ("heights", C.c_void_p), ("reserved0", C.c_uint32)]


class GroundInfo(C.Structure):
    """mmdx_ground_info (mmdx_ground_get_info)."""
    _fields_ = [("struct_size", C.c_uint32), ("nx", C.c_uint32), ("nz", C.c_uint32),
                ("origin_x", C.c_float), ("origin_z", C.c_float), ("cell_x", C.c_float), ("cell_z", C.c_float),
                ("min_height", C.c_float), ("max_height", C.c_float), ("device_ordinal", C.c_int32), ("reserved0", C.c_uint32)]


class GroundPlaceArgs(C.Structure):
    """mmdx_ground_place_args: device placements whose [i][1] is rewritten, the drop and the instance list of mmdx_ground_place."""
    _fields_ = [("struct_size", C.c_uint32), ("flags", C.c_uint32), ("n_instances", C.c_uint32), ("y_offset", C.c_float),
                ("placements", C.c_void_p), ("drop", C.c_void_p), ("select", C.POINTER(InstanceSelect))]


class GroundTargetsArgs(C.Structure):
    """mmdx_ground_targets_args: device placements and foot points in, reach targets and the hip drop out (mmdx_ground_targets)."""
    _fields_ = [("struct_size", C.c_uint32), ("flags", C.c_uint32), ("n_instances", C.c_uint32), ("n_feet", C.c_uint32),
                ("placements", C.c_void_p), ("points", C.c_void_p), ("point_stride", C.c_uint32), ("slab_stride", C.c_uint32),
                ("out_targets", C.c_void_p), ("out_drop", C.c_void_p), ("max_step", C.c_float), ("max_drop", C.c_float),
                ("select", C.POINTER(InstanceSelect))]


DEBUG_KERNELS = ("none", "deform", "pack", "frame", "cull", "aim", "reach")      # mmdx_debug_kernel


class DebugSolveShape(C.Structure):
    """mmdx_debug_solve_shape (include/mmdx_bench.h): what a skeleton's last solve launched."""
    _fields_ = [("struct_size", C.c_uint32), ("solver", C.c_uint32), ("nested", C.c_uint32), ("dense", C.c_uint32),
                ("select", C.c_uint32), ("workgroups", C.c_uint32), ("lds", C.c_uint32), ("segments", C.c_uint32),
                ("coop_launches", C.c_uint32), ("reserved0", C.c_uint32)]


DEBUG_SOLVERS = ("none", "ordered", "parallel_fk")               # mmdx_debug_solver


class MmdxError(RuntimeError):
    def __init__(self, status: int, message: str):
        super().__init__(f"mmdx error {status} ({ERR_NAMES.get(status, '?')}): {message}")
        self.status = status


# every entry point include/mmdx.h and include/mmdx_bench.h declare: name -> (restype, argtypes)
SIGNATURES = {
    "mmdx_abi_version": (C.c_uint32, []),
    "mmdx_last_error_string": (C.c_char_p, []),
    "mmdx_device_count": (C.c_int32, [C.POINTER(C.c_int32)]),
    "mmdx_device_select": (C.c_int32, [C.c_int32]),
    "mmdx_device_name": (C.c_int32, [C.c_int32, C.c_char_p, C.c_size_t]),
    "mmdx_model_create": (C.c_int32, [C.POINTER(ModelDesc), C.POINTER(C.c_void_p)]),
    "mmdx_model_destroy": (C.c_int32, [C.c_void_p]),
    "mmdx_model_get_info": (C.c_int32, [C.c_void_p, C.POINTER(ModelInfo)]),
    "mmdx_model_get_skin": (C.c_int32, [C.c_void_p, _i32p, _i32p, _f32p]),
    "mmdx_model_get_vertex_order": (C.c_int32, [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "mmdx_model_slot_weights": (C.c_int32, [C.c_void_p, _f32p, _f32p]),
    "mmdx_model_set_stream": (C.c_int32, [C.c_void_p, C.c_void_p]),
    "mmdx_deform": (C.c_int32, [C.c_void_p, _f32p, _f32p, _f32p, _f32p]),
    "mmdx_deform_vertex32": (C.c_int32, [C.c_void_p, _f32p, _f32p, C.c_float, C.c_void_p]),
    "mmdx_deform_batched": (C.c_int32, [C.c_void_p, C.POINTER(DeformArgs)]),
    "mmdx_deform_batched_bounds": (C.c_int32, [C.c_void_p, C.POINTER(DeformArgs), C.c_void_p]),
    "mmdx_deform_batched_select": (C.c_int32, [C.c_void_p, C.POINTER(DeformArgs), C.POINTER(InstanceSelect), C.c_void_p]),
    "mmdx_cull_bounds": (C.c_int32, [C.c_void_p, C.POINTER(CullArgs)]),
    "mmdx_cull_planes_from_matrix": (C.c_int32, [_f32p, C.c_uint32, _f32p]),
    "mmdx_palette_place": (C.c_int32, [C.c_void_p, C.POINTER(PlaceArgs)]),
    # bone sockets: (model, desc, out_set), (set), (set, info), (set, mmdx_sockets_args*)
    "mmdx_socket_set_create": (C.c_int32, [C.c_void_p, C.POINTER(SocketSetDesc), C.POINTER(C.c_void_p)]),
    "mmdx_socket_set_destroy": (None, [C.c_void_p]),
    "mmdx_socket_set_get_info": (C.c_int32, [C.c_void_p, C.POINTER(SocketSetInfo)]),
    "mmdx_palette_sockets": (C.c_int32, [C.c_void_p, C.POINTER(SocketsArgs)]),
    "mmdx_model_get_bone_boxes": (C.c_int32, [C.c_void_p, C.POINTER(BoneBoxInfo), _u32p, _f32p]),
    "mmdx_palette_bounds": (C.c_int32, [C.c_void_p, C.POINTER(PaletteBoundsArgs)]),
    "mmdx_sync": (C.c_int32, [C.c_void_p]),
    "mmdx_timer_start": (C.c_int32, [C.c_void_p]),
    "mmdx_timer_stop": (C.c_int32, [C.c_void_p, _f32p]),
    "mmdx_profile_enable": (C.c_int32, [C.c_void_p, C.c_int32]),
    "mmdx_profile_collect": (C.c_int32, [C.c_void_p, _u32p, _f32p, _f32p]),
    "mmdx_device_malloc": (C.c_int32, [C.POINTER(C.c_void_p), C.c_size_t]),
    "mmdx_device_free": (C.c_int32, [C.c_void_p]),
    "mmdx_host_malloc": (C.c_int32, [C.POINTER(C.c_void_p), C.c_size_t]),
    "mmdx_host_free": (C.c_int32, [C.c_void_p]),
    "mmdx_memcpy_h2d": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_size_t]),
    "mmdx_memcpy_d2h": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_size_t]),
    "mmdx_device_memset": (C.c_int32, [C.c_void_p, C.c_int, C.c_size_t]),
    "mmdx_device_synchronize": (C.c_int32, []),
    "mmdx_debug_reload_env": (None, []),
    "mmdx_debug_last_store_policy": (C.c_int32, [C.c_void_p, C.POINTER(C.c_int32)]),
    "mmdx_debug_last_launch_shape": (C.c_int32, [C.c_void_p, C.POINTER(DebugLaunchShape)]),
    "mmdx_debug_last_solve_shape": (C.c_int32, [C.c_void_p, C.POINTER(DebugSolveShape)]),
    "mmdx_debug_morph_pass_stats": (C.c_int32, [C.c_void_p, _u32p, _u32p, _u32p]),
    "mmdx_build_source_sha": (C.c_char_p, []),
    "mmdx_bench_copy": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int32, _f32p]),
    "mmdx_bench_fill": (C.c_int32, [C.c_void_p, C.c_size_t, C.c_int32, _f32p]),
    "mmdx_bench_store_pattern": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_int32, _f32p]),
    "mmdx_pmx_parse": (C.c_int32, [C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p)]),
    "mmdx_pmx_load_file": (C.c_int32, [C.c_char_p, C.POINTER(C.c_void_p)]),
    "mmdx_pmd_parse": (C.c_int32, [C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p)]),
    "mmdx_pmd_load_file": (C.c_int32, [C.c_char_p, C.POINTER(C.c_void_p)]),
    "mmdx_pmx_destroy": (None, [C.c_void_p]),
    "mmdx_pmx_get_info": (C.c_int32, [C.c_void_p, C.c_void_p]),
    "mmdx_pmx_get_model_desc": (C.c_int32, [C.c_void_p, C.POINTER(ModelDesc)]),
    "mmdx_pmx_get_arrays": (C.c_int32, [C.c_void_p, C.c_void_p]),
    "mmdx_pmx_get_name": (C.c_int32, [C.c_void_p, C.c_int32, C.c_uint32, C.c_char_p, C.c_size_t]),
    "mmdx_crowd_output_alloc": (C.c_int32, [C.c_void_p, C.c_uint32, C.c_int32, C.c_uint32, C.POINTER(C.c_void_p),
                                            C.POINTER(C.c_void_p), C.c_void_p]),
    "mmdx_model_output_pitch": (C.c_int32, [C.c_void_p, C.c_int32, _u32p]),
    "mmdx_crowd_output_alloc_pitched": (C.c_int32, [C.c_void_p, C.c_uint32, C.c_int32, C.c_uint32, C.c_uint32,
                                                    C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_void_p]),
    "mmdx_vmd_parse": (C.c_int32, [C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p)]),
    "mmdx_vmd_load_file": (C.c_int32, [C.c_char_p, C.POINTER(C.c_void_p)]),
    "mmdx_vmd_destroy": (None, [C.c_void_p]),
    "mmdx_vmd_get_info": (C.c_int32, [C.c_void_p, C.c_void_p]),
    "mmdx_vmd_track_name": (C.c_int32, [C.c_void_p, C.c_int32, C.c_uint32, C.c_char_p, C.c_size_t]),
    "mmdx_vmd_bone_track": (C.c_int32, [C.c_void_p, C.c_uint32, C.c_void_p, _u32p]),
    "mmdx_vmd_morph_track": (C.c_int32, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, _u32p]),
    "mmdx_vmd_bind_morphs": (C.c_int32, [C.c_void_p, C.c_uint32, C.POINTER(C.c_char_p), C.POINTER(C.c_void_p)]),
    "mmdx_morph_motion_get_info": (C.c_int32, [C.c_void_p, _u32p, _u32p, _u32p]),
    "mmdx_morph_motion_eval": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p]),
    "mmdx_morph_motion_eval_time": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p]),
    "mmdx_morph_motion_destroy": (None, [C.c_void_p]),
    "mmdx_vmd_bind_bones": (C.c_int32, [C.c_void_p, C.c_uint32, C.POINTER(C.c_char_p), C.POINTER(C.c_void_p)]),
    "mmdx_bone_motion_get_info": (C.c_int32, [C.c_void_p, _u32p, _u32p, _u32p, _u32p]),
    "mmdx_bone_motion_eval": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p]),
    "mmdx_bone_motion_eval_time": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p]),
    "mmdx_bone_motion_destroy": (None, [C.c_void_p]),
    "mmdx_skeleton_create": (C.c_int32, [C.c_void_p, C.POINTER(C.c_void_p)]),
    "mmdx_skeleton_get_info": (C.c_int32, [C.c_void_p, C.c_void_p]),
    "mmdx_skeleton_solve": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p]),
    "mmdx_skeleton_solve_motion": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p]),
    "mmdx_skeleton_solve_motion_time": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32,
                                                    C.c_void_p]),
    "mmdx_motion_set_create": (C.c_int32, [C.c_uint32, C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p)]),
    "mmdx_motion_set_get_info": (C.c_int32, [C.c_void_p, C.c_void_p]),
    "mmdx_motion_set_destroy": (None, [C.c_void_p]),
    # (set, model, n_instances, clips, frames | times, flags, out)
    "mmdx_motion_set_eval_bones": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]),
    "mmdx_motion_set_eval_bones_time": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32,
                                                    C.c_void_p]),
    "mmdx_motion_set_eval_morphs": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]),
    "mmdx_motion_set_eval_morphs_time": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32,
                                                     C.c_void_p]),
    "mmdx_skeleton_solve_motion_set": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32,
                                                   C.c_void_p]),
    "mmdx_skeleton_solve_motion_set_time": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p,
                                                        C.c_uint32, C.c_void_p]),
    # (set, model, mmdx_motion_blend_args*, out) and (skeleton, set, model, mmdx_motion_blend_args*, out)
    "mmdx_motion_set_blend_bones_time": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mmdx_motion_set_blend_morphs_time": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mmdx_skeleton_solve_motion_set_blend_time": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    # the same three for the listed instances: (set, model, args*, mmdx_instance_select*, out) and (skeleton, set, model, args*, select*, out)
    "mmdx_motion_set_blend_bones_time_select": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(InstanceSelect), C.c_void_p]),
    "mmdx_motion_set_blend_morphs_time_select": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(InstanceSelect), C.c_void_p]),
    "mmdx_skeleton_solve_motion_set_blend_time_select": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                                     C.POINTER(InstanceSelect), C.c_void_p]),
    # the crowd animator: (set, last_frames); (set, mmdx_animator_desc*, out); (animator, info*, clips*); (animator, blend args*);
    # (animator, arrays*); (animator, model, arrays*) x 2; (animator, model, n, ids, clips, fades, start_times, flags);
    # (animator, model, dt*, flags)
    "mmdx_motion_set_clip_frames": (C.c_int32, [C.c_void_p, C.c_void_p]),
    "mmdx_animator_create": (C.c_int32, [C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p)]),
    "mmdx_animator_destroy": (None, [C.c_void_p]),
    "mmdx_animator_get_info": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "mmdx_animator_operands": (C.c_int32, [C.c_void_p, C.c_void_p]),
    "mmdx_animator_device_arrays": (C.c_int32, [C.c_void_p, C.c_void_p]),
    "mmdx_animator_set_state": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "mmdx_animator_get_state": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "mmdx_animator_request": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32]),
    "mmdx_animator_advance": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32]),
    # root motion: (animator, set, model, mmdx_root_motion_args*); (bone motion, bone, axes, out)
    "mmdx_animator_root_motion": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(RootMotionArgs)]),
    "mmdx_bone_motion_in_place": (C.c_int32, [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_void_p)]),
    "mmdx_animator_root_motion_turn": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(RootTurnArgs)]),
    "mmdx_bone_motion_in_place_turn": (C.c_int32, [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_void_p)]),
    # clip markers: (animator, mmdx_event_set_desc*, out_set); (set); (set, info*); (animator, set, model, mmdx_events_args*)
    "mmdx_event_set_create": (C.c_int32, [C.c_void_p, C.POINTER(EventSetDesc), C.POINTER(C.c_void_p)]),
    "mmdx_event_set_destroy": (None, [C.c_void_p]),
    "mmdx_event_set_get_info": (C.c_int32, [C.c_void_p, C.POINTER(EventSetInfo)]),
    "mmdx_animator_events": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(EventsArgs)]),
    # spring bones: (skeleton, desc, out_set); (set); (set, info*); (set, model, mmdx_spring_args*); (set, model, n, state) x 2
    "mmdx_spring_set_create": (C.c_int32, [C.c_void_p, C.POINTER(SpringSetDesc), C.POINTER(C.c_void_p)]),
    "mmdx_spring_set_destroy": (None, [C.c_void_p]),
    "mmdx_spring_set_get_info": (C.c_int32, [C.c_void_p, C.POINTER(SpringSetInfo)]),
    "mmdx_spring_step": (C.c_int32, [C.c_void_p, C.c_void_p, C.POINTER(SpringArgs)]),
    "mmdx_spring_get_state": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]),
    "mmdx_spring_set_state": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]),
    # look-at: (skeleton, desc, out_set); (set); (set, info*); (set, model, mmdx_aim_args*)
    "mmdx_aim_set_create": (C.c_int32, [C.c_void_p, C.POINTER(AimSetDesc), C.POINTER(C.c_void_p)]),
    "mmdx_aim_set_destroy": (None, [C.c_void_p]),
    "mmdx_aim_set_get_info": (C.c_int32, [C.c_void_p, C.POINTER(AimSetInfo)]),
    "mmdx_palette_aim": (C.c_int32, [C.c_void_p, C.c_void_p, C.POINTER(AimArgs)]),
    # reach: (skeleton, desc, out_set); (set); (set, info*); (set, model, mmdx_reach_args*)
    "mmdx_reach_set_create": (C.c_int32, [C.c_void_p, C.POINTER(ReachSetDesc), C.POINTER(C.c_void_p)]),
    "mmdx_reach_set_destroy": (None, [C.c_void_p]),
    "mmdx_reach_set_get_info": (C.c_int32, [C.c_void_p, C.POINTER(ReachSetInfo)]),
    "mmdx_palette_reach": (C.c_int32, [C.c_void_p, C.c_void_p, C.POINTER(ReachArgs)]),
    # ground: (desc, out_ground); (ground); (ground, info*); (ground, model, mmdx_ground_place_args*); (ground, model, mmdx_ground_targets_args*)
    "mmdx_ground_create": (C.c_int32, [C.POINTER(GroundDesc), C.POINTER(C.c_void_p)]),
    "mmdx_ground_destroy": (None, [C.c_void_p]),
    "mmdx_ground_get_info": (C.c_int32, [C.c_void_p, C.POINTER(GroundInfo)]),
    "mmdx_ground_place": (C.c_int32, [C.c_void_p, C.c_void_p, C.POINTER(GroundPlaceArgs)]),
    "mmdx_ground_targets": (C.c_int32, [C.c_void_p, C.c_void_p, C.POINTER(GroundTargetsArgs)]),
    "mmdx_bone_motion_get_keys": (C.c_int32, [C.c_void_p, C.POINTER(BoneMotionKeys)]),
    "mmdx_skeleton_solve_morphed": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32,
                                                C.c_void_p]),
    # (skeleton, model, n_instances, poses, morph_weights, flags, mmdx_instance_select*, out)
    "mmdx_skeleton_solve_select": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32,
                                               C.POINTER(InstanceSelect), C.c_void_p]),
    "mmdx_skeleton_solve_pre": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32,
                                            C.c_void_p]),
    "mmdx_skeleton_solve_post": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p]),
    # the masked blend of two evaluated arrays: (model, mmdx_row_blend_args*, mmdx_instance_select* or NULL); and a mask row from the
    # hierarchy: (skeleton, n_roots, roots, inside, outside, out_mask)
    "mmdx_pose_blend": (C.c_int32, [C.c_void_p, C.POINTER(RowBlendArgs), C.POINTER(InstanceSelect)]),
    "mmdx_rate_blend": (C.c_int32, [C.c_void_p, C.POINTER(RowBlendArgs), C.POINTER(InstanceSelect)]),
    "mmdx_skeleton_subtree_mask": (C.c_int32, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_float, C.c_float, C.c_void_p]),
    # additive layers: (model, mmdx_row_add_args*, mmdx_instance_select* or NULL)
    "mmdx_pose_add": (C.c_int32, [C.c_void_p, C.POINTER(RowAddArgs), C.POINTER(InstanceSelect)]),
    "mmdx_rate_add": (C.c_int32, [C.c_void_p, C.POINTER(RowAddArgs), C.POINTER(InstanceSelect)]),
    "mmdx_skeleton_destroy": (None, [C.c_void_p]),
    "mmdx_graph_begin": (C.c_int32, [C.c_void_p]),
    "mmdx_graph_end": (C.c_int32, [C.c_void_p, C.POINTER(C.c_void_p)]),
    "mmdx_graph_launch": (C.c_int32, [C.c_void_p]),
    "mmdx_graph_destroy": (None, [C.c_void_p]),
    "mmdx_pmx_get_skeleton_desc": (C.c_int32, [C.c_void_p, C.c_void_p]),
}

_lib = None


def lib() -> C.CDLL:
    """Load libmmdx.so (once).  Raises if it has not been built: no fallback exists."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} is missing: build it with `python -m simple_mmd_renderer_amd.build` "
                "(hipcc, gfx950).  simple_mmd_renderer_amd has no CPU fallback.")
        l = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(l, name)
            fn.restype, fn.argtypes = res, args
        if l.mmdx_abi_version() != ABI_VERSION:
            raise RuntimeError("libmmdx.so ABI version mismatch")
        _lib = l
    return _lib


def library_source_sha() -> str:
    """The source revision stamped into the loaded library (mmdx_bench.h, mmdx_build_source_sha)."""
    return (lib().mmdx_build_source_sha() or b"").decode()


def check_library_matches_tree() -> dict:
    """The loaded library must have been built from the sources in this tree: returns both hashes, raises on a mismatch
    (MMDX_LIB experiment builds are exempt: tools/ compare variants on purpose)."""
    from . import build
    lib_sha, tree_sha = library_source_sha(), build.source_sha()
    if lib_sha != tree_sha and not os.environ.get("MMDX_LIB"):
        raise RuntimeError(f"libmmdx.so was built from other sources than this tree's (library {lib_sha}, tree {tree_sha}): "
                           "rebuild with `python -m simple_mmd_renderer_amd.build`")
    return {"library_source_sha": lib_sha, "tree_source_sha": tree_sha}


def check(status: int) -> None:
    if status != OK:
        raise MmdxError(status, (lib().mmdx_last_error_string() or b"").decode("utf-8", "replace"))

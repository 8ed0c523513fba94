"""ctypes binding of libvoxelhip.so (include/voxel_hip.h) shaped like the reference's `graphics::Svo`
(src/graphics/svo.rs:56-256): new / update / render / raycast / get_stats.

This is harness code. It adds nothing to the path: every method is one or two C-ABI calls, and every failure
of the native library raises -- there is no fallback of any kind.
"""
import ctypes as C
import math

import numpy as np

from .build import lib_path, share_hip_runtime_with_torch

VX_OK = 0
VX_MEM_HOST, VX_MEM_DEVICE = 0, 1
VX_FORMAT_RGBA32F, VX_FORMAT_RGBA8 = 0, 1
VX_COMM_ID_BYTES = 128
TILE = 32

MATERIAL_DTYPE = np.dtype([("specular_pow", "<f4"), ("specular_strength", "<f4"), ("tex_top", "<i4"), ("tex_side", "<i4"), ("tex_bottom", "<i4"),
                           ("tex_top_normal", "<i4"), ("tex_side_normal", "<i4"), ("tex_bottom_normal", "<i4")])
HIT_DTYPE = np.dtype([("t", "<f4"), ("value", "<u4"), ("face_id", "<i4"), ("flags", "<u4"), ("pos", "<f4", 3), ("lod", "<f4"), ("uv", "<f4", 2),
                      ("shadow_t", "<f4"), ("steps", "<u4")])
PICKER_TASK_DTYPE = np.dtype([("max_dst", "<f4"), ("_p0", "<f4", 3), ("pos", "<f4", 3), ("_p1", "<f4"), ("dir", "<f4", 3), ("_p2", "<f4")])
PICKER_RESULT_DTYPE = np.dtype([("dst", "<f4"), ("inside_voxel", "<u4"), ("_p0", "<f4", 2), ("pos", "<f4", 3), ("_p1", "<f4"), ("normal", "<f4", 3),
                                ("_p2", "<f4")])
FRAME_DTYPE = np.dtype([("t_min", "<f4"), ("ptr", "<u4"), ("idx", "<u4"), ("parent_octant_idx", "<u4"), ("scale", "<i4"), ("is_child", "<i4"),
                        ("is_leaf", "<i4"), ("crossed_boundary", "<i4"), ("next_ptr", "<u4")])
# vx_entity / vx_aabb_result (src/systems/physics.rs:10-75, src/graphics/svo_picker.rs:163-176)
ENTITY_DTYPE = np.dtype([("position", "<f4", 3), ("velocity", "<f4", 3), ("aabb_offset", "<f4", 3), ("aabb_extents", "<f4", 3), ("gravity", "<f4"),
                         ("max_fall_velocity", "<f4"), ("flags", "<u4"), ("grounded", "<u4")])
AABB_RESULT_DTYPE = np.dtype([("neg", "<f4", 3), ("pos", "<f4", 3)])
ENTITY_WALL_CLIP, ENTITY_FLYING = 1, 2
# vx_ray_hit (vx_raycast_batch): a PickerResult that keeps the block id and names the normal by its face
RAY_HIT_DTYPE = np.dtype([("dst", "<f4"), ("value", "<u4"), ("face_id", "<i4"), ("inside_voxel", "<u4"), ("pos", "<f4", 3), ("_pad", "<u4")])
VX_RAYS_TRANSLUCENT = 1
# vx_block_cell (vx_block_points): the leaf, or the empty cell, that holds a point
BLOCK_CELL_DTYPE = np.dtype([("value", "<u4"), ("cell_log2", "<u4")])
VX_CELL_OUTSIDE = 0xFFFFFFFF
# vx_block_at (vx_list_region): one block of a box -- `where`: the voxel's index in read_region's dense array (bits 0..23) and its open faces (bits
# 24..29, numbered like face_id); split_where takes it apart
BLOCK_AT_DTYPE = np.dtype([("where", "<u4"), ("value", "<u4")])
VX_LIST_FACES, VX_LIST_EXPOSED = 1, 2
# vx_scan_hit (vx_scan_points, vx_scan_columns): the first voxel holding a block along an axis; directions numbered like face_id
SCAN_HIT_DTYPE = np.dtype([("coord", "<i4"), ("value", "<u4"), ("cell_log2", "<u4"), ("_pad", "<u4")])
# vx_box_hit (vx_overlap_boxes): what a float box holds -- the voxels of its cover that hold a (counted) block, the first of them in
# read_region's order, their bounds [lo, hi); blocks == VX_BOX_INVALID: the record described no box
BOX_HIT_DTYPE = np.dtype([("blocks", "<u4"), ("value", "<u4"), ("lo", "<i4", 3), ("hi", "<i4", 3)])
VX_BOX_INVALID = 0xFFFFFFFF
# vx_move_hit (vx_move_boxes): how far a box got -- its origin after the move, what was added to it per axis, the sides on which a block lay
# ahead (bit 2a + (d_a > 0), numbered like face_id; VX_MOVE_INVALID: no box, or no motion), per axis the stopping voxel's value
MOVE_HIT_DTYPE = np.dtype([("origin", "<f4", 3), ("moved", "<f4", 3), ("contacts", "<u4"), ("value", "<u4", 3), ("_pad", "<u4", 2)])
VX_MOVE_INVALID, VX_MOVE_MAX_TRAVEL = 0xFFFFFFFF, 64.0
VX_MOVE_ORDER_YXZ, VX_MOVE_ORDER_XYZ, VX_MOVE_ORDER_ZYX = 0x21, 0x24, 0x06  # axis of pass 0 | pass 1 << 2 | pass 2 << 4
# vx_flood_info (vx_flood_points): what a flood reached -- cells with a step count (VX_FLOOD_INVALID: no position), the largest step count,
# the faces of the box a reached cell lies on (0: enclosed), the value at the seed. A field is one byte a cell: the step count, or one of
# VX_FLOOD_NO_POSITION, VX_FLOOD_UNREACHED, VX_FLOOD_BLOCKED
FLOOD_INFO_DTYPE = np.dtype([("reached", "<u4"), ("farthest", "<u4"), ("faces", "<u4"), ("seed_value", "<u4")])
VX_FLOOD_MAX_STEPS, VX_FLOOD_NO_POSITION, VX_FLOOD_UNREACHED, VX_FLOOD_BLOCKED = 250, 0xFD, 0xFE, 0xFF
VX_FLOOD_SEED_ALWAYS, VX_FLOOD_INVALID = 1, 0xFFFFFFFF
# vx_light_info (vx_light_boxes): what the light of a box amounts to -- the cells whose byte is not 0, the cells that emit, the columns whose top
# cell is exposed to the sky, the faces of the box on which a cell has a level of 2 or more. A field is one byte a cell: sky << 4 | block
LIGHT_INFO_DTYPE = np.dtype([("lit", "<u4"), ("sources", "<u4"), ("open_columns", "<u4"), ("faces", "<u4")])
VX_LIGHT_MAX_SIDE, VX_LIGHT_MAX_PROPS, VX_LIGHT_TRANSPARENT, VX_LIGHT_NO_SKY, VX_LIGHT_NO_BLOCKS, VX_LIGHT_INVALID = 48, 4096, 0x10, 1, 2, 0xFFFFFFFF
# vx_walk_info (vx_walk_points): what a walk reached -- reached, farthest, faces and seed_value as FLOOD_INFO_DTYPE's over standable cells, the y inside
# the box on which the seed and the goal came to stand, and the goal's step count (VX_WALK_NONE: none). A field is one byte a cell: the step
# count, or one of VX_WALK_NO_POSITION, VX_WALK_UNREACHED, VX_WALK_NO_STAND; a path entry is rx | ry << 8 | rz << 16, or VX_WALK_NONE
WALK_INFO_DTYPE = np.dtype([("reached", "<u4"), ("farthest", "<u4"), ("faces", "<u4"), ("seed_value", "<u4"), ("start_ry", "<u4"), ("goal_ry", "<u4"),
                            ("path_steps", "<u4"), ("_pad", "<u4")])
VX_WALK_MAX_STEPS, VX_WALK_NO_POSITION, VX_WALK_UNREACHED, VX_WALK_NO_STAND = 250, 0xFD, 0xFE, 0xFF
VX_WALK_STOP_AT_GOAL, VX_WALK_NONE = 1, 0xFFFFFFFF
# vx_label_piece and vx_label_info (vx_label_boxes): a loose piece -- its cells, its bounds inside the box (rx | ry << 8 | rz << 16, inclusive), its
# first cell | faces << 24 -- and what the solid cells of a box fall into: solid == held + loose + more. A field is one byte a cell:
# VX_LABEL_AIR, the piece's label 1..pieces, VX_LABEL_MORE or VX_LABEL_HELD
LABEL_PIECE_DTYPE = np.dtype([("cells", "<u4"), ("lo", "<u4"), ("hi", "<u4"), ("where", "<u4")])
LABEL_INFO_DTYPE = np.dtype([("solid", "<u4"), ("held", "<u4"), ("pieces", "<u4"), ("loose", "<u4"), ("more", "<u4"), ("steps", "<u4"), ("faces", "<u4"),
                             ("flags", "<u4")])
VX_LABEL_MAX_PIECES, VX_LABEL_MAX_STEPS, VX_LABEL_AIR, VX_LABEL_MORE, VX_LABEL_HELD, VX_LABEL_ALL_FACES, VX_LABEL_CUT = 250, 4096, 0x00, 0xFE, 0xFF, 0x3F, 1
# vx_distance_info (vx_distance_boxes): what the distances of a box amount to -- the target cells, the largest value of the field, the first cell in
# the field's order that holds it (rx | ry << 8 | rz << 16), the faces of the box a target lies on. A field is one uint16 a cell: the squared
# distance to the nearest target cell of the box, or VX_DISTANCE_NONE
DISTANCE_INFO_DTYPE = np.dtype([("targets", "<u4"), ("farthest", "<u4"), ("where", "<u4"), ("faces", "<u4")])
VX_DISTANCE_NONE, VX_DISTANCE_TO_AIR = 0xFFFF, 1
VX_DIR_NEG_X, VX_DIR_POS_X, VX_DIR_NEG_Y, VX_DIR_POS_Y, VX_DIR_NEG_Z, VX_DIR_POS_Z = range(6)
VX_SCAN_NONE = -0x80000000
VX_SCAN_TO_EDGE = 0xFFFFFFFF
FACE_NORMALS = np.array([[-1, 0, 0], [1, 0, 0], [0, -1, 0], [0, 1, 0], [0, 0, -1], [0, 0, 1]], dtype=np.float32)  # by face_id
assert HIT_DTYPE.itemsize == 48 and PICKER_TASK_DTYPE.itemsize == 48 and PICKER_RESULT_DTYPE.itemsize == 48 and FRAME_DTYPE.itemsize == 36
assert ENTITY_DTYPE.itemsize == 64 and AABB_RESULT_DTYPE.itemsize == 24 and RAY_HIT_DTYPE.itemsize == 32 and SCAN_HIT_DTYPE.itemsize == 16
assert BLOCK_AT_DTYPE.itemsize == 8 and BOX_HIT_DTYPE.itemsize == 32 and FLOOD_INFO_DTYPE.itemsize == 16 and LIGHT_INFO_DTYPE.itemsize == 16
assert WALK_INFO_DTYPE.itemsize == 32 and MOVE_HIT_DTYPE.itemsize == 48 and LABEL_PIECE_DTYPE.itemsize == 16 and LABEL_INFO_DTYPE.itemsize == 32
assert DISTANCE_INFO_DTYPE.itemsize == 16

COUNTER_FIELDS = ["rays", "iterations", "pushes", "leaf_tests", "leaf_tests_trilinear", "boundaries", "csvo_header_bytes", "csvo_pointer_bytes",
                  "pixels", "lit_pixels", "shadow_rays", "wave_steps", "services", "refills", "tail_wave_steps", "tail_iterations"]


class Uniforms(C.Structure):
    _fields_ = [("view", C.c_float * 16), ("fovy", C.c_float), ("aspect", C.c_float), ("ambient", C.c_float), ("light_dir", C.c_float * 3),
                ("cam_pos", C.c_float * 3), ("render_shadows", C.c_int32), ("shadow_distance", C.c_float), ("highlight_pos", C.c_float * 3)]


class Range(C.Structure):
    _fields_ = [("start", C.c_uint64), ("length", C.c_uint64)]


class Target(C.Structure):
    _fields_ = [("rgba32f", C.c_void_p), ("hits", C.c_void_p), ("memory", C.c_int32), ("tile_rank", C.c_uint32), ("tile_count", C.c_uint32),
                ("format", C.c_int32)]


class RayBatch(C.Structure):
    """vx_ray_batch"""
    _fields_ = [("origin", C.c_void_p), ("dir", C.c_void_p), ("max_dst", C.c_void_p), ("origin_stride", C.c_uint32), ("dir_stride", C.c_uint32),
                ("max_dst_stride", C.c_uint32), ("max_dst_all", C.c_float), ("flags", C.c_uint32)]


class BoxBatch(C.Structure):
    """vx_box_batch"""
    _fields_ = [("origin", C.c_void_p), ("offset", C.c_void_p), ("extents", C.c_void_p), ("origin_stride", C.c_uint32), ("offset_stride", C.c_uint32),
                ("extents_stride", C.c_uint32), ("only_value", C.c_uint32)]


class MoveShape(C.Structure):
    """vx_move_shape"""
    _fields_ = [("scale", C.c_float), ("skin", C.c_float), ("order", C.c_uint32), ("flags", C.c_uint32)]


class FloodShape(C.Structure):
    """vx_flood_shape"""
    _fields_ = [("size", C.c_uint32 * 3), ("seed_at", C.c_uint32 * 3), ("max_steps", C.c_uint32), ("pass_value", C.c_uint32), ("flags", C.c_uint32)]


class WalkShape(C.Structure):
    """vx_walk_shape"""
    _fields_ = [("size", C.c_uint32 * 3), ("seed_at", C.c_uint32 * 3), ("max_steps", C.c_uint32), ("pass_value", C.c_uint32), ("height", C.c_uint32),
                ("climb", C.c_uint32), ("drop", C.c_uint32), ("path_capacity", C.c_uint32), ("flags", C.c_uint32)]


class LightShape(C.Structure):
    """vx_light_shape"""
    _fields_ = [("size", C.c_uint32 * 3), ("flags", C.c_uint32), ("props", C.c_void_p), ("props_count", C.c_uint32)]


class LabelShape(C.Structure):
    """vx_label_shape"""
    _fields_ = [("size", C.c_uint32 * 3), ("anchor_faces", C.c_uint32), ("max_pieces", C.c_uint32), ("max_steps", C.c_uint32), ("pass_value", C.c_uint32),
                ("flags", C.c_uint32)]


class DistanceShape(C.Structure):
    """vx_distance_shape"""
    _fields_ = [("size", C.c_uint32 * 3), ("pass_value", C.c_uint32), ("match_value", C.c_uint32), ("flags", C.c_uint32), ("_pad", C.c_uint32 * 2)]


class Result(C.Structure):
    _fields_ = [("t", C.c_float), ("value", C.c_uint32), ("face_id", C.c_int32), ("pos", C.c_float * 3), ("uv", C.c_float * 2),
                ("color", C.c_float * 4), ("lod", C.c_float), ("inside_voxel", C.c_int32)]


class Stats(C.Structure):
    _fields_ = [("used_bytes", C.c_uint64), ("capacity_bytes", C.c_uint64), ("depth", C.c_uint32)]


class Counters(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in COUNTER_FIELDS]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n in COUNTER_FIELDS}


# every symbol include/voxel_hip.h declares: (restype, argtypes)
_vp, _u32, _u64, _sz, _int = C.c_void_p, C.c_uint32, C.c_uint64, C.c_size_t, C.c_int
SYMBOLS = {
    "vx_create": (_int, [_int, _sz, _int, C.POINTER(_vp)]),
    "vx_destroy": (None, [_vp]),
    "vx_set_materials": (_int, [_vp, _vp, _u32]),
    "vx_set_textures": (_int, [_vp, _vp, _u32, _u32, _u32, _u32]),
    "vx_staging_ptr": (_vp, [_vp]),
    "vx_capacity": (_sz, [_vp]),
    "vx_commit": (_int, [_vp, _u32, _vp, _u32, _u64]),
    "vx_commit_all": (_int, [_vp, _u32, _u64]),
    "vx_set_commit_mode": (_int, [_vp, _int]),
    "vx_commit_wait": (_int, [_vp]),
    "vx_get_stats": (_int, [_vp, C.POINTER(Stats)]),
    "vx_render": (_int, [_vp, C.POINTER(Uniforms), _u32, _u32, C.POINTER(Target)]),
    "vx_raycast": (_int, [_vp, _vp, _u32, _vp]),
    "vx_raycast_batch": (_int, [_vp, C.POINTER(RayBatch), _u32, _int, _vp]),
    "vx_trace_rays": (_int, [_vp, C.POINTER(Uniforms), C.POINTER(RayBatch), _u32, _int, _vp, _int, _vp]),
    "vx_trace_views": (_int, [_vp, C.POINTER(Uniforms), _u32, _u32, _u32, _int, _vp, _int, _vp]),
    "vx_block_points": (_int, [_vp, _vp, _u32, _u32, _int, _vp]),
    "vx_read_region": (_int, [_vp, C.POINTER(C.c_int32 * 3), C.POINTER(_u32 * 3), _int, _vp]),
    "vx_list_region": (_int, [_vp, C.POINTER(C.c_int32 * 3), C.POINTER(_u32 * 3), _u32, _int, _vp, _u32, _vp]),
    "vx_scan_points": (_int, [_vp, _vp, _u32, _u32, _int, _u32, _int, _vp]),
    "vx_scan_columns": (_int, [_vp, C.POINTER(C.c_int32 * 3), C.POINTER(_u32 * 3), _int, _int, _vp]),
    "vx_overlap_boxes": (_int, [_vp, C.POINTER(BoxBatch), _u32, _int, _vp]),
    "vx_move_boxes": (_int, [_vp, C.POINTER(BoxBatch), _vp, _u32, _u32, C.POINTER(MoveShape), _int, _vp]),
    "vx_flood_points": (_int, [_vp, _vp, _u32, _u32, C.POINTER(FloodShape), _int, _vp, _u32, _vp]),
    "vx_light_boxes": (_int, [_vp, _vp, _u32, _u32, C.POINTER(LightShape), _int, _vp, _u32, _vp]),
    "vx_walk_points": (_int, [_vp, _vp, _u32, _vp, _u32, _u32, C.POINTER(WalkShape), _int, _vp, _u32, _vp, _vp]),
    "vx_label_boxes": (_int, [_vp, _vp, _u32, _u32, C.POINTER(LabelShape), _int, _vp, _u32, _vp, _vp]),
    "vx_distance_boxes": (_int, [_vp, _vp, _u32, _u32, C.POINTER(DistanceShape), _int, _vp, _u32, _vp]),
    "vx_physics_step": (_int, [_vp, _vp, _u32, _int, C.c_float, _u32, _vp]),
    "vx_debug_trace": (_int, [_vp, C.POINTER(C.c_float * 3), C.POINTER(C.c_float * 3), C.c_float, _int, C.POINTER(Result), _vp, _u32, C.POINTER(_u32)]),
    "vx_sync": (_int, [_vp]),
    "vx_set_frames_in_flight": (_int, [_vp, _int]),
    "vx_wait_event": (_int, [_vp, _vp]),
    "vx_stream_wait_render": (_int, [_vp, _vp]),
    "vx_traversal_image": (_u64, [_int, _vp, _u64, _int, _vp, _u64]),
    "vx_traversal_image_with_origin": (_u64, [_int, _vp, _u64, _int, _vp, _u64, _vp, _u64]),
    "vx_arena_capacity": (_sz, [_vp]),
    "vx_resolve_2x2": (_int, [_vp, _vp, _u32, _u32, _vp, _vp]),
    "vx_assemble_tiles": (_int, [_vp, _vp, _u64, _u32, _u32, _u32, _vp]),
    "vx_assemble_tiles_on": (_int, [_vp, _vp, _u64, _u32, _u32, _u32, _vp, _vp]),
    "vx_assemble_tiles_format": (_int, [_vp, _vp, _u64, _u32, _u32, _u32, _vp, _int, _vp]),
    "vx_tile_order": (_u32, [_u32, _u32, _vp, _u32]),
    "vx_present_begin": (_int, [_vp, C.POINTER(Uniforms), _u32, _u32, _int, C.POINTER(_int)]),
    "vx_present_wait": (_int, [_vp, _int, C.POINTER(_vp), C.POINTER(_sz)]),
    "vx_comm_library": (_int, [C.c_char_p]),
    "vx_comm_unique_id": (_int, [_vp, _sz]),
    "vx_comm_init": (_int, [_vp, _int, _int, _vp]),
    "vx_comm_destroy": (_int, [_vp]),
    "vx_comm_info": (_int, [_vp, C.POINTER(_int), C.POINTER(_int)]),
    "vx_set_comm_headroom": (_int, [_vp, _int]),
    "vx_gather_tiles": (_int, [_vp, _vp, _u64, _vp, _int, C.POINTER(_int)]),
    "vx_wait_gather": (_int, [_vp, _int]),
    "vx_render_gather": (_int, [_vp, C.POINTER(Uniforms), _u32, _u32, C.POINTER(Target), _u64, _vp, _int, _vp, _int, C.POINTER(_int)]),
    "vx_comm_stream": (_vp, [_vp]),
    "vx_local_tile_count": (_u32, [_u32, _u32, _u32, _u32]),
    "vx_render_counters": (_int, [_vp, C.POINTER(Uniforms), _u32, _u32, _u32, _u32, C.POINTER(Counters)]),
    "vx_excursion_counters": (_int, [_vp, C.POINTER(_u64 * 4), _int]),
    "vx_image_info": (_int, [_vp, C.POINTER(_u64 * 4)]),
    "vx_debug_knobs": (_int, [_vp, C.POINTER(_u32 * 8)]),
    "vx_timeline_read": (_u32, [_vp, _vp, _u32]),
    "vx_gather_query": (_int, [_vp, _int]),
    "vx_comm_profile_read": (_int, [_vp, C.POINTER(C.c_double), C.POINTER(_u32)]),
    "vx_clock_probe": (_int, [_vp, _u32, C.POINTER(C.c_double)]),
    "vx_profile_enable": (_int, [_vp, _int]),
    "vx_profile_read": (_int, [_vp, C.POINTER(C.c_double), C.POINTER(_u32)]),
    "vx_stream": (_vp, [_vp]),
    "vx_device": (_int, [_vp]),
    "vx_last_error": (C.c_char_p, []),
    "vx_version": (C.c_char_p, []),
}

_lib = None


class VoxelHipError(RuntimeError):
    pass


def lib():
    """Loads libvoxelhip.so; raises if it (or any declared symbol) is missing -- never falls back."""
    global _lib
    if _lib is None:
        share_hip_runtime_with_torch()
        L = C.CDLL(str(lib_path("libvoxelhip.so")))
        for name, (res, args) in SYMBOLS.items():
            fn = getattr(L, name)  # AttributeError if the library does not export it
            fn.restype, fn.argtypes = res, args
        _lib = L
    return _lib


def _check(rc):
    if rc != VX_OK:
        raise VoxelHipError(f"libvoxelhip error {rc}: {lib().vx_last_error().decode()}")


def make_uniforms(view, fovy, aspect, ambient, light_dir, cam_pos, render_shadows, shadow_distance, highlight_pos=None):
    u = Uniforms()
    u.view = (C.c_float * 16)(*[float(x) for x in view])
    u.fovy, u.aspect, u.ambient = float(fovy), float(aspect), float(ambient)
    u.light_dir = (C.c_float * 3)(*[float(x) for x in light_dir])
    u.cam_pos = (C.c_float * 3)(*[float(x) for x in cam_pos])
    u.render_shadows = int(render_shadows)
    u.shadow_distance = float(shadow_distance)
    hp = highlight_pos if highlight_pos is not None else (math.nan,) * 3  # NaN when nothing is selected (svo.rs:211)
    u.highlight_pos = (C.c_float * 3)(*[float(x) for x in hp])
    return u


def local_tile_count(width, height, rank, count):
    return lib().vx_local_tile_count(width, height, rank, count)


def tile_order(width, height):
    """vx_tile_order: row-major tile ids in the Morton order the ranks share out."""
    n = lib().vx_tile_order(width, height, None, 0)
    out = np.zeros(n, dtype=np.uint32)
    lib().vx_tile_order(width, height, out.ctypes.data_as(_vp), n)
    return out


def comm_library(path):
    """The RCCL build to open instead of librccl.so.1 (vx_comm_library); before the first communicator."""
    _check(lib().vx_comm_library(str(path).encode()))


def comm_unique_id():
    """A fresh RCCL unique id (bytes) for vx_comm_init; made on ONE rank and handed to the others by the caller."""
    buf = C.create_string_buffer(VX_COMM_ID_BYTES)
    _check(lib().vx_comm_unique_id(buf, VX_COMM_ID_BYTES))
    return buf.raw


def traversal_image(svo_type, world_frame_words, used_bytes, layout=0, with_origin=False):
    """vx_traversal_image: world frame (uint32 words: scale, header, arena...) -> traversal image (uint32 words);
    layout 0 = ESVO frame (walkable by any ESVO traversal), 1 = what the renderer walks -- octants of one {pointer | value, masks} entry per existing
    child, addressed in 8-byte units, through a buffer resource --, 2 = the same bytes walked through a 64-bit pointer (images beyond 4 GiB).
    with_origin: (image, image) -- since round 6 the origin of a CSVO world's voxel-parent octant is a unit of the image itself, in front of the octant's
    values; what used to be a table of its own IS the image (a walk reads unit `lo` of it)."""
    f = np.ascontiguousarray(world_frame_words, dtype=np.uint32)
    n = lib().vx_traversal_image(svo_type, f.ctypes.data_as(_vp), used_bytes, layout, None, 0)
    if n == 0:
        raise ValueError("this world frame cannot be imaged")
    out = np.zeros(n, dtype=np.uint32)
    lib().vx_traversal_image(svo_type, f.ctypes.data_as(_vp), used_bytes, layout, out.ctypes.data_as(_vp), n)
    return (out, out) if with_origin else out


def entities_from_rows(rows):
    """host.py's entity rows (17 floats: position, velocity, aabb offset, aabb extents, wall_clip, flying, gravity, max_fall_velocity,
    is_grounded) as vx_entity records."""
    r = np.asarray(rows, dtype=np.float32).reshape(-1, 17)
    e = np.zeros(len(r), dtype=ENTITY_DTYPE)
    e["position"], e["velocity"], e["aabb_offset"], e["aabb_extents"] = r[:, 0:3], r[:, 3:6], r[:, 6:9], r[:, 9:12]
    e["gravity"], e["max_fall_velocity"] = r[:, 14], r[:, 15]
    e["flags"] = np.where(r[:, 12] != 0, ENTITY_WALL_CLIP, 0) | np.where(r[:, 13] != 0, ENTITY_FLYING, 0)
    e["grounded"] = r[:, 16] != 0
    return e


def entities_to_rows(entities):
    """vx_entity records as host.py's entity rows."""
    e = np.asarray(entities, dtype=ENTITY_DTYPE).reshape(-1)
    r = np.zeros((len(e), 17), dtype=np.float32)
    r[:, 0:3], r[:, 3:6], r[:, 6:9], r[:, 9:12] = e["position"], e["velocity"], e["aabb_offset"], e["aabb_extents"]
    r[:, 12] = (e["flags"] & ENTITY_WALL_CLIP) != 0
    r[:, 13] = (e["flags"] & ENTITY_FLYING) != 0
    r[:, 14], r[:, 15] = e["gravity"], e["max_fall_velocity"]
    r[:, 16] = e["grounded"] != 0
    return r


def entity_positions(entities):
    """The positions inside vx_entity records as the origins of a ray batch (Svo.raycast_batch): an (N, 3) float32 view at a stride of 64
    bytes -- of a NumPy array of ENTITY_DTYPE, or of a contiguous torch tensor whose bytes are vx_entity records. No copy."""
    return _record_vectors("entity_positions", "vx_entity", entities, ENTITY_DTYPE, "position")[0]


def entity_boxes(entities):
    """The boxes inside vx_entity records as the arguments of Svo.overlap_boxes: (origin, extents, offset) -- position, aabb_extents and
    aabb_offset as (N, 3) float32 views at a stride of 64 bytes, of a NumPy array of ENTITY_DTYPE or of a contiguous torch tensor whose
    bytes are vx_entity records. No copy: svo.overlap_boxes(*entity_boxes(e)) reads the records in place."""
    return _record_vectors("entity_boxes", "vx_entity", entities, ENTITY_DTYPE, "position", "aabb_extents", "aabb_offset")


def box_hits_to_numpy(hits):
    """A device record tensor of Svo.overlap_boxes as BOX_HIT_DTYPE records (copies to the host: synchronise first)."""
    return _to_numpy(hits, BOX_HIT_DTYPE)


def move_hits_to_numpy(hits):
    """A device record tensor of Svo.move_boxes as MOVE_HIT_DTYPE records (copies to the host: synchronise first)."""
    return _to_numpy(hits, MOVE_HIT_DTYPE)


def MOVE_SHAPE(scale=1.0, skin=2.0 ** -10, order=VX_MOVE_ORDER_YXZ, flags=0):
    """A vx_move_shape."""
    return MoveShape(float(scale), float(skin), int(order), int(flags))


def entity_velocities(entities):
    """vx_entity.velocity as the `motion` of Svo.move_boxes: an (N, 3) float32 view at a stride of 64 bytes, of what entity_boxes takes."""
    return _record_vectors("entity_velocities", "vx_entity", entities, ENTITY_DTYPE, "velocity")[0]


def flood_infos_to_numpy(infos):
    """A device record tensor of Svo.flood_points as FLOOD_INFO_DTYPE records (copies to the host: synchronise first)."""
    return _to_numpy(infos, FLOOD_INFO_DTYPE)


def flood_shape(size, seed_at=None, max_steps=VX_FLOOD_MAX_STEPS, pass_value=0, flags=0):
    """A vx_flood_shape; seed_at None: the box's centre cell, size // 2."""
    size = [int(v) for v in size]
    seed_at = [v // 2 for v in size] if seed_at is None else [int(v) for v in seed_at]
    return FloodShape((C.c_uint32 * 3)(*size), (C.c_uint32 * 3)(*seed_at), int(max_steps), int(pass_value), int(flags))


def walk_infos_to_numpy(infos):
    """A device record tensor of Svo.walk_points as WALK_INFO_DTYPE records (copies to the host: synchronise first)."""
    return _to_numpy(infos, WALK_INFO_DTYPE)


def walk_shape(size, seed_at=None, max_steps=VX_WALK_MAX_STEPS, pass_value=0, height=2, climb=1, drop=3, path_capacity=0, flags=0):
    """A vx_walk_shape; seed_at None: the box's centre cell, size // 2."""
    size = [int(v) for v in size]
    seed_at = [v // 2 for v in size] if seed_at is None else [int(v) for v in seed_at]
    return WalkShape((C.c_uint32 * 3)(*size), (C.c_uint32 * 3)(*seed_at), int(max_steps), int(pass_value), int(height), int(climb), int(drop), int(path_capacity), int(flags))


def light_infos_to_numpy(infos):
    """A device record tensor of Svo.light_boxes as LIGHT_INFO_DTYPE records (copies to the host: synchronise first)."""
    return _to_numpy(infos, LIGHT_INFO_DTYPE)


def label_pieces_to_numpy(pieces):
    """A device piece tensor of Svo.label_boxes as LABEL_PIECE_DTYPE records [N, max_pieces] (copies to the host: synchronise first)."""
    return _to_numpy(pieces, LABEL_PIECE_DTYPE).reshape(pieces.shape[0], -1)


def label_infos_to_numpy(infos):
    """A device record tensor of Svo.label_boxes as LABEL_INFO_DTYPE records (copies to the host: synchronise first)."""
    return _to_numpy(infos, LABEL_INFO_DTYPE)


def label_shape(size, anchor_faces=VX_LABEL_ALL_FACES, max_pieces=VX_LABEL_MAX_PIECES, max_steps=VX_LABEL_MAX_STEPS, pass_value=0, flags=0):
    """A vx_label_shape."""
    return LabelShape((C.c_uint32 * 3)(*size), int(anchor_faces), int(max_pieces), int(max_steps), int(pass_value), int(flags))


def distance_infos_to_numpy(infos):
    """A device record tensor of Svo.distance_boxes as DISTANCE_INFO_DTYPE records (copies to the host: synchronise first)."""
    return _to_numpy(infos, DISTANCE_INFO_DTYPE)


def distance_fields_to_numpy(fields):
    """A device field tensor of Svo.distance_boxes (int16 [N, field_stride / 2]) as a uint16 array of its shape, in which VX_DISTANCE_NONE reads as
    itself and not as -1 (copies to the host: synchronise first)."""
    return fields.cpu().numpy().view(np.uint16)


def distance_shape(size, pass_value=0, match_value=0, flags=0):
    """A vx_distance_shape."""
    return DistanceShape((C.c_uint32 * 3)(*(int(v) for v in size)), int(pass_value), int(match_value), int(flags))


def light_shape(size, props, flags=0):
    """(a vx_light_shape, the array its props pointer points into: keep it until the call has returned). props: uint8, at most 4,096 of them."""
    table = np.ascontiguousarray(np.asarray(props, dtype=np.uint8).reshape(-1))
    size = [int(v) for v in size]
    return LightShape((C.c_uint32 * 3)(*size), int(flags), table.ctypes.data if len(table) else None, len(table)), table


def ray_hits_to_numpy(hits):
    """A device hit tensor of Svo.raycast_batch as RAY_HIT_DTYPE records (copies to the host: synchronise first)."""
    return _to_numpy(hits, RAY_HIT_DTYPE)


def trace_hits_to_numpy(hits):
    """A device record tensor of Svo.trace_rays as HIT_DTYPE records (copies to the host: synchronise first)."""
    return _to_numpy(hits, HIT_DTYPE)


def ray_hit_positions(hits):
    """The positions inside vx_ray_hit records as the points of Svo.block_points: an (N, 3) float32 view at a stride of 32 bytes -- of a
    NumPy array of RAY_HIT_DTYPE, or of a device hit tensor of Svo.raycast_batch. No copy."""
    return _record_vectors("ray_hit_positions", "vx_ray_hit", hits, RAY_HIT_DTYPE, "pos")[0]


def block_cells_to_numpy(cells):
    """A device record tensor of Svo.block_points as BLOCK_CELL_DTYPE records (copies to the host: synchronise first)."""
    return _to_numpy(cells, BLOCK_CELL_DTYPE)


def block_ats_to_numpy(records):
    """A device record tensor of Svo.list_region as BLOCK_AT_DTYPE records (copies to the host: synchronise first)."""
    return _to_numpy(records, BLOCK_AT_DTYPE)


def split_where(where):
    """(index, faces) of vx_block_at.where values (VX_AT_INDEX, VX_AT_FACES): the voxel's index in read_region's dense array of the same box,
    and its open faces, bit f numbered like face_id. NumPy arrays, torch tensors and plain ints alike."""
    return where & 0xFFFFFF, (where >> 24) & 0x3F


def scan_hits_to_numpy(hits):
    """A device record tensor of Svo.scan_points or Svo.scan_columns as SCAN_HIT_DTYPE records, in the tensor's shape without its last axis
    (copies to the host: synchronise first)."""
    return _to_numpy(hits, SCAN_HIT_DTYPE).reshape(tuple(hits.shape[:-1]))


# ---- what the batch and block methods of Svo share: every one of them is its docstring, these, one call of the library and a return ----------
_U8, _U16, _U32 = np.dtype(np.uint8), np.dtype(np.uint16), np.dtype(np.uint32)
_DTYPE_NAMES = {v: k for k, v in list(globals().items()) if isinstance(v, np.dtype) and k.endswith("_DTYPE")}


def _to_numpy(records, dtype):
    """A device tensor's bytes as records of `dtype`, flat (copies to the host)."""
    return records.cpu().numpy().view(np.uint8).reshape(-1).view(dtype)


def _record_vectors(caller, c_name, records, dtype, *fields):
    """The (N, 3) float32 vectors that the named fields of `dtype` records are, as views at the records' stride: of a NumPy array of `dtype`, or
    of a contiguous torch tensor whose bytes are such records. No copy."""
    if isinstance(records, np.ndarray):
        if records.dtype != dtype:
            raise TypeError(f"{caller}: a host array must be of hip.{_DTYPE_NAMES[dtype]}")
        flat = records.reshape(-1)
        return tuple(flat[f] for f in fields)
    import torch

    nbytes = records.numel() * records.element_size()
    if nbytes % dtype.itemsize or not records.is_contiguous():
        raise TypeError(f"{caller}: a device tensor must be contiguous and hold whole {dtype.itemsize}-byte {c_name} records")
    rows = records.reshape(-1).view(torch.uint8).view(torch.float32).view(nbytes // dtype.itemsize, dtype.itemsize // 4)
    return tuple(rows[:, dtype.fields[f][1] // 4:dtype.fields[f][1] // 4 + 3] for f in fields)


def _ray_vectors(name, x, count, width, method="raycast_batch"):
    """(address, stride in bytes) of float32 vectors of `width` adjacent floats in a NumPy array or a torch tensor: `count` of them at the
    array's own row stride (shape (count, width); (count,) for width 1), or -- width 3 -- a single one (shape (3,)) with stride 0.
    method: the caller a refusal names."""
    is_np = isinstance(x, np.ndarray)
    if str(x.dtype) not in ("float32", "torch.float32"):
        raise TypeError(f"{method}: {name} must be float32")
    shape = tuple(x.shape)
    strides = tuple(x.strides) if is_np else tuple(4 * st for st in x.stride())
    ptr = x.ctypes.data if is_np else x.data_ptr()
    if width > 1 and shape[-1:] == (width,) and strides[-1] != 4:
        raise TypeError(f"{method}: the components of {name} must be adjacent floats")
    if width > 1 and shape == (width,):
        return ptr, 0
    if shape != ((count, width) if width > 1 else (count,)):
        raise TypeError(f"{method}: {name} has shape {shape} for {count} rays")
    if count <= 1:
        return ptr, 4 * width  # (nobody steps by it)
    if strides[0] < 0:
        raise TypeError(f"{method}: {name} has a negative stride")
    return ptr, strides[0]


def _points(method, name, x):
    """(memory kind, count, address, stride in bytes) of an (N, 3) float32 batch at any row stride, a NumPy array or a torch CUDA tensor."""
    host = isinstance(x, np.ndarray)
    if len(x.shape) != 2 or x.shape[1] != 3:
        raise TypeError(f"{method}: {name} must have shape (N, 3)")
    if not host and not getattr(x, "is_cuda", False):
        raise TypeError(f"{method}: {name} must be a NumPy array or a torch CUDA tensor")
    count = int(x.shape[0])
    ptr, stride = _ray_vectors(name, x, count, 3, method)
    return VX_MEM_HOST if host else VX_MEM_DEVICE, count, _vp(ptr), stride


def _lo_rows(method, lo):
    """(memory kind, count, address, stride in bytes) of the int32 (N, 3) corners of light_boxes and label_boxes."""
    host = isinstance(lo, np.ndarray)
    if len(lo.shape) != 2 or lo.shape[1] != 3:
        raise TypeError(f"{method}: lo must have shape (N, 3)")
    if not host and not getattr(lo, "is_cuda", False):
        raise TypeError(f"{method}: lo must be a NumPy array or a torch CUDA tensor")
    count = int(lo.shape[0])
    if host:
        if lo.dtype != np.int32 or (count and (lo.strides[1] != 4 or lo.strides[0] % 4 or lo.strides[0] < 12)):
            raise TypeError(f"{method}: lo must be int32 rows at a stride that is a multiple of 4 bytes and at least 12")
        return VX_MEM_HOST, count, _vp(lo.ctypes.data), int(lo.strides[0]) if count else 12
    if str(lo.dtype) != "torch.int32" or (count and (lo.stride(1) != 1 or lo.stride(0) < 3)):
        raise TypeError(f"{method}: lo must be int32 rows whose last axis is contiguous, at a stride of at least 3 elements")
    return VX_MEM_DEVICE, count, _vp(lo.data_ptr()), 4 * int(lo.stride(0)) if count else 12


def _box_batch(method, names, origin, extents, offset, only_value, device, *more):
    """(vx_box_batch, count, memory kind) of overlap_boxes' and move_boxes' boxes; `more`: what else has to lie where they lie."""
    host = isinstance(origin, np.ndarray)
    if len(origin.shape) != 2 or origin.shape[1] != 3:
        raise TypeError(f"{method}: origin must have shape (N, 3)")
    count = int(origin.shape[0])
    given = [origin, extents, *more] + ([offset] if offset is not None else [])
    if host and (device or not all(isinstance(x, np.ndarray) for x in given)):
        raise TypeError(f"{method}: {names} must all be NumPy arrays, or -- device=True -- all torch CUDA tensors")
    if not host and not all(getattr(x, "is_cuda", False) for x in given):
        raise TypeError(f"{method}: {names} must all be NumPy arrays or all torch CUDA tensors")
    batch = BoxBatch()
    batch.origin, batch.origin_stride = _ray_vectors("origin", origin, count, 3, method)
    batch.extents, batch.extents_stride = _ray_vectors("extents", extents, count, 3, method)
    if offset is not None:
        batch.offset, batch.offset_stride = _ray_vectors("offset", offset, count, 3, method)
    batch.only_value = int(only_value)
    return batch, count, VX_MEM_HOST if host else VX_MEM_DEVICE


def _region(lo, size, out, device):
    """(lo, size, memory kind) of a region call: the box as the library reads it; the host's memory unless device=True or `out` is no NumPy array."""
    host = not device and (out is None or isinstance(out, np.ndarray))
    return (C.c_int32 * 3)(*(int(v) for v in lo)), (_u32 * 3)(*(int(v) for v in size)), VX_MEM_HOST if host else VX_MEM_DEVICE


def _ptr(x):
    """None, or where a NumPy array's or a torch tensor's first byte lies, as the library takes it."""
    if x is None:
        return None
    return _vp(x.ctypes.data if isinstance(x, np.ndarray) else x.data_ptr())


def _asked(x, none):
    """What a fields, info, pieces or paths argument asks for: None -- no output --, True -- fresh memory -- or the memory to write to. `none`: what
    None stands for in this method (flood_points and walk_points: none; light_boxes and label_boxes: fresh memory; False is none everywhere)."""
    if x is None:
        x = none
    return None if x is False else x


def _out(where, out, mem, count, dtype, shape, on, exact=True, what="N", unit="values"):
    """An output of `count` items of `dtype`. None: none. True: fresh memory -- a NumPy array of `shape`, or for device memory, on the device of
    `on` (a tensor, or a device's name), an int32 tensor of shape + (a record's words,), of `shape` for plain numbers (uint8 for bytes). Else
    the caller's, which has to be contiguous, writeable and of the dtype (a NumPy array) or on the device (a tensor), and hold exactly `count`
    items (exact=True), exactly in host memory and at least in device memory ("host"), or at least (False). where, what, unit: for the refusal."""
    if out is None:
        return None
    size, host = dtype.itemsize, mem == VX_MEM_HOST
    if out is True:
        if host:
            return np.zeros(shape, dtype=dtype)
        import torch

        return torch.empty(shape + (size // 4,) if dtype.names else shape, dtype=torch.uint8 if size == 1 else torch.int32, device=getattr(on, "device", on))
    if host:
        ok = isinstance(out, np.ndarray) and out.dtype == dtype and (out.size == count if exact else out.size >= count) and out.flags.c_contiguous and out.flags.writeable
    else:
        ok = getattr(out, "is_cuda", False) and out.is_contiguous()
        if ok:
            nbytes = out.numel() * out.element_size()
            ok = nbytes == count * size if exact is True else nbytes >= count * size
    if not ok:
        least = "" if exact is True or (exact and host) else "at least "
        if not host:
            raise TypeError(f"{where} must be a contiguous CUDA tensor of {least}{what}{f' x {size}' if size > 1 else ''} bytes")
        kind = f"array of {what} hip.{_DTYPE_NAMES[dtype]} records" if dtype.names else f"{dtype.name} array of {least}{what} {unit}"
        raise TypeError(f"{where} must be a writeable C-contiguous {kind}")
    return out


def _fields_out(method, fields, mem, count, shape, field_stride, on):
    """The `fields` of a field call (_out's None, True or the caller's): a row of bytes a query, field_stride apart -- 0: the shape's cells rounded
    up to 16."""
    stride = int(field_stride) if field_stride else (int(shape.size[0]) * int(shape.size[1]) * int(shape.size[2]) + 15) // 16 * 16
    return _out(f"{method}: fields", fields, mem, count * stride, _U8, (count, stride), on, False, "N x field_stride", "bytes")


def _trace_outputs(method, what, out, mem, count, px_shape, hit_shape, fmt, want_rgba, want_hits, on):
    """(pixels, records) of trace_rays and trace_views, None for what is not wanted: the members of `out`, which may be longer than `count`
    pixels or records, or fresh memory where one is None -- as _out's, but for the pixels, float32 or uint8 by fmt."""
    if not want_rgba and not want_hits:
        raise TypeError(f"{method}: nothing asked for")
    rgba, hits = out if out is not None else (None, None)
    host, bytes8 = mem == VX_MEM_HOST, fmt == VX_FORMAT_RGBA8
    if not want_rgba:
        rgba = None
    elif rgba is None:
        if host:
            rgba = np.zeros(px_shape, dtype=np.uint8 if bytes8 else np.float32)
        else:
            import torch

            rgba = torch.empty(px_shape, dtype=torch.uint8 if bytes8 else torch.float32, device=getattr(on, "device", on))
    if not want_hits:
        hits = None
    elif hits is None:
        hits = _out(None, True, mem, count, HIT_DTYPE, hit_shape, on)
    for a, size in ((rgba, 4 if bytes8 else 16), (hits, HIT_DTYPE.itemsize)):
        if a is None:
            continue
        if host and not (isinstance(a, np.ndarray) and a.nbytes >= count * size and a.flags.c_contiguous and a.flags.writeable):
            raise TypeError(f"{method}: an output must be a writeable C-contiguous array of at least {what} pixels / records")
        if not host and not (getattr(a, "is_cuda", False) and a.is_contiguous() and a.numel() * a.element_size() >= count * size):
            raise TypeError(f"{method}: an output must be a contiguous CUDA tensor of at least {what} pixels / records")
    return rgba, hits


def _device_ptr(x):
    """A device pointer (int) or anything with data_ptr() (a torch CUDA tensor)."""
    return int(x.data_ptr()) if hasattr(x, "data_ptr") else int(x)


class Svo:
    """`graphics::Svo` over the C ABI."""

    def __init__(self, svo_type, capacity_bytes, device=0):
        self._h = _vp()
        self.svo_type = svo_type
        _check(lib().vx_create(svo_type, capacity_bytes, device, C.byref(self._h)))

    def close(self):
        if getattr(self, "_h", None):
            lib().vx_destroy(self._h)
            self._h = None

    __del__ = close

    # -- resources ---------------------------------------------------------------------------------------
    def set_materials(self, materials):
        m = np.ascontiguousarray(materials, dtype=MATERIAL_DTYPE)
        _check(lib().vx_set_materials(self._h, m.ctypes.data_as(_vp), m.size))

    def set_textures(self, base_rgba8, mip_levels):
        """base_rgba8: uint8 [layers][h][w][4], row 0 = bottom (already flipped like TextureArrayBuilder does)."""
        t = np.ascontiguousarray(base_rgba8, dtype=np.uint8)
        layers, h, w, c = t.shape
        assert c == 4
        _check(lib().vx_set_textures(self._h, t.ctypes.data_as(_vp), w, h, layers, mip_levels))

    # -- Svo::update (svo.rs:171-189) ---------------------------------------------------------------------
    def update(self, world):
        ranges = world.updated_ranges()
        staging = lib().vx_staging_ptr(self._h)
        world.write_changes_to(staging + 4, lib().vx_arena_capacity(self._h), True)
        arr = (Range * max(len(ranges), 1))()
        for i, (s, n) in enumerate(ranges):
            arr[i].start, arr[i].length = s, n
        _check(lib().vx_commit(self._h, world.depth, C.cast(arr, _vp), len(ranges), world.size_in_bytes))

    def update_full(self, world):
        """First upload into a fresh buffer: WorldSvo::write_to (whole arena) instead of the dirty ranges, which a
        WorldSvo only tracks for ONE target buffer (they are cleared by the first write_changes_to)."""
        if not hasattr(world, "write_frame_to"):
            self.upload_frame(world.frame(pad_words=0), world.depth)
            return
        # straight into the staging buffer, as graphics::Svo::update writes into its mapped buffer (svo.rs:171-189): no copy on the way
        try:
            wrote = world.write_frame_to(lib().vx_staging_ptr(self._h), lib().vx_capacity(self._h))
        except ValueError as e:
            raise VoxelHipError(str(e)) from None
        header = 20 if self.svo_type == 1 else 4
        _check(lib().vx_commit_all(self._h, world.depth, max(wrote - 4 - header, 0)))

    def upload_frame(self, frame_words, depth):
        """Copies a complete mapped-buffer image ([f32 scale][header][arena]) into staging and commits all of it."""
        raw = np.ascontiguousarray(frame_words).view(np.uint8)
        cap = lib().vx_capacity(self._h)
        if raw.size > cap:
            raise VoxelHipError("frame larger than the world buffer")
        C.memmove(lib().vx_staging_ptr(self._h), raw.ctypes.data, raw.size)
        header = 20 if self.svo_type == 1 else 4
        _check(lib().vx_commit_all(self._h, depth, max(raw.size - 4 - header, 0)))

    def set_commit_mode(self, pipelined):
        """VX_COMMIT_PIPELINED: update() only posts the commit; a worker thread of the context does the rest."""
        _check(lib().vx_set_commit_mode(self._h, 1 if pipelined else 0))

    def commit_wait(self):
        _check(lib().vx_commit_wait(self._h))

    def get_stats(self):
        s = Stats()
        _check(lib().vx_get_stats(self._h, C.byref(s)))
        return dict(used_bytes=int(s.used_bytes), capacity_bytes=int(s.capacity_bytes), depth=int(s.depth))

    # -- Svo::render (svo.rs:196-229) ---------------------------------------------------------------------
    def render(self, uniforms, width, height, want_hits=False, tile_rank=0, tile_count=1, fmt=VX_FORMAT_RGBA32F):
        """Returns (image [h][w][4] -- float32, row 0 = bottom; or uint8 (fmt RGBA8), row 0 = top --, hits or None); tile-sharded
        calls return compact tile lists."""
        dt = np.uint8 if fmt == VX_FORMAT_RGBA8 else np.float32
        if tile_count > 1:
            n = local_tile_count(width, height, tile_rank, tile_count)
            img = np.zeros((n, TILE, TILE, 4), dtype=dt)
            hits = np.zeros((n, TILE, TILE), dtype=HIT_DTYPE) if want_hits else None
        else:
            img = np.zeros((height, width, 4), dtype=dt)
            hits = np.zeros((height, width), dtype=HIT_DTYPE) if want_hits else None
        t = Target(img.ctypes.data, hits.ctypes.data if want_hits else None, VX_MEM_HOST, tile_rank, tile_count, fmt)
        _check(lib().vx_render(self._h, C.byref(uniforms), width, height, C.byref(t)))
        return img, hits

    def render_device(self, uniforms, width, height, out_ptr, hits_ptr=None, tile_rank=0, tile_count=1, fmt=VX_FORMAT_RGBA32F):
        """Asynchronous render into device memory (e.g. a torch tensor's data_ptr()); pair with sync()."""
        t = Target(out_ptr, hits_ptr, VX_MEM_DEVICE, tile_rank, tile_count, fmt)
        _check(lib().vx_render(self._h, C.byref(uniforms), width, height, C.byref(t)))

    # -- pipelined presentation -------------------------------------------------------------------------------
    def present_begin(self, uniforms, width, height, fmt=VX_FORMAT_RGBA8):
        slot = _int(0)
        _check(lib().vx_present_begin(self._h, C.byref(uniforms), width, height, fmt, C.byref(slot)))
        return slot.value

    def present_wait(self, slot, width, height, fmt=VX_FORMAT_RGBA8):
        """The slot's image as a numpy VIEW of the library's pinned ring (copy it to keep it beyond three more frames)."""
        ptr, n = _vp(), _sz(0)
        _check(lib().vx_present_wait(self._h, slot, C.byref(ptr), C.byref(n)))
        dt = np.uint8 if fmt == VX_FORMAT_RGBA8 else np.float32
        buf = (C.c_char * n.value).from_address(ptr.value)
        return np.frombuffer(buf, dtype=dt).reshape(height, width, 4)

    # -- multi-GPU ------------------------------------------------------------------------------------------------
    def comm_init(self, nranks, rank, unique_id):
        _check(lib().vx_comm_init(self._h, nranks, rank, C.c_char_p(unique_id)))

    def comm_destroy(self):
        _check(lib().vx_comm_destroy(self._h))

    def set_comm_headroom(self, waves_per_cu):
        """Wave slots per CU left to RCCL's workgroups by a context whose communicator has more than one rank (vx_set_comm_headroom)."""
        _check(lib().vx_set_comm_headroom(self._h, int(waves_per_cu)))

    def gather_tiles(self, tiles_ptr, bytes_per_rank, gathered_ptr, root=0):
        ticket = _int(-1)
        _check(lib().vx_gather_tiles(self._h, tiles_ptr, bytes_per_rank, gathered_ptr, root, C.byref(ticket)))
        return ticket.value

    def render_gather(self, uniforms, width, height, tiles_ptr, bytes_per_rank, gathered_ptr, image_ptr, wait_ticket=-1, tile_rank=0, tile_count=1, fmt=VX_FORMAT_RGBA32F, root=0):
        """One sharded frame in one call (vx_render_gather): wait for the exchange that last read the list, render this rank's tiles, gather them to
        `root`, and assemble on the root. Returns the exchange's ticket."""
        t = Target(tiles_ptr, None, VX_MEM_DEVICE, tile_rank, tile_count, fmt)
        ticket = _int(-1)
        _check(lib().vx_render_gather(self._h, C.byref(uniforms), width, height, C.byref(t), bytes_per_rank, gathered_ptr, root, image_ptr, wait_ticket, C.byref(ticket)))
        return ticket.value

    def wait_gather(self, ticket):
        _check(lib().vx_wait_gather(self._h, ticket))

    def gather_query(self, ticket):
        """1 = that gather (and an assembly issued behind it on the communicator's stream) has finished, 0 = not yet, -1 = error. Never blocks."""
        return int(lib().vx_gather_query(self._h, ticket))

    def comm_profile_read(self):
        ms, n = C.c_double(0), _u32(0)
        _check(lib().vx_comm_profile_read(self._h, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    @property
    def comm_stream(self):
        return lib().vx_comm_stream(self._h)

    def assemble_tiles_format(self, tiles_ptr, stride_pixels, tile_count, width, height, out_ptr, fmt, stream):
        _check(lib().vx_assemble_tiles_format(self._h, tiles_ptr, stride_pixels, tile_count, width, height, out_ptr, fmt, _vp(stream or 0)))

    def render_counters(self, uniforms, width, height, tile_rank=0, tile_count=1):
        c = Counters()
        _check(lib().vx_render_counters(self._h, C.byref(uniforms), width, height, tile_rank, tile_count, C.byref(c)))
        return c.as_dict()

    # -- Svo::raycast (svo.rs:233-255) --------------------------------------------------------------------
    def raycast(self, tasks):
        tasks = np.ascontiguousarray(tasks, dtype=PICKER_TASK_DTYPE)
        out = np.zeros(tasks.size, dtype=PICKER_RESULT_DTYPE)
        _check(lib().vx_raycast(self._h, tasks.ctypes.data_as(_vp), tasks.size, out.ctypes.data_as(_vp)))
        return out

    def raycast_batch(self, origins, dirs, max_dst=-1.0, translucent=False, out=None):
        """vx_raycast_batch: picker.glsl for rays read where they lie; hits keep the block id (RAY_HIT_DTYPE).
        origins: (N, 3) float32, any row stride (a[:, :3] of an (N, 4) array, tasks["pos"], entity_positions(e)); dirs: (N, 3) or one (3,)
        for every ray; max_dst: a number for every ray, or (N,) float32 at any stride (tasks["max_dst"]).
        Host (NumPy arrays): synchronous; returns `out` or a fresh array of RAY_HIT_DTYPE.
        Device (torch CUDA tensors): returns after enqueueing, without synchronising -- pair with sync(); the hits are `out` or a fresh
        int32 tensor of shape (N, 8) on the rays' device, whose rows are vx_ray_hit records (ray_hits_to_numpy)."""
        b, count, mem = self._ray_batch(origins, dirs, max_dst, "raycast_batch")
        b.flags = VX_RAYS_TRANSLUCENT if translucent else 0
        out = _out("raycast_batch: out", True if out is None else out, mem, count, RAY_HIT_DTYPE, (count,), origins)
        _check(lib().vx_raycast_batch(self._h, C.byref(b), count, mem, _ptr(out)))
        return out

    def _ray_batch(self, origins, dirs, max_dst, method):
        """(vx_ray_batch, count, memory kind) of raycast_batch's three ray arguments."""
        host = isinstance(origins, np.ndarray)
        count = int(origins.shape[0]) if len(origins.shape) == 2 else -1
        if count < 0 or origins.shape[1] != 3:
            raise TypeError("raycast_batch: origins must have shape (N, 3)")
        b = RayBatch()
        per_ray = not isinstance(max_dst, (int, float, np.floating, np.integer))
        arrays = [origins, dirs] + ([max_dst] if per_ray else [])
        if any(isinstance(a, np.ndarray) != host for a in arrays) or (not host and not all(getattr(a, "is_cuda", False) for a in arrays)):
            raise TypeError("raycast_batch: origins, dirs and max_dst must all be NumPy arrays or all be torch CUDA tensors")
        b.origin, b.origin_stride = _ray_vectors("origins", origins, count, 3, method)
        b.dir, b.dir_stride = _ray_vectors("dirs", dirs, count, 3, method)
        if per_ray:
            b.max_dst, b.max_dst_stride = _ray_vectors("max_dst", max_dst, count, 1, method)
        else:
            b.max_dst, b.max_dst_stride, b.max_dst_all = None, 0, float(max_dst)
        return b, count, VX_MEM_HOST if host else VX_MEM_DEVICE

    def trace_rays(self, uniforms, origins, dirs, max_dst=-1.0, want_hits=False, fmt=VX_FORMAT_RGBA32F, out=None, want_rgba=True):
        """vx_trace_rays: world.glsl's trace_ray, or the sky, for rays read where they lie (the arguments of raycast_batch: NumPy arrays, or
        torch CUDA tensors). Returns (pixels, records). pixels: (N, 4) float32, or (N, 4) uint8 for fmt RGBA8; None with want_rgba=False.
        records: vx_hit (HIT_DTYPE) when want_hits, else None. out: (pixels, records) to write into instead of fresh arrays (either may be
        None to have a fresh one; they may be longer than N).
        Host: synchronous. Device: returns after enqueueing -- pair with sync(); records are an int32 tensor of shape (N, 12) (trace_hits_to_numpy)."""
        b, count, mem = self._ray_batch(origins, dirs, max_dst, "trace_rays")
        rgba, hits = _trace_outputs("trace_rays", "N", out, mem, count, (count, 4), (count,), fmt, want_rgba, want_hits, origins)
        _check(lib().vx_trace_rays(self._h, C.byref(uniforms), C.byref(b), count, mem, _ptr(rgba), fmt, _ptr(hits)))
        return rgba, hits

    def trace_views(self, views, width, height, want_hits=False, want_rgba=True, fmt=VX_FORMAT_RGBA32F, out=None, device=False):
        """vx_trace_views: world.glsl's main for every pixel of many small views in one launch. views: a list of Uniforms or a ctypes array of
        them (host memory always; free to change once the call returns). Returns (pixels, records). pixels: (count, H, W, 4) float32 with row 0
        at the bottom, or uint8 with the top row first for fmt RGBA8; None with want_rgba=False. records: (count, H * W) vx_hit (HIT_DTYPE) in
        the row order of that format when want_hits, else None. out: (pixels, records) to write into instead of fresh arrays (either may be None
        to have a fresh one; they may be longer than needed).
        Host: synchronous. Device (torch CUDA tensors in `out`, or device=True): returns after enqueueing -- pair with sync(); records are an int32
        tensor of shape (count, H * W, 12) (trace_hits_to_numpy)."""
        if not want_rgba and not want_hits:
            raise TypeError("trace_views: nothing asked for")
        table = views if isinstance(views, C.Array) else (Uniforms * max(len(views), 1))(*views)
        count = len(views)
        given = [a for a in (out or ()) if a is not None]
        if given and any(isinstance(a, np.ndarray) != isinstance(given[0], np.ndarray) for a in given):
            raise TypeError("trace_views: the outputs must both be NumPy arrays or both be torch CUDA tensors")
        if given:
            device = not isinstance(given[0], np.ndarray)
        mem = VX_MEM_DEVICE if device else VX_MEM_HOST
        rgba, hits = _trace_outputs("trace_views", "count * H * W", out, mem, count * width * height, (count, height, width, 4), (count, height * width), fmt,
                                    want_rgba, want_hits, "cuda")
        _check(lib().vx_trace_views(self._h, table, count, width, height, mem, _ptr(rgba), fmt, _ptr(hits)))
        return rgba, hits

    # -- block ids read from the device (gameplay.rs:161-201: get_block(floor(pos)), asked of the world the device holds) -----------------------
    def block_points(self, positions, out=None):
        """vx_block_points: the leaf, or the empty cell, that holds each position (BLOCK_CELL_DTYPE: value, cell_log2).
        positions: (N, 3) float32 at any row stride (a[:, :3] of an (N, 4) array, entity_positions(e), ray_hit_positions(hits)).
        Host (a NumPy array): synchronous; returns `out` or a fresh array of BLOCK_CELL_DTYPE.
        Device (a torch CUDA tensor): returns after enqueueing, without synchronising -- pair with sync(); the records are `out` or a fresh
        int32 tensor of shape (N, 2) on the positions' device (block_cells_to_numpy)."""
        mem, count, ptr, stride = _points("block_points", "positions", positions)
        out = _out("block_points: out", True if out is None else out, mem, count, BLOCK_CELL_DTYPE, (count,), positions)
        _check(lib().vx_block_points(self._h, ptr, stride, count, mem, _ptr(out)))
        return out

    def read_region(self, lo, size, out=None, device=False):
        """vx_read_region: the block ids of the box [lo, lo + size) in integer SVO coordinates, 0 outside the world, as a dense uint32 array
        indexed [z - lo.z][y - lo.y][x - lo.x] (x fastest). At most 2^24 voxels a call.
        Host (default): synchronous; returns `out` or a fresh NumPy array of shape (size.z, size.y, size.x).
        Device (device=True, or `out` a torch CUDA tensor): returns after enqueueing, without synchronising -- pair with sync(); the ids
        are `out` or a fresh int32 tensor of that shape (the bits of the uint32 ids)."""
        lo3, size3, mem = _region(lo, size, out, device)
        shape = (int(size[2]), int(size[1]), int(size[0]))
        out = _out("read_region: out", True if out is None else out, mem, shape[0] * shape[1] * shape[2], _U32, shape, "cuda", True, "size.x * size.y * size.z", "values")
        _check(lib().vx_read_region(self._h, C.byref(lo3), C.byref(size3), mem, _ptr(out)))
        return out

    def list_region(self, lo, size, flags=0, capacity=None, out=None, device=False):
        """vx_list_region: the blocks the box [lo, lo + size) holds as a compact list of BLOCK_AT_DTYPE records (where: read_region's index and
        the open faces, split_where; value), ascending by (z >> 3, y >> 3, x >> 3, z, y, x). flags: VX_LIST_FACES fills the face bits,
        VX_LIST_EXPOSED keeps only blocks with an open face. capacity: the most records to write (default: what `out` holds, or the box's
        voxels); 0 only counts. Returns (records, total): total is the number of records the box has, whatever the capacity.
        Host (default): synchronous; the records are the first min(total, capacity) of `out`, or a fresh array of that many; total an int.
        Device (device=True, or `out` a torch CUDA tensor): returns after enqueueing, without synchronising -- pair with sync(); the records
        are `out` or a fresh int32 tensor of shape (capacity, 2), of which the first min(total, capacity) rows are written
        (block_ats_to_numpy); total is an int32 tensor of one element on the device."""
        lo3, size3, mem = _region(lo, size, out, device)
        voxels = int(size[0]) * int(size[1]) * int(size[2])
        if mem == VX_MEM_HOST:
            if out is not None and (out.dtype != BLOCK_AT_DTYPE or not out.flags.c_contiguous or not out.flags.writeable):
                raise TypeError("list_region: out must be a writeable C-contiguous array of hip.BLOCK_AT_DTYPE records")
            total = _u32(0)
            if out is None:
                if capacity is None:  # count first: the array is as long as the list
                    _check(lib().vx_list_region(self._h, C.byref(lo3), C.byref(size3), int(flags), mem, None, 0, C.byref(total)))
                    capacity = total.value
                capacity = min(int(capacity), voxels)  # (a box has no more records than voxels)
                out = np.zeros(capacity, dtype=BLOCK_AT_DTYPE)
            held = out.size
        else:
            import torch

            if out is None:
                out = torch.empty((voxels if capacity is None else int(capacity), 2), dtype=torch.int32, device="cuda")
            elif not getattr(out, "is_cuda", False) or not out.is_contiguous() or (out.numel() * out.element_size()) % BLOCK_AT_DTYPE.itemsize:
                raise TypeError("list_region: out must be a contiguous CUDA tensor of whole 8-byte records")
            held = out.numel() * out.element_size() // BLOCK_AT_DTYPE.itemsize
            total = torch.zeros(1, dtype=torch.int32, device=out.device)
        capacity = held if capacity is None else int(capacity)
        if capacity > held:
            raise TypeError("list_region: out holds fewer than `capacity` records")
        _check(lib().vx_list_region(self._h, C.byref(lo3), C.byref(size3), int(flags), mem, _ptr(out) if capacity else None, capacity,
                                    C.byref(total) if mem == VX_MEM_HOST else _ptr(total)))
        return (out.reshape(-1)[:min(total.value, capacity)], total.value) if mem == VX_MEM_HOST else (out, total)

    # -- the first block along an axis (get_block, gameplay.rs:161-201, looped along it) ----------------------------------------------------------
    def scan_points(self, positions, direction, reach=VX_SCAN_TO_EDGE, out=None):
        """vx_scan_points: the first block from floor(position) on along `direction` (VX_DIR_*), at most `reach` voxels on, the start included
        (SCAN_HIT_DTYPE: coord along the axis or VX_SCAN_NONE, value, cell_log2). positions: as block_points takes them.
        Host (a NumPy array): synchronous; returns `out` or a fresh array of SCAN_HIT_DTYPE.
        Device (a torch CUDA tensor): returns after enqueueing, without synchronising -- pair with sync(); the records are `out` or a fresh
        int32 tensor of shape (N, 4) on the positions' device (scan_hits_to_numpy)."""
        mem, count, ptr, stride = _points("scan_points", "positions", positions)
        out = _out("scan_points: out", True if out is None else out, mem, count, SCAN_HIT_DTYPE, (count,), positions)
        _check(lib().vx_scan_points(self._h, ptr, stride, count, int(direction), int(reach), mem, _ptr(out)))
        return out

    def scan_columns(self, lo, size, direction, out=None, device=False):
        """vx_scan_columns: per column of the box [lo, lo + size) across the axis of `direction` (VX_DIR_*), the first block from the face the
        scan enters, as a dense array of SCAN_HIT_DTYPE indexed [v - lo.v][u - lo.u], u < v the two other axes (VX_DIR_NEG_Y: a heightmap
        [z][x]). At most 2^24 columns a call.
        Host (default): synchronous; returns `out` or a fresh NumPy array of shape (size.v, size.u).
        Device (device=True, or `out` a torch CUDA tensor): returns after enqueueing, without synchronising -- pair with sync(); the records
        are `out` or a fresh int32 tensor of shape (size.v, size.u, 4) (scan_hits_to_numpy)."""
        lo3, size3, mem = _region(lo, size, out, device)
        a = int(direction) >> 1
        u, v = (1 if a == 0 else 0), (1 if a == 2 else 2)
        shape = (int(size[v]), int(size[u])) if 0 <= a <= 2 and all(int(n) for n in size) else (0, 0)
        out = _out("scan_columns: out", True if out is None else out, mem, shape[0] * shape[1], SCAN_HIT_DTYPE, shape, "cuda", True, "size.u * size.v")
        _check(lib().vx_scan_columns(self._h, C.byref(lo3), C.byref(size3), int(direction), mem, _ptr(out)))
        return out

    # -- what float boxes hold (gameplay.rs:211-222: the player's AABB against a voxel, for a batch) -----------------------------------------------
    def overlap_boxes(self, origin, extents, offset=None, only_value=0, out=None, device=False):
        """vx_overlap_boxes: what each box [origin + offset, origin + offset + extents) holds (BOX_HIT_DTYPE: blocks -- the voxels of its cover
        that hold a block, or VX_BOX_INVALID --, value of the first of them, their bounds lo, hi). origin: (N, 3) float32 at any row stride;
        extents and offset: the same, or one (3,) vector for every box; offset None: no add (entity_boxes(e) gives all three of vx_entity
        records in place). only_value: 0 = every block counts, else only voxels of that id. At most 64 along each axis.
        Host (NumPy arrays): synchronous; returns `out` or a fresh array of BOX_HIT_DTYPE.
        Device (torch CUDA tensors; device=True insists on them): returns after enqueueing, without synchronising -- pair with sync(); the
        records are `out` or a fresh int32 tensor of shape (N, 8) on the origins' device (box_hits_to_numpy)."""
        batch, count, mem = _box_batch("overlap_boxes", "origin, extents and offset", origin, extents, offset, only_value, device)
        out = _out("overlap_boxes: out", True if out is None else out, mem, count, BOX_HIT_DTYPE, (count,), origin, "host")
        _check(lib().vx_overlap_boxes(self._h, C.byref(batch), count, mem, _ptr(out)))
        return out

    # -- float boxes moved through the world, stopped by blocks (what physics.rs:171-184 asks of the picker fan, of every voxel ahead) ---------------
    def move_boxes(self, origin, extents, motion, offset=None, scale=1.0, skin=2.0 ** -10, order=VX_MOVE_ORDER_YXZ, only_value=0, out=None, device=False):
        """vx_move_boxes: each box [origin + offset, origin + offset + extents) moved by motion * scale, axis by axis in `order`, stopped `skin`
        short of the first counted voxel ahead of its leading face (MOVE_HIT_DTYPE: the origin after the move, moved per axis, contacts -- or
        VX_MOVE_INVALID --, the stopping voxel's value per axis). The boxes as overlap_boxes takes them; motion: (N, 3) float32 at any row
        stride, or one (3,) vector for every box (entity_velocities(e) gives vx_entity.velocity in place, with scale = delta_time).
        Host (NumPy arrays): synchronous; returns `out` or a fresh array of MOVE_HIT_DTYPE.
        Device (torch CUDA tensors; device=True insists on them): returns after enqueueing, without synchronising -- pair with sync(); the
        records are `out` or a fresh int32 tensor of shape (N, 12) on the origins' device (move_hits_to_numpy)."""
        batch, count, mem = _box_batch("move_boxes", "origin, extents, motion and offset", origin, extents, offset, only_value, device, motion)
        motion_ptr, motion_stride = _ray_vectors("motion", motion, count, 3, "move_boxes")
        shape = MOVE_SHAPE(scale, skin, order)
        out = _out("move_boxes: out", True if out is None else out, mem, count, MOVE_HIT_DTYPE, (count,), origin, "host")
        _check(lib().vx_move_boxes(self._h, C.byref(batch), _vp(motion_ptr), motion_stride, count, C.byref(shape), mem, _ptr(out)))
        return out

    # -- step distances through air (a breadth-first search over get_block, gameplay.rs:161-201, for a batch) ----------------------------------------
    def flood_points(self, positions, size, seed_at=None, max_steps=VX_FLOOD_MAX_STEPS, pass_value=0, flags=0, fields=True, info=True, field_stride=0):
        """vx_flood_points: the breadth-first flood of the box of `size` cells (1..32 an axis) around each position, whose cell floor(p) is cell
        `seed_at` of the box (None: size // 2). positions: as block_points takes them. Returns (fields, info), either None when not asked for:
        fields -- uint8 [N, field_stride], of which the first size.x * size.y * size.z bytes of a row are the query's cells, x fastest (the step
        count, or VX_FLOOD_NO_POSITION, VX_FLOOD_UNREACHED, VX_FLOOD_BLOCKED); field_stride 0: the voxel count rounded up to 16 -- and info --
        FLOOD_INFO_DTYPE records. fields and info: True for fresh memory, False or None for none, or the memory to write to.
        Host (a NumPy array): synchronous.
        Device (a torch CUDA tensor): returns after enqueueing, without synchronising -- pair with sync(); fields is a uint8 tensor and info
        an int32 tensor of shape (N, 4) on the positions' device (flood_infos_to_numpy)."""
        mem, count, ptr, stride = _points("flood_points", "positions", positions)
        shape = flood_shape(size, seed_at, max_steps, pass_value, flags)
        fields = _fields_out("flood_points", _asked(fields, None), mem, count, shape, field_stride, positions)
        info = _out("flood_points: info", _asked(info, None), mem, count, FLOOD_INFO_DTYPE, (count,), positions, "host")
        _check(lib().vx_flood_points(self._h, ptr, stride, count, C.byref(shape), mem, _ptr(fields), int(field_stride), _ptr(info)))
        return fields, info

    # -- light levels (two breadth-first searches over get_block, gameplay.rs:161-201, for a batch of boxes) --------------------------------------------
    def light_boxes(self, lo, size, props, flags=0, fields=None, info=None, field_stride=0):
        """vx_light_boxes: the sky and block light levels of every cell of the boxes [lo_k, lo_k + size) (1..48 cells an axis). lo: int32 (N, 3),
        a NumPy array or a torch CUDA tensor, packed or a strided view whose last axis is contiguous (the stride a multiple of 4 bytes, at least
        12). props: uint8, props[id] = emission | VX_LIGHT_TRANSPARENT, always host memory. Returns (fields, info), either None when not asked for:
        fields -- uint8 [N, field_stride], of which the first size.x * size.y * size.z bytes of a row are the box's cells, x fastest, sky << 4 |
        block; field_stride 0: the voxel count rounded up to 16 -- and info -- LIGHT_INFO_DTYPE records. fields and info: None (or True) for fresh
        memory, False for none, or the memory to write to (unlike flood_points, where None stands for none).
        Host (a NumPy array): synchronous.
        Device (a torch CUDA tensor): returns after enqueueing, without synchronising -- pair with sync(); fields is a uint8 tensor and info
        an int32 tensor of shape (N, 4) on lo's device (light_infos_to_numpy)."""
        mem, count, ptr, stride = _lo_rows("light_boxes", lo)
        shape, table = light_shape(size, props, flags)
        fields = _fields_out("light_boxes", _asked(fields, True), mem, count, shape, field_stride, lo)
        info = _out("light_boxes: info", _asked(info, True), mem, count, LIGHT_INFO_DTYPE, (count,), lo, "host")
        _check(lib().vx_light_boxes(self._h, ptr, stride, count, C.byref(shape), mem, _ptr(fields), int(field_stride), _ptr(info)))
        del table  # (read during the call)
        return fields, info

    # -- loose pieces (connected components over get_block, gameplay.rs:161-201, for a batch of boxes) -----------------------------------------------
    def label_boxes(self, lo, size, anchor_faces=VX_LABEL_ALL_FACES, max_pieces=VX_LABEL_MAX_PIECES, max_steps=VX_LABEL_MAX_STEPS, pass_value=0, fields=None,
                    pieces=None, info=None, field_stride=0):
        """vx_label_boxes: the solid cells of the boxes [lo_k, lo_k + size) (1..32 cells an axis) that hang on nothing -- held from the faces
        anchor_faces names, the loose pieces labelled 1, 2, ... in the field's order, the rest VX_LABEL_MORE. lo: as light_boxes takes it.
        Returns (fields, pieces, info), each None when not asked for: fields -- uint8 [N, field_stride], of which the first size.x * size.y *
        size.z bytes of a row are the box's cells, x fastest; field_stride 0: the voxel count rounded up to 16 --, pieces -- LABEL_PIECE_DTYPE
        records [N, max_pieces] (none with max_pieces == 0) -- and info -- LABEL_INFO_DTYPE records. fields, pieces and info: None (or True)
        for fresh memory, False for none, or the memory to write to.
        Host (a NumPy array): synchronous.
        Device (a torch CUDA tensor): returns after enqueueing, without synchronising -- pair with sync(); fields is a uint8 tensor, pieces an
        int32 tensor of shape (N, max_pieces, 4) and info one of shape (N, 8) on lo's device (label_pieces_to_numpy, label_infos_to_numpy)."""
        mem, count, ptr, stride = _lo_rows("label_boxes", lo)
        shape = label_shape(size, anchor_faces, max_pieces, max_steps, pass_value)
        most = shape.max_pieces
        fields = _fields_out("label_boxes", _asked(fields, True), mem, count, shape, field_stride, lo)
        pieces = _out("label_boxes: pieces", _asked(pieces, most > 0), mem, count * most, LABEL_PIECE_DTYPE, (count, most), lo, "host", "N x max_pieces")
        info = _out("label_boxes: info", _asked(info, True), mem, count, LABEL_INFO_DTYPE, (count,), lo, "host")
        _check(lib().vx_label_boxes(self._h, ptr, stride, count, C.byref(shape), mem, _ptr(fields), int(field_stride), _ptr(pieces), _ptr(info)))
        return fields, pieces, info

    # -- squared distances to the nearest block (a distance transform over get_block, gameplay.rs:161-201, for a batch of boxes) -------------------------
    def distance_boxes(self, lo, size, pass_value=0, match_value=0, flags=0, fields=None, info=None, field_stride=0):
        """vx_distance_boxes: for every cell of the boxes [lo_k, lo_k + size) (1..32 cells an axis) the squared distance, in cells, to the nearest
        target cell of the box -- a solid cell (non-zero and not pass_value), or with match_value the cells of that id; under VX_DISTANCE_TO_AIR
        the others. lo: as light_boxes takes it. Returns (fields, info), either None when not asked for: fields -- uint16 [N, field_stride / 2],
        of which the first size.x * size.y * size.z entries of a row are the box's cells, x fastest, VX_DISTANCE_NONE everywhere when the box
        holds no target; field_stride, in BYTES, 0: twice the voxel count rounded up to 16 -- and info -- DISTANCE_INFO_DTYPE records. fields and
        info: None (or True) for fresh memory, False for none, or the memory to write to.
        Host (a NumPy array): synchronous.
        Device (a torch CUDA tensor): returns after enqueueing, without synchronising -- pair with sync(); fields is an int16 tensor, in which
        VX_DISTANCE_NONE reads as -1 (distance_fields_to_numpy), and info an int32 tensor of shape (N, 4) on lo's device
        (distance_infos_to_numpy)."""
        mem, count, ptr, stride = _lo_rows("distance_boxes", lo)
        shape = distance_shape(size, pass_value, match_value, flags)
        entries = (int(field_stride) if field_stride else (2 * int(shape.size[0]) * int(shape.size[1]) * int(shape.size[2]) + 15) // 16 * 16) // 2
        fields = _asked(fields, True)
        if fields is True and mem == VX_MEM_DEVICE:
            import torch

            fields = torch.empty((count, entries), dtype=torch.int16, device=lo.device)
        fields = _out("distance_boxes: fields", fields, mem, count * entries, _U16, (count, entries), lo, False, "N x field_stride / 2", "entries")
        info = _out("distance_boxes: info", _asked(info, True), mem, count, DISTANCE_INFO_DTYPE, (count,), lo, "host")
        _check(lib().vx_distance_boxes(self._h, ptr, stride, count, C.byref(shape), mem, _ptr(fields), int(field_stride), _ptr(info)))
        return fields, info

    # -- walking distances and paths (a search over get_block, gameplay.rs:161-201, on the walking graph, for a batch) --------------------------------
    def walk_points(self, positions, size, goals=None, seed_at=None, max_steps=VX_WALK_MAX_STEPS, pass_value=0, height=2, climb=1, drop=3, path_capacity=0, flags=0,
                    fields=True, info=True, paths=None, field_stride=0):
        """vx_walk_points: breadth-first step counts over the walking graph (a floor below, `height` cells of headroom, one block up with climb,
        up to `drop` down) of the box of `size` cells around each position, and the path to each goal. positions: as flood_points takes them.
        goals: None, float32 (N, 3) at any row stride, or (3,): one goal for all; on the positions' side (host or device). Returns (fields,
        info, paths), each None when not asked for: fields -- uint8 [N, field_stride] as flood_points' (the step count, or VX_WALK_NO_POSITION,
        VX_WALK_UNREACHED, VX_WALK_NO_STAND) --, info -- WALK_INFO_DTYPE records --, paths -- uint32 [N, path_capacity], entry i the cell after
        i + 1 steps as rx | ry << 8 | rz << 16, VX_WALK_NONE beyond the path. fields, info, paths: True for fresh memory, False or None for none,
        or the memory to write to; paths None: fresh memory when goals are given and path_capacity > 0.
        Host (a NumPy array): synchronous.
        Device (a torch CUDA tensor): returns after enqueueing, without synchronising -- pair with sync(); fields is a uint8 tensor, info an
        int32 tensor of shape (N, 8) (walk_infos_to_numpy) and paths an int32 tensor of shape (N, path_capacity) on the positions' device."""
        mem, count, ptr, stride = _points("walk_points", "positions", positions)
        if goals is not None and isinstance(goals, np.ndarray) != (mem == VX_MEM_HOST):
            raise TypeError("walk_points: goals must lie where the positions lie")
        shape = walk_shape(size, seed_at, max_steps, pass_value, height, climb, drop, path_capacity, flags)
        goal_ptr, goal_stride = (None, 0) if goals is None else _ray_vectors("goals", goals, count, 3, "walk_points")
        cap = int(path_capacity)
        fields = _fields_out("walk_points", _asked(fields, None), mem, count, shape, field_stride, positions)
        info = _out("walk_points: info", _asked(info, None), mem, count, WALK_INFO_DTYPE, (count,), positions, "host")
        paths = _out("walk_points: paths", _asked(paths, goals is not None and cap > 0), mem, count * cap, _U32, (count, cap), positions, False, "N x path_capacity", "entries")
        _check(lib().vx_walk_points(self._h, ptr, stride, None if goal_ptr is None else _vp(goal_ptr), goal_stride, count, C.byref(shape), mem, _ptr(fields),
                                    int(field_stride), _ptr(paths), _ptr(info)))
        return fields, info, paths

    # -- Physics::step_many (src/systems/physics.rs:122-136), on the device ---------------------------------------
    def physics_step(self, entities, dt, steps=1, want_contacts=False, count=None, contacts=None):
        """vx_physics_step: `steps` fixed steps of `dt` for every entity in one launch.
        Host: `entities` is a C-contiguous NumPy array of ENTITY_DTYPE, updated in place; synchronous; returns the contacts
        (AABB_RESULT_DTYPE) when want_contacts, else None.
        Device: `entities` is a torch CUDA tensor (its bytes are vx_entity records) or a raw device pointer with `count`; the call
        returns after enqueueing -- pair with sync(). want_contacts: into `contacts` (a device tensor or pointer of count x 24 bytes)
        or, for a tensor, into a fresh float32 tensor of shape (count, 6), which is returned."""
        if isinstance(entities, np.ndarray):
            if entities.dtype != ENTITY_DTYPE or not entities.flags.c_contiguous or not entities.flags.writeable:
                raise TypeError("physics_step: host entities must be a writeable C-contiguous array of hip.ENTITY_DTYPE")
            out = np.zeros(entities.size, dtype=AABB_RESULT_DTYPE) if want_contacts else None
            _check(lib().vx_physics_step(self._h, entities.ctypes.data_as(_vp), entities.size, VX_MEM_HOST, float(dt), int(steps),
                                         out.ctypes.data_as(_vp) if want_contacts else None))
            return out
        if count is None:
            if not hasattr(entities, "numel"):
                raise TypeError("physics_step: a raw device pointer needs count")
            nbytes = entities.numel() * entities.element_size()
            if nbytes % ENTITY_DTYPE.itemsize or not entities.is_contiguous():
                raise TypeError("physics_step: a device tensor must be contiguous and hold whole 64-byte vx_entity records")
            count = nbytes // ENTITY_DTYPE.itemsize
        out = contacts
        if want_contacts and out is None:
            if not hasattr(entities, "new_empty"):
                raise TypeError("physics_step: contacts of a raw device pointer need a `contacts` pointer")
            import torch

            out = torch.empty((count, 6), dtype=torch.float32, device=entities.device)
        _check(lib().vx_physics_step(self._h, _vp(_device_ptr(entities)), count, VX_MEM_DEVICE, float(dt), int(steps),
                                     _vp(_device_ptr(out)) if out is not None else None))
        return out

    def debug_trace(self, pos, direction, max_dst, cast_translucent, max_frames=100):
        p = (C.c_float * 3)(*[float(x) for x in pos])
        d = (C.c_float * 3)(*[float(x) for x in direction])
        res = Result()
        frames = np.zeros(max(max_frames, 1), dtype=FRAME_DTYPE)
        n = _u32(0)
        _check(lib().vx_debug_trace(self._h, C.byref(p), C.byref(d), max_dst, int(cast_translucent), C.byref(res), frames.ctypes.data_as(_vp),
                                    max_frames, C.byref(n)))
        return res, frames[:min(n.value, max_frames)], n.value

    def assemble_tiles(self, tiles_ptr, stride_floats, tile_count, width, height, out_ptr, stream=None):
        """stream = a raw hipStream_t to launch on (default: the context's own stream)."""
        if stream is None:
            _check(lib().vx_assemble_tiles(self._h, tiles_ptr, stride_floats, tile_count, width, height, out_ptr))
        else:
            _check(lib().vx_assemble_tiles_on(self._h, tiles_ptr, stride_floats, tile_count, width, height, out_ptr, _vp(stream)))

    def resolve_2x2(self, src_ptr, width, height, dst_ptr, stream=None):
        """Box-filters a (2*width x 2*height) device image down to width x height on the raw hipStream_t `stream`."""
        _check(lib().vx_resolve_2x2(self._h, src_ptr, width, height, dst_ptr, _vp(stream or 0)))

    def sync(self):
        _check(lib().vx_sync(self._h))

    def set_frames_in_flight(self, frames):
        _check(lib().vx_set_frames_in_flight(self._h, frames))

    def wait_event(self, hip_event):
        """The next render waits for this raw hipEvent_t (e.g. torch.cuda.Event.cuda_event)."""
        _check(lib().vx_wait_event(self._h, _vp(hip_event)))

    def stream_wait_render(self, stream):
        """Makes the raw hipStream_t `stream` wait for the most recently issued render."""
        _check(lib().vx_stream_wait_render(self._h, _vp(stream)))

    def timeline(self):
        """Per wave of the last launch: [start, queue empty, exit] in 10 ns ticks, sub-tiles taken | phases | ticks in them, then the
        wave's life and its traversal loop in shader cycles and the loop's trips (voxel_hip.h: vx_timeline_read; needs VX_TIMELINE=1)."""
        out = np.zeros((8192, 8), dtype=np.uint64)
        n = lib().vx_timeline_read(self._h, out.ctypes.data_as(_vp), 8192)
        return out[:n]

    def knobs(self):
        """vx_debug_knobs: the scheduling knobs the context runs with."""
        out = (_u32 * 8)()
        _check(lib().vx_debug_knobs(self._h, C.byref(out)))
        v = [int(x) for x in out]
        v[7:] = [v[7] & 1, (v[7] >> 1) & 1]  # the last word: the measurement build | the whole-frame build in use << 1
        return dict(zip(("refill_min", "service_min", "waves_per_cu", "queue_stripe", "tile_strip", "hot_first", "comm_headroom", "measurement_build", "plain_frame"), v))

    def image_info(self):
        out = (_u64 * 4)()
        _check(lib().vx_image_info(self._h, C.byref(out)))
        return {"layout": int(out[0]), "image_bytes": int(out[1]), "origin_bytes": int(out[2]), "chunks": int(out[3])}

    def excursion_counters(self, reset=True, stop=False):
        """Reads the counters of the walks inside voxels. reset=True zeroes them and (re)starts the counting -- it is off until first asked for, it
        costs frame time --; stop=True zeroes them and switches it off again."""
        out = (_u64 * 4)()
        _check(lib().vx_excursion_counters(self._h, C.byref(out), 2 if stop else int(reset)))
        return {"rays": int(out[0]), "started_over": int(out[1]), "service_phases": int(out[2]), "iterations_on_bytes": int(out[3])}

    def clock_probe(self, microseconds=200):
        """The shader clock (MHz) the device runs at during the call (vx_clock_probe); callable from a second thread while frames render."""
        mhz = C.c_double(0)
        _check(lib().vx_clock_probe(self._h, microseconds, C.byref(mhz)))
        return mhz.value

    def profile_enable(self, on=True):
        _check(lib().vx_profile_enable(self._h, int(on)))

    def profile_read(self):
        ms, n = C.c_double(0), _u32(0)
        _check(lib().vx_profile_read(self._h, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    @property
    def stream(self):
        return lib().vx_stream(self._h)

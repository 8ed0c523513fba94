//! Raw FFI of `libvoxelhip.so` (include/voxel_hip.h): the MI355X drop-in for the OpenGL side of `graphics::Svo`.
//!
//! Goes to `src/graphics/voxel_hip_sys.rs`. Every item mirrors one declaration of the C header, in the header's order; layouts are
//! `#[repr(C)]` and checked at compile time against the sizes the header's structs have. Link with
//! `println!("cargo:rustc-link-lib=dylib=voxelhip");` (and a `rustc-link-search` to where the library is installed) in `build.rs`.
#![allow(non_camel_case_types, dead_code)]

use std::os::raw::{c_char, c_int, c_void};

use crate::graphics::svo_picker::{PickerResult, PickerTask};
use crate::graphics::svo_registry::MaterialInstance;

pub const VX_SVO_ESVO: c_int = 1; // = SvoType::Esvo.shader_type_define (svo.rs:35)
pub const VX_SVO_CSVO: c_int = 2; // = SvoType::Csvo.shader_type_define (svo.rs:36)

pub const VX_OK: c_int = 0;
pub const VX_ERR_INVALID_ARGUMENT: c_int = 1;
pub const VX_ERR_NO_DEVICE: c_int = 2;
pub const VX_ERR_OUT_OF_MEMORY: c_int = 3;
pub const VX_ERR_CAPACITY: c_int = 4;
pub const VX_ERR_HIP: c_int = 5;
pub const VX_ERR_STATE: c_int = 6;

pub const VX_MEM_HOST: i32 = 0;
pub const VX_MEM_DEVICE: i32 = 1;
pub const VX_FORMAT_RGBA32F: i32 = 0;
pub const VX_FORMAT_RGBA8: i32 = 1;
pub const VX_COMM_ID_BYTES: usize = 128;
pub const VX_ENTITY_WALL_CLIP: u32 = 1; // vx_entity.flags: EntityCapabilities::wall_clip (physics.rs:39)
pub const VX_ENTITY_FLYING: u32 = 2; // EntityCapabilities::flying (physics.rs:41)
pub const VX_RAYS_TRANSLUCENT: u32 = 1; // vx_ray_batch.flags: intersect_octree's cast_translucent (picker.glsl passes false)

/// Opaque: replaces `struct Svo`'s GL objects (svo.rs:56-73).
#[repr(C)]
pub struct vx_context {
    _private: [u8; 0],
}

/// One dirty range of the serialized arena: `RangeBuffer::updated_ranges` (internal.rs:151-154,166), in bytes.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct vx_range {
    pub start: u64,
    pub length: u64,
}

/// The uniforms `Svo::render` sets on world.glsl (svo.rs:201-215).
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct vx_uniforms {
    pub view: [f32; 16],
    pub fovy: f32,
    pub aspect: f32,
    pub ambient: f32,
    pub light_dir: [f32; 3],
    pub cam_pos: [f32; 3],
    pub render_shadows: i32,
    pub shadow_distance: f32,
    pub highlight_pos: [f32; 3],
}

#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct vx_hit {
    pub t: f32,
    pub value: u32,
    pub face_id: i32,
    pub flags: u32,
    pub pos: [f32; 3],
    pub lod: f32,
    pub uv: [f32; 2],
    pub shadow_t: f32,
    pub steps: u32,
}

/// What `Physics::update_entity` reads and writes of an `Entity` (physics.rs:10-75, 138-170).
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct vx_entity {
    pub position: [f32; 3],
    pub velocity: [f32; 3],
    pub aabb_offset: [f32; 3],
    pub aabb_extents: [f32; 3],
    pub gravity: f32,
    pub max_fall_velocity: f32,
    pub flags: u32,
    pub grounded: u32,
}

/// `AabbResult` (svo_picker.rs:163-176): -1 = none.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct vx_aabb_result {
    pub neg: [f32; 3],
    pub pos: [f32; 3],
}

/// A batch of rays read where they lie (`vx_raycast_batch`): byte strides, multiples of 4; `dir_stride == 0`: one direction for every
/// ray; `max_dst` null: `max_dst_all` for every ray. Every pointer is in the memory kind given to the call.
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct vx_ray_batch {
    pub origin: *const c_void,
    pub dir: *const c_void,
    pub max_dst: *const c_void,
    pub origin_stride: u32,
    pub dir_stride: u32,
    pub max_dst_stride: u32,
    pub max_dst_all: f32,
    pub flags: u32,
}

/// `PickerResult` (svo_picker.rs:24-32) with the block id kept and the normal as its face (0..5 = -x,+x,-y,+y,-z,+z); `dst == -1`: no
/// hit, every other field 0.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq)]
pub struct vx_ray_hit {
    pub dst: f32,
    pub value: u32,
    pub face_id: i32,
    pub inside_voxel: u32,
    pub pos: [f32; 3],
    pub _pad: u32,
}

/// The leaf, or the empty cell, that holds a point (`vx_block_points`): the block id (0 = no block) and log2 of the answering cell's side
/// (0: a full-detail block), or `VX_CELL_OUTSIDE` for a point outside the world.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct vx_block_cell {
    pub value: u32,
    pub cell_log2: u32,
}
/// `vx_block_cell::cell_log2` of a point outside [0, 2^depth)^3 (the header's VX_CELL_OUTSIDE)
pub const VX_CELL_OUTSIDE: u32 = u32::MAX;

/// One block of a box (`vx_list_region`). `where`: bits 0..23 the voxel's index in `vx_read_region`'s dense array of the same box, bits 24..29
/// its open faces (bit f, numbered like `face_id`, set when the neighbour on that side holds no block; 0 without `VX_LIST_FACES`).
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct vx_block_at {
    pub r#where: u32,
    pub value: u32,
}
/// `vx_list_region` flags (the header's VX_LIST_FACES, VX_LIST_EXPOSED): fill the face bits; keep only blocks with an open face
pub const VX_LIST_FACES: u32 = 0x1;
pub const VX_LIST_EXPOSED: u32 = 0x2;
/// the header's VX_AT_INDEX and VX_AT_FACES
pub const fn vx_at_index(at: u32) -> u32 { at & 0xFF_FFFF }
pub const fn vx_at_faces(at: u32) -> u32 { (at >> 24) & 0x3F }

/// The first voxel holding a block along an axis (`vx_scan_points`, `vx_scan_columns`): its coordinate along the scan axis (`VX_SCAN_NONE`:
/// no block), its block id and log2 of the answering leaf's side (`VX_CELL_OUTSIDE`: a position with a NaN or infinite component).
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct vx_scan_hit {
    pub coord: i32,
    pub value: u32,
    pub cell_log2: u32,
    pub _pad: u32,
}
/// directions of travel of a scan, numbered like `face_id`
pub const VX_DIR_NEG_X: c_int = 0;
pub const VX_DIR_POS_X: c_int = 1;
pub const VX_DIR_NEG_Y: c_int = 2;
pub const VX_DIR_POS_Y: c_int = 3;
pub const VX_DIR_NEG_Z: c_int = 4;
pub const VX_DIR_POS_Z: c_int = 5;
/// `vx_scan_hit::coord` when no block was found (the header's VX_SCAN_NONE)
pub const VX_SCAN_NONE: i32 = i32::MIN;
/// `reach`: as far as the world goes (the header's VX_SCAN_TO_EDGE)
pub const VX_SCAN_TO_EDGE: u32 = u32::MAX;

/// A batch of axis-aligned boxes read where they lie (`vx_overlap_boxes`): box i spans [mn, mx) with mn = origin[i] + offset[i] (offset null:
/// mn = origin[i]) and mx = mn + extents[i]. Strides in bytes, multiples of 4; origin_stride >= 12; offset_stride and extents_stride >= 12, or
/// 0 = that one vector for every box. `vx_entity` records are read in place: &e[0].position, &e[0].aabb_offset, &e[0].aabb_extents, strides 64.
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct vx_box_batch {
    pub origin: *const c_void,
    pub offset: *const c_void,
    pub extents: *const c_void,
    pub origin_stride: u32,
    pub offset_stride: u32,
    pub extents_stride: u32,
    pub only_value: u32,
}
/// What a box holds (`vx_overlap_boxes`): the voxels of its cover that hold a (counted) block (`VX_BOX_INVALID`: the record described no
/// box), the block id of the first of them in `vx_read_region`'s order, and their bounds [lo, hi) in SVO coordinates.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct vx_box_hit {
    pub blocks: u32,
    pub value: u32,
    pub lo: [i32; 3],
    pub hi: [i32; 3],
}
/// `vx_box_hit::blocks` of a record that described no box (the header's VX_BOX_INVALID)
pub const VX_BOX_INVALID: u32 = u32::MAX;

/// What every box of a `vx_move_boxes` call shares: displacement = motion * scale (one fp32 multiply a component), the gap a stopped box
/// keeps from the block that stopped it (0..=1), the order of the passes (a permutation of the axes in bits 0..1, 2..3, 4..5), and 0.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq)]
pub struct vx_move_shape {
    pub scale: f32,
    pub skin: f32,
    pub order: u32,
    pub flags: u32,
}
/// How far a box got (`vx_move_boxes`): its origin after the move, what was added to it per axis, the sides on which a block lay ahead (bit
/// 2a + (d_a > 0), numbered like face_id; `VX_MOVE_INVALID`: no box, or no motion), per axis the stopping voxel's block id; `_pad` is written 0.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq)]
pub struct vx_move_hit {
    pub origin: [f32; 3],
    pub moved: [f32; 3],
    pub contacts: u32,
    pub value: [u32; 3],
    pub _pad: [u32; 2],
}
/// `vx_move_hit::contacts` of a record that described no box or no motion (the header's VX_MOVE_INVALID)
pub const VX_MOVE_INVALID: u32 = u32::MAX;
/// the largest displacement along an axis (the header's VX_MOVE_MAX_TRAVEL)
pub const VX_MOVE_MAX_TRAVEL: f32 = 64.0;
/// `vx_move_shape::order`: y, then x, then z (the header's VX_MOVE_ORDER_YXZ)
pub const VX_MOVE_ORDER_YXZ: u32 = 0x21;

/// What every query of a `vx_flood_points` call shares: the box of each query (1..32 cells an axis), the seed's cell inside it (lo =
/// floor(p) - seed_at), the step limit (0..=VX_FLOOD_MAX_STEPS), a block id that passes like air (0: none), and 0 or VX_FLOOD_SEED_ALWAYS.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct vx_flood_shape {
    pub size: [u32; 3],
    pub seed_at: [u32; 3],
    pub max_steps: u32,
    pub pass_value: u32,
    pub flags: u32,
}
/// What a flood reached (`vx_flood_points`): the cells with a step count (`VX_FLOOD_INVALID`: no position), the largest step count, the faces
/// of the box a reached cell lies on (bit f numbered like face_id; 0 = enclosed), and `vx_block_points`' value at the seed.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct vx_flood_info {
    pub reached: u32,
    pub farthest: u32,
    pub faces: u32,
    pub seed_value: u32,
}
/// the header's VX_FLOOD_* (written in hexadecimal there and here)
pub const VX_FLOOD_MAX_STEPS: u32 = 0xFA;
/// a field's bytes that are no step count: of a position that is no position; passable but not reached; not passable
pub const VX_FLOOD_NO_POSITION: u8 = 0xFD;
pub const VX_FLOOD_UNREACHED: u8 = 0xFE;
pub const VX_FLOOD_BLOCKED: u8 = 0xFF;
/// `vx_flood_shape::flags`: the seed cell is step 0 and spreads even if it holds a block
pub const VX_FLOOD_SEED_ALWAYS: u32 = 0x1;
/// `vx_flood_info::reached` of a position that is no position
pub const VX_FLOOD_INVALID: u32 = u32::MAX;

/// What every query of a `vx_light_boxes` call shares: the box of each query (1..=VX_LIGHT_MAX_SIDE cells an axis), 0 or one of
/// VX_LIGHT_NO_SKY and VX_LIGHT_NO_BLOCKS, and the table of props -- HOST memory whatever the call's memory kind, read during the call:
/// props[id] = emission (bits 0..3) | VX_LIGHT_TRANSPARENT; ids at or above props_count (at most VX_LIGHT_MAX_PROPS) are opaque and dark.
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct vx_light_shape {
    pub size: [u32; 3],
    pub flags: u32,
    pub props: *const u8,
    pub props_count: u32,
}
/// What the light of a box amounts to (`vx_light_boxes`): the cells whose byte is not 0, the cells that emit (0 under VX_LIGHT_NO_BLOCKS),
/// the columns whose top cell is exposed to the sky (0 under VX_LIGHT_NO_SKY), and the faces of the box (bit f numbered like face_id) on
/// which a cell has a level of 2 or more in either channel.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct vx_light_info {
    pub lit: u32,
    pub sources: u32,
    pub open_columns: u32,
    pub faces: u32,
}
/// the header's VX_LIGHT_* (48 and 4,096, written in hexadecimal here)
pub const VX_LIGHT_MAX_SIDE: u32 = 0x30;
pub const VX_LIGHT_MAX_PROPS: u32 = 0x1000;
/// a props byte's bit 4: light passes through this block
pub const VX_LIGHT_TRANSPARENT: u8 = 0x10;
/// `vx_light_shape::flags`: leave that channel 0
pub const VX_LIGHT_NO_SKY: u32 = 0x1;
pub const VX_LIGHT_NO_BLOCKS: u32 = 0x2;
pub const VX_LIGHT_INVALID: u32 = u32::MAX;

/// What every query of a `vx_walk_points` call shares: the box of each query (1..32 cells on x and z; size[1] + height <= 32), the seed's cell
/// inside it (lo = floor(p) - seed_at), the step limit (0..=VX_WALK_MAX_STEPS), a block id that passes like air (0: none), the agent's height
/// (1..=4 cells of headroom), the step up it can take (0 or 1), the most it steps down (0..=3), the entries of a query's path (0..=252, a
/// multiple of 4), and 0 or VX_WALK_STOP_AT_GOAL.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct vx_walk_shape {
    pub size: [u32; 3],
    pub seed_at: [u32; 3],
    pub max_steps: u32,
    pub pass_value: u32,
    pub height: u32,
    pub climb: u32,
    pub drop: u32,
    pub path_capacity: u32,
    pub flags: u32,
}
/// What a walk reached (`vx_walk_points`): `reached`, `farthest`, `faces` and `seed_value` as `vx_flood_info`'s, over standable cells; the y
/// inside the box of the cells the seed and the goal settled on (`VX_WALK_NONE`: it stands nowhere; for the goal also: none given, outside the
/// box); the goal's step count (`VX_WALK_NONE`: not reached); `_pad` is written 0.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct vx_walk_info {
    pub reached: u32,
    pub farthest: u32,
    pub faces: u32,
    pub seed_value: u32,
    pub start_ry: u32,
    pub goal_ry: u32,
    pub path_steps: u32,
    pub _pad: u32,
}
/// the header's VX_WALK_* (written in hexadecimal there and here)
pub const VX_WALK_MAX_STEPS: u32 = 0xFA;
/// a field's bytes that are no step count: of a position that is no position; standable but not reached; not standable
pub const VX_WALK_NO_POSITION: u8 = 0xFD;
pub const VX_WALK_UNREACHED: u8 = 0xFE;
pub const VX_WALK_NO_STAND: u8 = 0xFF;
/// `vx_walk_shape::flags`: the flood ends after the whole step that reaches the settled goal
pub const VX_WALK_STOP_AT_GOAL: u32 = 0x1;
/// no cell, no step count: `vx_walk_info::start_ry`, `goal_ry`, `path_steps`, and a path's entries beyond its end
pub const VX_WALK_NONE: u32 = u32::MAX;

/// What every query of a `vx_label_boxes` call shares: the box of each query (1..=32 cells an axis), the faces of the box (bits 0..=5: -x, +x,
/// -y, +y, -z, +z) on which a solid cell is held, the most pieces to label (0..=VX_LABEL_MAX_PIECES), the step budget of all floods of a query
/// together (0..=VX_LABEL_MAX_STEPS), a block id that counts as air (0: none), and flags (0).
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct vx_label_shape {
    pub size: [u32; 3],
    pub anchor_faces: u32,
    pub max_pieces: u32,
    pub max_steps: u32,
    pub pass_value: u32,
    pub flags: u32,
}
/// One loose piece of a box (`vx_label_boxes`): its cells (0: no such piece, the whole record is 0), its bounds inside the box as
/// rx | ry << 8 | rz << 16 (both inclusive), and its first cell in the same form | faces << 24 (bit f: a cell of it lies on face f of the box).
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct vx_label_piece {
    pub cells: u32,
    pub lo: u32,
    pub hi: u32,
    pub r#where: u32,
}
/// What the solid cells of a box fall into (`vx_label_boxes`): `solid == held + loose + more`; `pieces` labelled pieces of `loose` cells; the
/// budget used; the faces of the box a solid cell lies on; 0 or VX_LABEL_CUT.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct vx_label_info {
    pub solid: u32,
    pub held: u32,
    pub pieces: u32,
    pub loose: u32,
    pub more: u32,
    pub steps: u32,
    pub faces: u32,
    pub flags: u32,
}
/// the header's VX_LABEL_* (250 and 4,096, written in hexadecimal here)
pub const VX_LABEL_MAX_PIECES: u32 = 0xFA;
pub const VX_LABEL_MAX_STEPS: u32 = 0x1000;
/// a field's bytes: not solid; 1..=pieces: the piece's label; solid but neither held nor labelled; held
pub const VX_LABEL_AIR: u8 = 0x00;
pub const VX_LABEL_MORE: u8 = 0xFE;
pub const VX_LABEL_HELD: u8 = 0xFF;
pub const VX_LABEL_ALL_FACES: u32 = 0x3F;
/// `vx_label_info::flags`: the step budget ran out
pub const VX_LABEL_CUT: u32 = 0x1;

/// What every query of a `vx_distance_boxes` call shares: the box of each query (1..=32 cells an axis), a block id that counts as air (0: none;
/// 0 with a match_value), the block id whose cells are the targets (0: every solid cell), and flags (0 or VX_DISTANCE_TO_AIR).
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct vx_distance_shape {
    pub size: [u32; 3],
    pub pass_value: u32,
    pub match_value: u32,
    pub flags: u32,
    pub _pad: [u32; 2],
}
/// What the distances of a box amount to (`vx_distance_boxes`): the target cells, the largest value of the field (VX_DISTANCE_NONE: no
/// target), the first cell in the field's order that holds it as rx | ry << 8 | rz << 16, and the faces of the box a target lies on.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct vx_distance_info {
    pub targets: u32,
    pub farthest: u32,
    pub r#where: u32,
    pub faces: u32,
}
/// a field's entry, and `vx_distance_info::farthest`, when the box holds no target (the header's value, written in hexadecimal as there)
pub const VX_DISTANCE_NONE: u16 = 0xFFFF;
/// `vx_distance_shape::flags`: the target set is complemented within the box
pub const VX_DISTANCE_TO_AIR: u32 = 0x1;

#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct vx_stats {
    pub used_bytes: u64,
    pub capacity_bytes: u64,
    pub depth: u32,
}

#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct vx_target {
    pub rgba32f: *mut c_void,
    pub hits: *mut vx_hit,
    pub memory: i32,
    pub tile_rank: u32,
    pub tile_count: u32,
    pub format: i32,
}

const _: () = assert!(std::mem::size_of::<vx_range>() == 16);
const _: () = assert!(std::mem::size_of::<vx_uniforms>() == 4 * (16 + 3 + 3 + 3 + 1 + 1 + 3));
const _: () = assert!(std::mem::size_of::<vx_hit>() == 48);
const _: () = assert!(std::mem::size_of::<vx_entity>() == 64);
const _: () = assert!(std::mem::size_of::<vx_aabb_result>() == 24);
const _: () = assert!(std::mem::size_of::<vx_ray_batch>() == 48);
const _: () = assert!(std::mem::size_of::<vx_ray_hit>() == 32);
const _: () = assert!(std::mem::size_of::<vx_block_cell>() == 8);
const _: () = assert!(std::mem::size_of::<vx_block_at>() == 8);
const _: () = assert!(std::mem::size_of::<vx_scan_hit>() == 16);
const _: () = assert!(std::mem::size_of::<vx_box_batch>() == 40);
const _: () = assert!(std::mem::size_of::<vx_box_hit>() == 32);
const _: () = assert!(std::mem::size_of::<vx_move_shape>() == 16);
const _: () = assert!(std::mem::size_of::<vx_move_hit>() == 48);
const _: () = assert!(std::mem::size_of::<vx_flood_shape>() == 36);
const _: () = assert!(std::mem::size_of::<vx_flood_info>() == 16);
const _: () = assert!(std::mem::size_of::<vx_light_shape>() == 32);
const _: () = assert!(std::mem::size_of::<vx_light_info>() == 16);
const _: () = assert!(std::mem::size_of::<vx_walk_shape>() == 52);
const _: () = assert!(std::mem::size_of::<vx_walk_info>() == 32);
const _: () = assert!(std::mem::size_of::<vx_label_shape>() == 32);
const _: () = assert!(std::mem::size_of::<vx_label_piece>() == 16);
const _: () = assert!(std::mem::size_of::<vx_label_info>() == 32);
const _: () = assert!(std::mem::size_of::<vx_distance_shape>() == 32);
const _: () = assert!(std::mem::size_of::<vx_distance_info>() == 16);
const _: () = assert!(std::mem::size_of::<MaterialInstance>() == 32); // svo_registry.rs:29-40 is #[repr(C)]
const _: () = assert!(std::mem::size_of::<PickerTask>() == 48 && std::mem::size_of::<PickerResult>() == 48); // svo_picker.rs:13-32

extern "C" {
    // ---- lifetime (Svo::new, Drop) ------------------------------------------------------------------------------------
    pub fn vx_create(svo_type: c_int, capacity_bytes: usize, device: c_int, out: *mut *mut vx_context) -> c_int;
    pub fn vx_destroy(ctx: *mut vx_context);
    // ---- resources (VoxelRegistry::build_material_buffer, TextureArrayBuilder::build) ---------------------------------------
    pub fn vx_set_materials(ctx: *mut vx_context, rows: *const MaterialInstance, count: u32) -> c_int;
    pub fn vx_set_textures(ctx: *mut vx_context, rgba8: *const u8, width: u32, height: u32, layers: u32, mip_levels: u32) -> c_int;
    // ---- SVO upload (Svo::update) ---------------------------------------------------------------------------------------
    pub fn vx_staging_ptr(ctx: *mut vx_context) -> *mut u8;
    pub fn vx_capacity(ctx: *const vx_context) -> usize;
    pub fn vx_arena_capacity(ctx: *const vx_context) -> usize;
    pub fn vx_commit(ctx: *mut vx_context, depth: u32, ranges: *const vx_range, count: u32, used_bytes: u64) -> c_int;
    pub fn vx_commit_all(ctx: *mut vx_context, depth: u32, used_bytes: u64) -> c_int;
    /// VX_COMMIT_INLINE = 0, VX_COMMIT_PIPELINED = 1 (a worker thread of the context does the image update and the uploads)
    pub fn vx_set_commit_mode(ctx: *mut vx_context, mode: c_int) -> c_int;
    pub fn vx_commit_wait(ctx: *mut vx_context) -> c_int;
    pub fn vx_get_stats(ctx: *const vx_context, out: *mut vx_stats) -> c_int;
    // ---- the hot path (Svo::render, Svo::raycast) ---------------------------------------------------------------------------
    pub fn vx_render(ctx: *mut vx_context, uniforms: *const vx_uniforms, width: u32, height: u32, target: *const vx_target) -> c_int;
    pub fn vx_raycast(ctx: *mut vx_context, tasks: *const PickerTask, count: u32, results: *mut PickerResult) -> c_int;
    /// picker.glsl for `count` plain rays (PickerBatch::add_ray) read through the strides of `rays`; `memory`: VX_MEM_HOST / VX_MEM_DEVICE
    pub fn vx_raycast_batch(ctx: *mut vx_context, rays: *const vx_ray_batch, count: u32, memory: c_int, hits: *mut vx_ray_hit) -> c_int;
    /// world.glsl:27-108,132-138 (trace_ray, or the sky) for `count` rays read through the strides of `rays`: `count` pixels in `format` to `rgba`
    /// and / or `count` vx_hit records to `hits` (either may be null, not both); `memory`: VX_MEM_HOST / VX_MEM_DEVICE
    pub fn vx_trace_rays(ctx: *mut vx_context, uniforms: *const vx_uniforms, rays: *const vx_ray_batch, count: u32, memory: c_int, rgba: *mut c_void,
                         format: c_int, hits: *mut vx_hit) -> c_int;
    /// world.glsl:110-141 (main) for every pixel of `count` views of width x height in one launch; `views`: host memory always; view k's pixels
    /// (in `format`) and vx_hit records at index k * width * height of `rgba` / `hits` (either may be null, not both); `memory` (of the outputs):
    /// VX_MEM_HOST / VX_MEM_DEVICE
    pub fn vx_trace_views(ctx: *mut vx_context, views: *const vx_uniforms, count: u32, width: u32, height: u32, memory: c_int, rgba: *mut c_void,
                          format: c_int, hits: *mut vx_hit) -> c_int;
    /// get_block(floor(pos)) (gameplay.rs:161-201) asked of the world the device holds, for `count` positions (a float[3] at pos + i * pos_stride,
    /// e.g. inside vx_entity or vx_ray_hit records); `memory`: VX_MEM_HOST / VX_MEM_DEVICE
    pub fn vx_block_points(ctx: *mut vx_context, pos: *const c_void, pos_stride: u32, count: u32, memory: c_int, out: *mut vx_block_cell) -> c_int;
    /// the block ids of the box [lo, lo + size) as a dense array, x fastest, 0 outside the world; at most 2^24 voxels; `memory`: VX_MEM_HOST / VX_MEM_DEVICE
    pub fn vx_read_region(ctx: *mut vx_context, lo: *const [i32; 3], size: *const [u32; 3], memory: c_int, out: *mut u32) -> c_int;
    /// the blocks the box [lo, lo + size) holds as a compact list in a fixed order (brick by brick, dense-index order inside a brick), with the
    /// faces that touch air under `flags` (VX_LIST_*); `*total`: the records the box has, of which the first min(total, capacity) are written
    /// to `out` (capacity 0: only counted); `memory` (of `out` and `total`): VX_MEM_HOST / VX_MEM_DEVICE
    pub fn vx_list_region(ctx: *mut vx_context, lo: *const [i32; 3], size: *const [u32; 3], flags: u32, memory: c_int, out: *mut vx_block_at,
                          capacity: u32, total: *mut u32) -> c_int;
    /// the first block from floor(pos) on along `direction` (VX_DIR_*), at most `reach` voxels on (the start counts; VX_SCAN_TO_EDGE: to the
    /// world's edge), for `count` positions read as vx_block_points reads them; `memory`: VX_MEM_HOST / VX_MEM_DEVICE
    pub fn vx_scan_points(ctx: *mut vx_context, pos: *const c_void, pos_stride: u32, count: u32, direction: c_int, reach: u32, memory: c_int,
                          out: *mut vx_scan_hit) -> c_int;
    /// the same scan for every column of the box [lo, lo + size) across the axis of `direction`, from the face it enters, as a dense array
    /// [v - lo[v]][u - lo[u]] (u < v the two other axes; VX_DIR_NEG_Y: a heightmap [z][x]); `memory`: VX_MEM_HOST / VX_MEM_DEVICE
    pub fn vx_scan_columns(ctx: *mut vx_context, lo: *const [i32; 3], size: *const [u32; 3], direction: c_int, memory: c_int, out: *mut vx_scan_hit) -> c_int;
    /// what each of `count` float boxes (`vx_box_batch`) holds: how many voxels of its cover hold a block (`only_value`: of that id), the first
    /// of them, their bounds; a record that is no box gives `VX_BOX_INVALID`; `memory`: VX_MEM_HOST / VX_MEM_DEVICE (`out` aligned to 16 bytes)
    pub fn vx_overlap_boxes(ctx: *mut vx_context, boxes: *const vx_box_batch, count: u32, memory: c_int, out: *mut vx_box_hit) -> c_int;
    /// each of `count` float boxes (`vx_box_batch`) moved by its motion (a float[3] at motion + i * motion_stride, 0 = one for all) times
    /// `shape.scale`, axis by axis in `shape.order`, stopped `shape.skin` short of the first counted voxel ahead of its leading face; a record
    /// that is no box or has no finite motion of at most `VX_MOVE_MAX_TRAVEL` gives `VX_MOVE_INVALID`; `memory`: VX_MEM_HOST / VX_MEM_DEVICE
    /// (`out` aligned to 16 bytes)
    pub fn vx_move_boxes(ctx: *mut vx_context, boxes: *const vx_box_batch, motion: *const c_void, motion_stride: u32, count: u32,
                         shape: *const vx_move_shape, memory: c_int, out: *mut vx_move_hit) -> c_int;
    /// step distances through air around each of `count` positions (read as `vx_block_points` reads them): a breadth-first flood of the box
    /// `shape` describes; query k's field -- a byte a cell, x fastest -- at fields + k * field_stride (a multiple of 16, 0 = the voxel count
    /// rounded up to 16), its record at info[k]; either output may be null, not both; `memory`: VX_MEM_HOST / VX_MEM_DEVICE (both aligned to 16)
    pub fn vx_flood_points(ctx: *mut vx_context, pos: *const c_void, pos_stride: u32, count: u32, shape: *const vx_flood_shape, memory: c_int,
                           fields: *mut u8, field_stride: u32, info: *mut vx_flood_info) -> c_int;
    /// sky and block light levels (0..15 each, sky << 4 | block a cell, x fastest) of the boxes [lo_k, lo_k + shape.size), lo_k an int32[3]
    /// at lo + k * lo_stride; box k's field at fields + k * field_stride (a multiple of 16, 0 = the voxel count rounded up to 16), its record
    /// at info[k]; either output may be null, not both; `memory`: VX_MEM_HOST / VX_MEM_DEVICE (both aligned to 16); props is host memory
    pub fn vx_light_boxes(ctx: *mut vx_context, lo: *const c_void, lo_stride: u32, count: u32, shape: *const vx_light_shape, memory: c_int,
                          fields: *mut u8, field_stride: u32, info: *mut vx_light_info) -> c_int;
    /// walking distances and paths for ground agents around each of `count` positions (read as `vx_block_points` reads them; `goal`: null, or a
    /// float[3] at goal + k * goal_stride, a goal_stride of 0 meaning one goal for all): breadth-first step counts over the walking graph of the
    /// box `shape` describes -- a floor below, `height` cells of headroom, one block up, `drop` down; query k's field -- a byte a cell, x fastest --
    /// at fields + k * field_stride (a multiple of 16, 0 = the voxel count rounded up to 16), its path -- `path_capacity` cells as rx | ry << 8 |
    /// rz << 16, VX_WALK_NONE beyond its end -- at paths + k * path_capacity, its record at info[k]; any output may be null, not all; `memory`:
    /// VX_MEM_HOST / VX_MEM_DEVICE (all three aligned to 16)
    pub fn vx_walk_points(ctx: *mut vx_context, pos: *const c_void, pos_stride: u32, goal: *const c_void, goal_stride: u32, count: u32,
                          shape: *const vx_walk_shape, memory: c_int, fields: *mut u8, field_stride: u32, paths: *mut u32, info: *mut vx_walk_info) -> c_int;
    /// the loose pieces of the solid cells of the boxes [lo_k, lo_k + shape.size), lo_k an int32[3] at lo + k * lo_stride: held from the anchor
    /// faces, then labelled 1, 2, ... in the field's order within the step budget; box k's field (a byte a cell, x fastest) at fields + k *
    /// field_stride (a multiple of 16, 0 = the voxel count rounded up to 16), its shape.max_pieces piece records at pieces + k *
    /// shape.max_pieces, its record at info[k]; any output may be null, not all; `memory`: VX_MEM_HOST / VX_MEM_DEVICE (all three aligned to 16)
    pub fn vx_label_boxes(ctx: *mut vx_context, lo: *const c_void, lo_stride: u32, count: u32, shape: *const vx_label_shape, memory: c_int,
                          fields: *mut u8, field_stride: u32, pieces: *mut vx_label_piece, info: *mut vx_label_info) -> c_int;
    /// the squared distance from every cell of the boxes [lo_k, lo_k + shape.size), lo_k an int32[3] at lo + k * lo_stride, to the nearest target
    /// cell of the box; box k's field (a u16 a cell, x fastest, VX_DISTANCE_NONE without a target) at fields + k * field_stride BYTES (a multiple of
    /// 16, 0 = twice the voxel count rounded up to 16), its record at info[k]; either output may be null, not both; `memory`: VX_MEM_HOST /
    /// VX_MEM_DEVICE (both aligned to 16)
    pub fn vx_distance_boxes(ctx: *mut vx_context, lo: *const c_void, lo_stride: u32, count: u32, shape: *const vx_distance_shape, memory: c_int,
                             fields: *mut c_void, field_stride: u32, info: *mut vx_distance_info) -> c_int;
    /// Physics::step_many (physics.rs:122-136) `steps` times for `count` entities in one launch; `memory`: VX_MEM_HOST / VX_MEM_DEVICE
    pub fn vx_physics_step(ctx: *mut vx_context, entities: *mut vx_entity, count: u32, memory: c_int, delta_time: f32, steps: u32,
                           contacts: *mut vx_aabb_result) -> c_int;
    pub fn vx_sync(ctx: *mut vx_context) -> c_int;
    pub fn vx_set_frames_in_flight(ctx: *mut vx_context, frames: c_int) -> c_int;
    pub fn vx_wait_event(ctx: *mut vx_context, hip_event: *mut c_void) -> c_int;
    pub fn vx_stream_wait_render(ctx: *mut vx_context, stream: *mut c_void) -> c_int;
    // ---- pipelined presentation (render + blit_to_default, world.rs:269-283) ------------------------------------------------
    pub fn vx_present_begin(ctx: *mut vx_context, uniforms: *const vx_uniforms, width: u32, height: u32, format: c_int, out_slot: *mut c_int) -> c_int;
    pub fn vx_present_wait(ctx: *mut vx_context, slot: c_int, pixels: *mut *const c_void, bytes: *mut usize) -> c_int;
    // ---- multi-GPU: one process per GPU, screen tiles, RCCL gather --------------------------------------------------------------
    pub fn vx_tile_order(width: u32, height: u32, out: *mut u32, capacity: u32) -> u32;
    pub fn vx_local_tile_count(width: u32, height: u32, tile_rank: u32, tile_count: u32) -> u32;
    pub fn vx_comm_library(path: *const c_char) -> c_int;
    pub fn vx_comm_unique_id(out_id: *mut c_void, bytes: usize) -> c_int;
    pub fn vx_comm_init(ctx: *mut vx_context, nranks: c_int, rank: c_int, unique_id: *const c_void) -> c_int;
    pub fn vx_comm_destroy(ctx: *mut vx_context) -> c_int;
    pub fn vx_comm_info(ctx: *const vx_context, nranks: *mut c_int, rank: *mut c_int) -> c_int;
    pub fn vx_set_comm_headroom(ctx: *mut vx_context, waves_per_cu: c_int) -> c_int;
    pub fn vx_gather_tiles(ctx: *mut vx_context, tiles: *const c_void, bytes_per_rank: u64, gathered: *mut c_void, root: c_int, out_ticket: *mut c_int) -> c_int;
    pub fn vx_wait_gather(ctx: *mut vx_context, ticket: c_int) -> c_int;
    pub fn vx_gather_query(ctx: *mut vx_context, ticket: c_int) -> c_int;
    pub fn vx_render_gather(ctx: *mut vx_context, uniforms: *const vx_uniforms, width: u32, height: u32, target: *const vx_target, bytes_per_rank: u64,
                            gathered: *mut c_void, root: c_int, image: *mut c_void, wait_ticket: c_int, out_ticket: *mut c_int) -> c_int;
    pub fn vx_comm_stream(ctx: *mut vx_context) -> *mut c_void;
    pub fn vx_assemble_tiles(ctx: *mut vx_context, tiles: *const f32, stride_floats: u64, tile_count: u32, width: u32, height: u32, out_rgba32f: *mut f32) -> c_int;
    pub fn vx_assemble_tiles_format(ctx: *mut vx_context, tiles: *const c_void, stride_pixels: u64, tile_count: u32, width: u32, height: u32, out: *mut c_void,
                                    format: c_int, stream: *mut c_void) -> c_int;
    pub fn vx_resolve_2x2(ctx: *mut vx_context, src_rgba32f: *const f32, width: u32, height: u32, dst_rgba32f: *mut f32, stream: *mut c_void) -> c_int;
    // ---- diagnostics ------------------------------------------------------------------------------------------------------
    pub fn vx_image_info(ctx: *const vx_context, out: *mut [u64; 4]) -> c_int;
    pub fn vx_stream(ctx: *mut vx_context) -> *mut c_void;
    pub fn vx_device(ctx: *const vx_context) -> c_int;
    pub fn vx_last_error() -> *const c_char;
    pub fn vx_version() -> *const c_char;
}

/// `vx_last_error()` as a `String`.
pub fn last_error() -> String {
    unsafe { std::ffi::CStr::from_ptr(vx_last_error()) }.to_string_lossy().into_owned()
}

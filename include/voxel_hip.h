/* voxel_hip.h -- C ABI of libvoxelhip.so: the MI355X (gfx950) drop-in for voxel-rs's `graphics::Svo`.
 *
 * Every entry point replaces one piece of the reference's OpenGL render/raycast surface
 * (/root/reference/src/graphics/svo.rs); the citation next to each declaration names it. All positions are in
 * SVO space [0, 2^depth) exactly as `graphics::Svo` expects (svo.rs:55); world<->SVO conversion stays with the
 * caller (src/systems/worldsvo.rs:397-435). Single caller thread per context, like the reference (svo.rs:56-73
 * holds RefCell'd GL state). No exceptions cross this boundary: functions return a vx_status, details via
 * vx_last_error(). Plain pointers and sizes only.
 *
 * The reference-side binding (Rust `extern "C"` block + safe wrapper) is shown in INTEGRATION.md.
 */
#ifndef VOXEL_HIP_H
#define VOXEL_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* SvoType (svo.rs:18-39): the values are the reference's shader defines SVO_TYPE_ESVO / SVO_TYPE_CSVO
 * (assets/shaders/svo.glsl:65-66). */
#define VX_SVO_ESVO 1
#define VX_SVO_CSVO 2

typedef enum vx_status {
    VX_OK = 0,
    VX_ERR_INVALID_ARGUMENT = 1,
    VX_ERR_NO_DEVICE = 2,      /* no usable HIP device: there is NO CPU fallback */
    VX_ERR_OUT_OF_MEMORY = 3,
    VX_ERR_CAPACITY = 4,       /* a range does not fit the world buffer (reference: assert!, esvo.rs:328 / csvo.rs:301) */
    VX_ERR_HIP = 5,            /* a HIP runtime call failed */
    VX_ERR_STATE = 6           /* e.g. render before any commit */
} vx_status;

typedef enum vx_memory { VX_MEM_HOST = 0, VX_MEM_DEVICE = 1 } vx_memory;
/* Pixel format of a render target. RGBA32F is the reference's framebuffer (the image2D of world.glsl:10, row 0 = bottom); RGBA8 is
 * what Framebuffer::as_image reads back from it (src/graphics/framebuffer.rs:97-111): glReadPixels(RGBA, UNSIGNED_BYTE) -- clamp
 * to [0,1], round to the nearest of 255 steps, NaN -> 0 -- flipped vertically, so a whole image has its TOP row first. A quarter
 * of the bytes for a presenting embedder's read-back and for the multi-GPU gather. */
typedef enum vx_format { VX_FORMAT_RGBA32F = 0, VX_FORMAT_RGBA8 = 1 } vx_format;
/* What "identical to the reference" means for a pixel. Everything a ray's PATH depends on -- every traversal float (t, position, uv,
 * the per-iteration t_min), hit identity, flags, step counts, and the shadow ray's origin and with it the normal-mapped normal -- is
 * bit for bit the reference's arithmetic (fp32, no contraction, explicit fma where the shader says so, IEEE division and square root).
 * The COLOUR of a pixel agrees with the CPU restatement of the shaders to 5e-6 absolute, for four stated reasons, all colour-only:
 *   - pow() of the specular term is exp2(y * log2(x)) on the hardware's 1-ulp v_exp_f32 / v_log_f32 (GLSL's own definition) instead of a
 *     correctly rounded powf: within 1.2e-7 absolute on its domain;
 *   - acos() of the sky gradient is a degree-7 polynomial (Abramowitz & Stegun 4.4.46): 4.3e-7 rad;
 *   - acos' argument is clamped to [-1, 1] (world.glsl:98 does not; the reference's expected image shows no undefined horizon pixels).
 *     The restatement clamps too, so only the comparison with the reference's own PNG (tests/test_render_png.py, 1e-3) can see this one;
 *   - the four texels of a bilinear tap are blended in byte units and the common 1/255 applied once (< 4e-7; > 0 in exactly the same
 *     cases, so the alpha test that decides a hit is unaffected). */

typedef struct vx_context vx_context; /* replaces `struct Svo` (svo.rs:56-73): owns every device object */

/* MaterialInstance, 32-byte rows indexed by BlockId (src/graphics/svo_registry.rs:29-40; svo.glsl:48-59).
 * Texture fields are array layers, -1 = none. */
typedef struct vx_material {
    float specular_pow, specular_strength;
    int32_t tex_top, tex_side, tex_bottom;
    int32_t tex_top_normal, tex_side_normal, tex_bottom_normal;
} vx_material;

/* One dirty range of the serialized SVO arena, in the coordinates of the reference's
 * `RangeBuffer::updated_ranges` (src/world/hds/internal.rs:151-154,166): byte offsets relative to the
 * first byte AFTER the writer's header (ESVO: 20-byte preamble, esvo.rs:179-188; CSVO: 4-byte root pointer,
 * csvo.rs:291-292). */
typedef struct vx_range {
    uint64_t start, length;
} vx_range;

/* The uniforms `Svo::render` sets on world.glsl (svo.rs:201-215; assets/shaders/world.glsl:12-25).
 * `view` is u_view = look_to_rh(cam_pos, cam_fwd, cam_up)^-1, column-major (svo.rs:197).
 * highlight_pos = NaN when nothing is selected (svo.rs:211). light_dir must be normalised by the caller
 * (src/gamelogic/world.rs:106). */
typedef struct vx_uniforms {
    float view[16];
    float fovy, aspect;
    float ambient;
    float light_dir[3];
    float cam_pos[3];
    int32_t render_shadows;
    float shadow_distance;
    float highlight_pos[3];
} vx_uniforms;

/* PickerTask / PickerResult with the std430 layout of assets/shaders/picker.glsl:9-27
 * (src/graphics/svo_picker.rs:13-32): 48 bytes each, vec3s at 16 and 32. */
typedef struct vx_picker_task {
    float max_dst, _pad0[3];
    float pos[3], _pad1;
    float dir[3], _pad2;
} vx_picker_task;

typedef struct vx_picker_result {
    float dst;             /* -1 = no hit */
    uint32_t inside_voxel; /* GLSL bool */
    float _pad0[2];
    float pos[3], _pad1;
    float normal[3], _pad2;
} vx_picker_result;

/* An entity as systems::Physics steps it (src/systems/physics.rs:10-75: the fields Physics::update_entity reads and writes,
 * physics.rs:139-170); 64 bytes. Positions in SVO space like everything else here. */
typedef struct vx_entity {
    float position[3];
    float velocity[3];
    float aabb_offset[3];   /* AABBDef (physics.rs:77-87): the box spans position + offset .. position + offset + extents */
    float aabb_extents[3];
    float gravity, max_fall_velocity; /* EntityCapabilities (physics.rs:36-57) */
    uint32_t flags;     /* bit0 wall_clip, bit1 flying */
    uint32_t grounded;  /* out: EntityState::is_grounded (physics.rs:30-34) after the last step */
} vx_entity;
#define VX_ENTITY_WALL_CLIP 1
#define VX_ENTITY_FLYING 2

/* AabbResult (src/graphics/svo_picker.rs:163-176): shortest hit distance of a box's ray fan per axis, in negative and in positive
 * direction, -1 = none; 24 bytes. */
typedef struct vx_aabb_result {
    float neg[3];
    float pos[3];
} vx_aabb_result;

/* A batch of rays read where they already lie (vx_raycast_batch). Every pointer is in the memory kind given to the call. Strides are in
 * bytes and are multiples of 4; a float[3] is read at origin + i*origin_stride (stride >= 12), at dir + i*dir_stride (stride >= 12, or
 * 0 = one direction for every ray); max_dst: NULL = max_dst_all for every ray, else a float at max_dst + i*max_dst_stride (stride >= 4,
 * or 0 = that one float for every ray). */
typedef struct vx_ray_batch {
    const void* origin;
    const void* dir;
    const void* max_dst;
    uint32_t origin_stride, dir_stride, max_dst_stride;
    float max_dst_all;
    uint32_t flags;               /* VX_RAYS_TRANSLUCENT: intersect_octree's cast_translucent = true (picker.glsl passes false) */
} vx_ray_batch;
#define VX_RAYS_TRANSLUCENT 1

/* What a ray of a batch found: PickerResult (svo_picker.rs:24-32) with the block id kept and the normal as its face; 32 bytes. */
typedef struct vx_ray_hit {
    float dst;                    /* -1 = no hit: every other field 0 then */
    uint32_t value;               /* BlockId of the voxel hit (OctreeResult.value, svo.glsl:31-40) */
    int32_t face_id;              /* 0..5 = -x,+x,-y,+y,-z,+z: the picker's normal is this face's */
    uint32_t inside_voxel;
    float pos[3];
    uint32_t _pad;                /* written 0 */
} vx_ray_hit;

/* The leaf (or the empty cell) that holds a point (vx_block_points); 8 bytes. */
typedef struct vx_block_cell {
    uint32_t value;               /* BlockId stored in the leaf whose cell contains floor(p); 0 = no block there */
    uint32_t cell_log2;           /* the answering cell is the cube of side 2^cell_log2 aligned to its size that contains floor(p): 0 for a
                                     full-detail block, 2 for a voxel of a LOD-3 chunk, and for value 0 the size of the empty cell at which
                                     the descent ended; VX_CELL_OUTSIDE for a point outside [0, 2^depth)^3 */
} vx_block_cell;
#define VX_CELL_OUTSIDE 0xFFFFFFFFu

/* directions of travel of a scan (vx_scan_points, vx_scan_columns), numbered like face_id */
#define VX_DIR_NEG_X 0
#define VX_DIR_POS_X 1
#define VX_DIR_NEG_Y 2            /* downwards: a heightmap */
#define VX_DIR_POS_Y 3
#define VX_DIR_NEG_Z 4
#define VX_DIR_POS_Z 5
#define VX_SCAN_NONE ((int32_t)0x80000000) /* vx_scan_hit.coord when no block was found */
#define VX_SCAN_TO_EDGE 0xFFFFFFFFu        /* reach: as far as the world goes */

/* The first voxel holding a block along an axis (vx_scan_points, vx_scan_columns); 16 bytes. */
typedef struct vx_scan_hit {
    int32_t coord;                /* its coordinate ALONG THE SCAN AXIS (the other two are the column's); VX_SCAN_NONE: none */
    uint32_t value;               /* its BlockId; 0 = none */
    uint32_t cell_log2;           /* the answering leaf is the aligned cube of side 2^cell_log2 holding that voxel (0 full detail, 2 a voxel
                                     of a LOD-3 chunk, ...); 0 for none; VX_CELL_OUTSIDE for a position that is no position (a NaN or
                                     infinite component; points only) */
    uint32_t _pad;                /* written 0 */
} vx_scan_hit;

/* A batch of axis-aligned boxes read where they lie (vx_overlap_boxes). Box i spans, per axis, [mn, mx) with
 *   mn = origin[i] + offset[i]   (one fp32 add; offset == NULL: mn = origin[i])
 *   mx = mn + extents[i]         (one fp32 add)
 * -- the order of gameplay.rs:212-217 and of the physics fan (physics.rs / svo_picker.rs:183-243), so a vx_entity record is read in
 * place: origin = &e[0].position, offset = &e[0].aabb_offset, extents = &e[0].aabb_extents, all three strides 64.
 * Every pointer 4-byte aligned, in the memory kind given to the call; strides in bytes, multiples of 4; origin_stride >= 12; offset_stride
 * and extents_stride >= 12, or 0 = that one vector for every box. */
typedef struct vx_box_batch {
    const void* origin;
    const void* offset;    /* may be NULL */
    const void* extents;
    uint32_t origin_stride, offset_stride, extents_stride;
    uint32_t only_value;   /* 0: every block counts; else only voxels whose BlockId equals it (water, lava, a ladder) */
} vx_box_batch;

#define VX_BOX_INVALID 0xFFFFFFFFu
/* What a box holds (vx_overlap_boxes); 32 bytes. */
typedef struct vx_box_hit {
    uint32_t blocks;   /* voxels of the box's cover that hold a (counted) block; VX_BOX_INVALID: the record described no box */
    uint32_t value;    /* BlockId of the first of them in vx_read_region's order (z, then y, then x ascending); 0 = none */
    int32_t lo[3];     /* the bounds of those voxels in SVO coordinates, [lo, hi); all 0 when blocks is 0 or VX_BOX_INVALID */
    int32_t hi[3];
} vx_box_hit;

#define VX_MOVE_INVALID   0xFFFFFFFFu
#define VX_MOVE_MAX_TRAVEL 64.0f
#define VX_MOVE_ORDER_YXZ 0x21u   /* axis of pass 0 | pass 1 << 2 | pass 2 << 4: y, then x, then z */
/* What every box of a vx_move_boxes call shares; read on the host during the call. */
typedef struct vx_move_shape {
    float scale;      /* displacement = motion * scale, one fp32 multiply a component (vx_entity.velocity in place, scale = delta_time) */
    float skin;       /* finite, 0 <= skin <= 1: the gap a stopped box keeps from the block that stopped it */
    uint32_t order;   /* a permutation of the axes 0, 1, 2 in bits 0..1, 2..3, 4..5; every other bit 0 */
    uint32_t flags;   /* 0 */
} vx_move_shape;
/* How far a box got (vx_move_boxes); 48 bytes. */
typedef struct vx_move_hit {
    float origin[3];    /* the box's origin after the move */
    float moved[3];     /* what was added to it, per axis */
    uint32_t contacts;  /* bit 2a + (d_a > 0): a block was found ahead of that side of the box within the scan's range (numbered like
                           face_id); VX_MOVE_INVALID: the record described no box, or no motion */
    uint32_t value[3];  /* per axis the BlockId of the stopping voxel, 0 = none */
    uint32_t _pad[2];   /* written 0 */
} vx_move_hit;

#define VX_FLOOD_MAX_STEPS   250u
#define VX_FLOOD_NO_POSITION 0xFDu   /* every byte of a field whose position is no position */
#define VX_FLOOD_UNREACHED   0xFEu   /* passable, not reached within max_steps */
#define VX_FLOOD_BLOCKED     0xFFu   /* not passable */
#define VX_FLOOD_SEED_ALWAYS 1u      /* the seed cell is step 0 and spreads even if it holds a block (a lamp is a block) */
#define VX_FLOOD_INVALID     0xFFFFFFFFu
/* What every query of a vx_flood_points call shares; read on the host during the call. */
typedef struct vx_flood_shape {
    uint32_t size[3];      /* the box of each query, 1..32 an axis */
    uint32_t seed_at[3];   /* the seed's cell inside the box, < size: lo = floor(p) - seed_at */
    uint32_t max_steps;    /* 0..VX_FLOOD_MAX_STEPS */
    uint32_t pass_value;   /* 0: only air passes; else voxels with this BlockId pass too (water) */
    uint32_t flags;        /* 0 or VX_FLOOD_SEED_ALWAYS */
} vx_flood_shape;
/* What a flood reached (vx_flood_points); 16 bytes. */
typedef struct vx_flood_info {
    uint32_t reached;      /* cells with a step count (the seed included); VX_FLOOD_INVALID: no position */
    uint32_t farthest;     /* the largest step count; 0 when reached <= 1 */
    uint32_t faces;        /* bit f (numbered like face_id) set when a reached cell lies on that face of the box: 0 = the flood is
                              enclosed within the box */
    uint32_t seed_value;   /* vx_block_points' value at the seed cell */
} vx_flood_info;

#define VX_LIGHT_MAX_SIDE    48u
#define VX_LIGHT_MAX_PROPS   4096u
#define VX_LIGHT_TRANSPARENT 0x10u   /* props bit 4: light passes through this block */
#define VX_LIGHT_NO_SKY      1u      /* flags: leave the sky channel (the high nibble) 0 and scan no column */
#define VX_LIGHT_NO_BLOCKS   2u      /* flags: leave the block channel (the low nibble) 0 */
#define VX_LIGHT_INVALID     0xFFFFFFFFu
/* What every query of a vx_light_boxes call shares; read on the host during the call. */
typedef struct vx_light_shape {
    uint32_t size[3];        /* the box of each query, 1..VX_LIGHT_MAX_SIDE an axis */
    uint32_t flags;          /* 0, VX_LIGHT_NO_SKY or VX_LIGHT_NO_BLOCKS; not both */
    const uint8_t* props;    /* HOST memory whatever `memory` says: props[id] = emission (bits 0..3) | VX_LIGHT_TRANSPARENT; bits 5..7 must be 0 */
    uint32_t props_count;    /* 0..VX_LIGHT_MAX_PROPS; ids at or above it: opaque, emit nothing. props[0] is ignored: air passes light and emits
                                none */
} vx_light_shape;
/* What the light of a box amounts to (vx_light_boxes); 16 bytes. */
typedef struct vx_light_info {
    uint32_t lit;            /* cells whose byte is not 0 */
    uint32_t sources;        /* cells of the box whose block emits (emission > 0); 0 under VX_LIGHT_NO_BLOCKS */
    uint32_t open_columns;   /* columns (x, z) of the box whose TOP cell is exposed to the sky; 0 under VX_LIGHT_NO_SKY */
    uint32_t faces;          /* bit f (numbered like face_id) set when a cell on that face of the box has a level >= 2 in either channel:
                                light that would go on beyond the box */
} vx_light_info;

#define VX_WALK_MAX_STEPS   250u
#define VX_WALK_NO_POSITION 0xFDu   /* every byte of a field whose position is no position */
#define VX_WALK_UNREACHED   0xFEu   /* standable, not reached within max_steps */
#define VX_WALK_NO_STAND    0xFFu   /* the agent cannot stand here */
#define VX_WALK_STOP_AT_GOAL 1u     /* flags: the flood ends after the whole step that reaches the settled goal */
#define VX_WALK_NONE        0xFFFFFFFFu
/* What every query of a vx_walk_points call shares; read on the host during the call. */
typedef struct vx_walk_shape {
    uint32_t size[3];        /* the box of each query; 1..32 on x and z; size[1] >= 1 and size[1] + height <= 32 */
    uint32_t seed_at[3];     /* < size: lo = floor(p) - seed_at, as in vx_flood_shape */
    uint32_t max_steps;      /* 0..VX_WALK_MAX_STEPS */
    uint32_t pass_value;     /* as vx_flood_shape's: this id passes like air (and, like air, is no floor) */
    uint32_t height;         /* 1..4 cells of headroom the agent needs */
    uint32_t climb;          /* 0 or 1: the step up it can take */
    uint32_t drop;           /* 0..3: the most it steps down */
    uint32_t path_capacity;  /* 0..252, a multiple of 4: entries of a query's path */
    uint32_t flags;          /* 0 or VX_WALK_STOP_AT_GOAL */
} vx_walk_shape;
/* What a walk reached (vx_walk_points); 32 bytes, two 16-byte stores. */
typedef struct vx_walk_info {
    uint32_t reached, farthest, faces, seed_value;   /* as vx_flood_info, over standable cells */
    uint32_t start_ry;       /* y, inside the box, of the cell the seed settled on; VX_WALK_NONE: it stands nowhere */
    uint32_t goal_ry;        /* the same for the goal; VX_WALK_NONE: no goal given, no position, outside the box, or it stands nowhere */
    uint32_t path_steps;     /* step count of the settled goal; VX_WALK_NONE when goal_ry is, or the goal was not reached */
    uint32_t _pad;           /* written 0 */
} vx_walk_info;

#define VX_LABEL_MAX_PIECES 250u
#define VX_LABEL_MAX_STEPS  4096u
#define VX_LABEL_AIR   0x00u   /* not solid */
#define VX_LABEL_MORE  0xFEu   /* solid, neither held nor one of the labelled pieces */
#define VX_LABEL_HELD  0xFFu   /* solid, connected to an anchor face through solid cells of the box */
#define VX_LABEL_ALL_FACES 0x3Fu
#define VX_LABEL_CUT   1u      /* vx_label_info.flags: the step budget ran out */
/* What every query of a vx_label_boxes call shares; 32 bytes; read on the host during the call. */
typedef struct vx_label_shape {
    uint32_t size[3];        /* the box of each query, 1..32 an axis */
    uint32_t anchor_faces;   /* bits 0..5, numbered like vx_flood_info.faces (-x, +x, -y, +y, -z, +z): a solid cell on such a face of the box
                                is held */
    uint32_t max_pieces;     /* 0..VX_LABEL_MAX_PIECES */
    uint32_t max_steps;      /* 0..VX_LABEL_MAX_STEPS: the budget of all floods of a query together */
    uint32_t pass_value;     /* 0, or a BlockId that counts as air (vx_flood_shape's) */
    uint32_t flags;          /* 0 */
} vx_label_shape;
/* One loose piece of a box (vx_label_boxes); 16 bytes, one 16-byte store. */
typedef struct vx_label_piece {
    uint32_t cells;          /* 0: no such piece (then the whole record is 0) */
    uint32_t lo, hi;         /* the piece's bounds inside the box, rx | ry << 8 | rz << 16, both inclusive */
    uint32_t where;          /* its first cell, rx | ry << 8 | rz << 16, | faces << 24: bit f set when a cell of the piece lies on face f of
                                the box */
} vx_label_piece;
/* What the solid cells of a box fall into (vx_label_boxes); 32 bytes, two 16-byte stores. */
typedef struct vx_label_info {
    uint32_t solid, held, pieces, loose, more, steps, faces, flags;   /* cell counts: solid == held + loose + more; pieces: the labelled
                                pieces, loose their cells; steps: the budget used; faces: bit f set when a solid cell lies on face f of the
                                box; flags: 0 or VX_LABEL_CUT */
} vx_label_info;

#define VX_DISTANCE_NONE   0xFFFFu   /* a field's entry, and vx_distance_info.farthest: the box holds no target */
#define VX_DISTANCE_TO_AIR 1u        /* flags: the target set is complemented within the box */
/* What every query of a vx_distance_boxes call shares; 32 bytes; read on the host during the call. */
typedef struct vx_distance_shape {
    uint32_t size[3];        /* the box of each query, 1..32 an axis */
    uint32_t pass_value;     /* 0, or a BlockId that counts as air (vx_label_shape's); 0 with a match_value */
    uint32_t match_value;    /* 0: every solid cell is a target; else only the cells of this BlockId are */
    uint32_t flags;          /* 0 or VX_DISTANCE_TO_AIR */
    uint32_t _pad[2];        /* ignored */
} vx_distance_shape;
/* What the distances of a box amount to (vx_distance_boxes); 16 bytes, one 16-byte store. */
typedef struct vx_distance_info {
    uint32_t targets;        /* the number of target cells */
    uint32_t farthest;       /* the largest value of the field; VX_DISTANCE_NONE: no target */
    uint32_t where;          /* rx | ry << 8 | rz << 16 of the first cell in the field's order that holds `farthest`: the roomiest cell */
    uint32_t faces;          /* bit f set when a target lies on face f of the box, numbered like vx_flood_info.faces */
} vx_distance_info;

/* Optional per-pixel record of what trace_ray saw (world.glsl:27-90) -- the "hit position, depth" outputs
 * used for parity checks; not part of the reference's surface. */
typedef struct vx_hit {
    float t;          /* primary hit distance in SVO units, -1 = miss */
    uint32_t value;   /* BlockId of the hit voxel */
    int32_t face_id;  /* 0..5 = -x,+x,-y,+y,-z,+z */
    uint32_t flags;   /* bit0 hit, bit1 shadow ray cast, bit2 in shadow, bit3 highlight outline */
    float pos[3];
    float lod;
    float uv[2];
    float shadow_t;   /* hit distance of the shadow ray, -1 = unoccluded / not cast */
    uint32_t steps;   /* traversal loop iterations, primary + shadow */
} vx_hit;

/* OctreeResult and StackFrame of the debug harness (assets/shaders/svo.glsl:31-40, svo.test.glsl:13-33). */
typedef struct vx_result {
    float t;
    uint32_t value;
    int32_t face_id;
    float pos[3];
    float uv[2];
    float color[4];
    float lod;
    int32_t inside_voxel;
} vx_result;

typedef struct vx_frame {
    float t_min;
    uint32_t ptr, idx, parent_octant_idx; /* CSVO: 4th field = depth (svo.csvo.glsl:285) */
    int32_t scale, is_child, is_leaf, crossed_boundary;
    uint32_t next_ptr;
} vx_frame;

/* graphics::svo::Stats (svo.rs:75-83) */
typedef struct vx_stats {
    uint64_t used_bytes, capacity_bytes;
    uint32_t depth;
} vx_stats;

/* Step counters of the instrumented kernel variant (algorithmic-bytes model). */
typedef struct vx_counters {
    uint64_t rays, iterations, pushes, leaf_tests, leaf_tests_trilinear, boundaries;
    uint64_t csvo_header_bytes, csvo_pointer_bytes;
    uint64_t pixels, lit_pixels, shadow_rays;
    /* occupancy of the persistent wavefront kernel: trips of its traversal loop summed over waves (iterations / (64 *
     * wave_steps) = fraction of lanes traversing), service phases run, queue refills (0 for the per-pixel kernel) */
    uint64_t wave_steps, services, refills;
    /* the same after a wave found the queue empty (the frame's tail): loop trips and lane-iterations */
    uint64_t tail_wave_steps, tail_iterations;
} vx_counters;

/* Where vx_render writes. Tiles are 32x32 pixels; the image's tiles are taken in MORTON order of their (x, y) (vx_tile_order: any
 * run of consecutive places is a compact patch of the screen) and shared out round-robin: a context renders the tiles at the places
 * j with j % tile_count == tile_rank (multi-GPU screen sharding; 0/1 = whole image).
 *   tile_count <= 1: the target is width*height pixels -- RGBA32F: row 0 = bottom, the image2D of world.glsl:10; RGBA8: row 0 = top.
 *   tile_count  > 1: the target is a compact tile list: local tile k (the tile at place k*tile_count + tile_rank) occupies pixels
 *                    [k*1024, (k+1)*1024), pixel (x,y) of the tile (y counted from the bottom) at y*32+x.
 * hits (optional) uses the same indexing with vx_hit elements. */
typedef struct vx_target {
    void* rgba32f;  /* the pixels, in `format` */
    vx_hit* hits;
    int32_t memory; /* vx_memory of both pointers */
    uint32_t tile_rank, tile_count;
    int32_t format; /* vx_format; 0 = RGBA32F */
} vx_target;

/* ---- lifetime ------------------------------------------------------------------------------------------ */

/* Svo::new (svo.rs:109-149): capacity_bytes = size_mb * 1000 * 1000 of world buffer (svo.rs:133). Allocates
 * the pinned staging mirror, the device world buffer, streams and events on HIP device `device`. */
int vx_create(int svo_type, size_t capacity_bytes, int device, vx_context** out);
/* Drop for Svo (src/graphics/buffer.rs:41-47,95-101) */
void vx_destroy(vx_context* ctx);

/* ---- resources ------------------------------------------------------------------------------------------ */

/* VoxelRegistry::build_material_buffer (svo_registry.rs:135-165): rows indexed by BlockId. */
int vx_set_materials(vx_context* ctx, const vx_material* rows, uint32_t count);
/* TextureArrayBuilder::build + TextureArray::new (src/graphics/texture_array.rs:83-153,191-236): `rgba8` is
 * layers*height*width*4 bytes, base level only, ALREADY flipped vertically (row 0 = bottom, :92,126);
 * mip_levels is clamped to min(mip_levels, ilog2(min(w,h))) like :108 and the chain is generated here
 * (2x2 box filter, the glGenerateMipmap of :259). Sampler state is fixed to the reference's (:200-203). */
int vx_set_textures(vx_context* ctx, const uint8_t* rgba8, uint32_t width, uint32_t height, uint32_t layers, uint32_t mip_levels);

/* ---- SVO upload ------------------------------------------------------------------------------------------ */

/* MappedBuffer::cast / offset (svo.rs:175,181): host-pinned mirror of the world buffer, capacity_bytes long,
 * valid until vx_destroy. The caller's `WorldSvo::write_changes_to(ptr + 4, vx_arena_capacity(ctx), reset)` writes here
 * exactly as it writes into the mapped SSBO. */
uint8_t* vx_staging_ptr(vx_context* ctx);
size_t vx_capacity(const vx_context* ctx);
/* Bytes the serialized arena may take: vx_capacity() minus the 4-byte scale and the writer's header (ESVO: 20-byte preamble,
 * CSVO: 4-byte root pointer). This is the exact `dst_len` for write_changes_to(ptr + 4, dst_len, reset): its check
 * `start + length < dst_len` (esvo.rs:328, csvo.rs:301) is relative to the first byte AFTER that header. (The reference itself
 * passes `len - 1` (svo.rs:180), which lets a nearly full world run up to 22 bytes past the mapped buffer; the staging mirror
 * is allocated 64 bytes larger than vx_capacity() so that this call pattern cannot write outside it, and vx_commit rejects
 * any range or used_bytes beyond vx_arena_capacity() with VX_ERR_CAPACITY.) */
size_t vx_arena_capacity(const vx_context* ctx);
/* Svo::update (svo.rs:171-189): stores f32 2^-depth at byte 0 (:173-175), waits for in-flight renders like
 * render_fence.wait() (:178), then copies the writer's header and the given dirty arena ranges to the device
 * (asynchronously; later renders/raycasts are ordered after it). used_bytes = WorldSvo::size_in_bytes() for
 * vx_get_stats (:183-187).
 * A context also keeps a traversal image of the world (vx_traversal_image): the chunks inside the given ranges and the root
 * octree are re-laid out as octants of one 8-byte entry per existing child on host worker threads and the changed parts uploaded;
 * vx_render walks the image (device memory on top of the world's own bytes: 0.37x them for ESVO, about 2.3x for CSVO;
 * VX_TRAVERSAL_IMAGE=0 in the environment turns it off). The staging mirror must hold the whole current world, i.e. every change has to go through
 * vx_staging_ptr (it does when write_changes_to is the only writer). */
int vx_commit(vx_context* ctx, uint32_t depth, const vx_range* ranges, uint32_t count, uint64_t used_bytes);
/* Same, treating [0, used_bytes) of the arena as dirty (what the first write_changes_to after write_to does). */
int vx_commit_all(vx_context* ctx, uint32_t depth, uint64_t used_bytes);
/* Pipelined commits. VX_COMMIT_INLINE (default): vx_commit does the image update and queues the uploads before it returns, and
 * every later render sees the new world. VX_COMMIT_PIPELINED: vx_commit only posts the job to a worker thread of the context
 * (0.01 ms) and returns; the worker updates the image, packs and queues the uploads while the caller goes on -- renders issued
 * meanwhile show the world as of the commit before, WHOLLY (world bytes and image change together, ordered on the
 * device behind the frames in flight and before every later one), so a change becomes visible at most one frame late, like the
 * reference's own one-frame lag between Svo::update and the next fence (svo.rs:171-189, 196-229). One job at a time: the next
 * vx_commit, vx_staging_ptr (the worker reads the mirror: ask for the pointer before writing the next changes, as
 * write_changes_to's callers do), vx_commit_wait and vx_sync wait for the posted one. A pipelined commit's error (VX_ERR_HIP
 * etc.) is reported by the next vx_commit, vx_commit_wait or vx_sync. The first commit of a context is always done inline. */
typedef enum vx_commit_mode { VX_COMMIT_INLINE = 0, VX_COMMIT_PIPELINED = 1 } vx_commit_mode;
int vx_set_commit_mode(vx_context* ctx, int mode);
/* wait until the posted commit has been queued on the device (not for the device itself: vx_sync), return its error */
int vx_commit_wait(vx_context* ctx);
/* Svo::get_stats (svo.rs:191-193) */
int vx_get_stats(const vx_context* ctx, vx_stats* out);

/* ---- the hot path ---------------------------------------------------------------------------------------- */

/* Svo::render (svo.rs:196-229) = world.glsl main for every pixel: primary ray, shading, <=1 shadow ray, sky.
 * Device targets are written asynchronously on the context's stream (vx_sync = the render fence); host
 * targets return when the image is in place.
 * Scheduling only, never a pixel's value: image-only renders use what earlier frames of the same view on the same stream cost -- the
 * order in which work is handed out, and (a view whose uniforms are bit for bit the last frame's) which pixels a wave's lanes take
 * together -- so a view that stands still renders faster from its third frame on; a moving view is not affected. */
int vx_render(vx_context* ctx, const vx_uniforms* uniforms, uint32_t width, uint32_t height, const vx_target* target);
/* Svo::raycast (svo.rs:233-255) = picker.glsl over `count` tasks (no 100-task cap); synchronous like the
 * reference's fence wait (:248-249). Host pointers. */
int vx_raycast(vx_context* ctx, const vx_picker_task* tasks, uint32_t count, vx_picker_result* results);
/* Svo::raycast (svo.rs:233-255) = picker.glsl:30-51 for the plain rays of a batch (PickerBatch::add_ray, svo_picker.rs:53-55), read where
 * they lie: `count` rays gathered through the strides of `rays` (packed [N,3] arrays, vx_picker_task or vx_entity records, one direction
 * or one max_dst for all), `count` hits written to `hits`. A ray means what picker.glsl's task means and is not validated, like
 * vx_raycast's; dst, inside_voxel and pos are bit for bit vx_raycast's, `value` is the block hit (what the reference asks the host world
 * for after the cast: get_block(floor(pos)), gameplay.rs:161-201) and face_id names the normal. One ray a lane on the world's own bytes.
 * memory = VX_MEM_HOST: synchronous like Svo::raycast (svo.rs:248-249): the rays are packed into pinned memory the kernel reads and the
 * hits come back through it; one launch, one wait. VX_MEM_DEVICE: every pointer of `rays` and `hits` is device memory (`rays` itself is
 * read on the host during the call); enqueued on the context's stream, returns after enqueueing, ordered like every other launch on that
 * stream -- behind the commits made so far and behind an earlier vx_physics_step, whose vx_entity records it may read directly
 * (origin = &entities[0].position, origin_stride = 64); later commits wait for it; the fence is vx_sync.
 * `hits` must not overlap anything `rays` points to.
 * VX_ERR_INVALID_ARGUMENT (its message names the field; nothing is written): a null ctx, or null rays / hits with count > 0; a null
 * origin or dir; a stride that breaks the rules of vx_ray_batch; an unknown bit in flags; an unknown memory kind. count == 0: VX_OK.
 * Before the first commit: VX_ERR_STATE. */
int vx_raycast_batch(vx_context* ctx, const vx_ray_batch* rays, uint32_t count, int memory, vx_ray_hit* hits);
/* world.glsl:27-108,132-138 for rays the caller generates itself: per ray i of the batch -- gathered through the strides of `rays` exactly as
 * vx_raycast_batch gathers it -- trace_ray(ro, rd) (a primary cast with cast_translucent = true, the highlight outline, the normal map, diffuse
 * and specular light, at most one shadow ray along -light_dir) or, where nothing was hit, get_sky_color(rd). world.glsl's main (:110-129) is
 * the only part of the shader that knows a camera, and it is the part left out: an orthographic map, a cube map, a distorted or foveated view,
 * a mirror ray or a sparse set of pixels are batches of rays. One ray a lane on the world's own bytes, a kernel of its own (csrc/trace).
 * Outputs, at least one of them: `rgba` receives `count` pixels at index i in `format` -- VX_FORMAT_RGBA32F: 16 bytes a ray; VX_FORMAT_RGBA8: the
 * 4 bytes vx_render's RGBA8 targets hold (clamp to [0,1], round to the nearest of 255 steps, NaN -> 0), with no row flip: a batch has no
 * rows --; `hits` receives `count` vx_hit records, each exactly what vx_render records for a pixel whose primary ray is that ray (t, value,
 * face_id, flags, pos, lod, uv, shadow_t, steps = primary + shadow), bit for bit; colours agree with vx_render's to the stated 5e-6.
 * Uniforms: ambient, light_dir, cam_pos, render_shadows, shadow_distance and highlight_pos are used; view, fovy and aspect are ignored.
 * cam_pos feeds the specular term only (world.glsl:73) and is independent of the rays' origins.
 * max_dst limits the PRIMARY cast only -- a ray it ends is a miss and gets the sky --; the shadow ray is never limited, as in the shader.
 * max_dst = NULL with max_dst_all = -1 is the shader's own behaviour. flags: 0 or VX_RAYS_TRANSLUCENT, and both cast as world.glsl:29 does
 * (translucent). A ray means what trace_ray's arguments mean and is not validated: the shader passes a normalised rd, and get_sky_color
 * divides by the length of its horizontal part (rd.x = rd.z = 0 makes the sky term 0/0 there as here).
 * Memory kinds, ordering and fences are vx_raycast_batch's. VX_MEM_HOST: synchronous; rays, pixels and records travel through pinned memory
 * the kernel reads and writes; one launch, one wait. VX_MEM_DEVICE: every pointer of `rays`, `rgba` and `hits` are device memory (`uniforms`
 * and `rays` themselves are read on the host during the call; rgba aligned to a pixel, hits to 16 bytes); enqueued on the context's stream,
 * returns after enqueueing, ordered behind the commits made so far, an earlier vx_physics_step and an earlier vx_raycast_batch; later commits
 * wait for it; the fence is vx_sync. rgba and hits must not overlap each other or anything `rays` points to.
 * VX_ERR_INVALID_ARGUMENT (its message names the field; nothing is written): a null ctx; null uniforms, null rays or both outputs null with
 * count > 0; vx_ray_batch's stride and null rules; an unknown bit in flags; an unknown memory kind or format; count > 16777216 (2^24).
 * count == 0: VX_OK. Before the first commit: VX_ERR_STATE. */
int vx_trace_rays(vx_context* ctx, const vx_uniforms* uniforms, const vx_ray_batch* rays, uint32_t count, int memory, void* rgba, int format,
                  vx_hit* hits);
/* Svo::render (svo.rs:196-229) = world.glsl's main (world.glsl:110-141) for every pixel of `count` SMALL views in ONE launch: the eyes of a few
 * hundred entities, the six faces of a cube map, a handful of probes -- where a vx_render per view pays a launch (and, for host targets, a wait) per
 * view for a grid a 64 x 64 image cannot fill. main is the part vx_trace_rays leaves out; this call puts it back, per view: the pixel's primary
 * ray from the view's `view`, `fovy` and `aspect`, then trace_ray or the sky as vx_trace_rays runs them, shaded with the view's own ambient,
 * light_dir, cam_pos, render_shadows, shadow_distance and highlight_pos. One pixel a lane on the world's own bytes, a workgroup an 8 x 8 tile of
 * one view, a kernel of its own (csrc/trace); it walks no traversal image, so deep worlds and textures whose height is no power of two behave as
 * they do for vx_trace_rays and the picker.
 * `views`: `count` vx_uniforms records in HOST memory whatever `memory` says; they are read during the call (the tangent of fovy / 2 and the
 * ray origin are evaluated on the host, as vx_render evaluates them, or the rays would not be vx_render's bit for bit) and may be overwritten
 * as soon as it returns. All views share width, height and format.
 * Outputs, at least one of them: view k's image lies at pixel k * width * height of `rgba`, its records at the same index of `hits`; inside a
 * view every pixel and record lies where vx_render puts it for a whole-image target of that format -- VX_FORMAT_RGBA32F: row 0 = bottom;
 * VX_FORMAT_RGBA8: the top row first, for the records too. View k's records are bit for bit those of vx_render(ctx, &views[k], width, height,
 * {hits}); its colours agree with vx_render's to the stated 5e-6, and RGBA8 is the packing of those colours.
 * memory is the kind of rgba and hits. VX_MEM_HOST: synchronous; the table of views, pixels and records travel through pinned memory the kernel
 * reads and writes; one launch, one wait. VX_MEM_DEVICE (rgba aligned to a pixel, hits to 16 bytes): enqueued on the context's stream, returns
 * after enqueueing, ordered behind the commits made so far and an earlier vx_physics_step, vx_raycast_batch or vx_trace_rays; later commits wait
 * for it; the fence is vx_sync. rgba and hits must not overlap.
 * VX_ERR_INVALID_ARGUMENT (its message names the field; nothing is written): an unknown memory kind or format; width or height of 0 or above
 * 8192; count * width * height > 16777216 (2^24); null views or both outputs null with count > 0; a misaligned device output; a null ctx.
 * count == 0: VX_OK. Before the first commit: VX_ERR_STATE. */
int vx_trace_views(vx_context* ctx, const vx_uniforms* views, uint32_t count, uint32_t width, uint32_t height, int memory, void* rgba, int format,
                   vx_hit* hits);
/* Which block is at each of `count` positions: get_block(floor(pos)) (gameplay.rs:161-201), which the reference asks of its host world, asked
 * of the world the device holds -- for callers whose positions lie in device memory and who keep no host world. A float[3] is read at
 * pos + i*pos_stride (pos 4-byte aligned; the stride a multiple of 4 and >= 12): packed [N,3] arrays, vx_entity.position (stride 64) and
 * vx_ray_hit.pos (pos = &hits[0].pos, stride 32) are read in place, behind an earlier vx_physics_step or vx_raycast_batch on the stream.
 * out[i] = the leaf, or the empty cell, that holds floor(p): a pure lookup, the descent from the root by the bits of floor(p) through the
 * world's OWN bytes (ESVO: the child descriptor words get_octant_ptr reads, svo.esvo.glsl:168-173; CSVO: read_next_ptr and read_leaf,
 * svo.csvo.glsl:53-133, across the chunk boundary with its material section) -- so it holds for deep worlds, worlds beyond 4 GiB, worlds
 * without a traversal image and LOD chunks, and has none of a ray's start-inside-a-voxel quirks. A component that is NaN, infinite, below
 * 0 or at or above 2^depth gives {0, VX_CELL_OUTSIDE}; -0.0f is 0. One point a lane.
 * Memory kinds, ordering and fences are vx_raycast_batch's. VX_MEM_HOST: synchronous; positions and records travel through pinned memory the
 * kernel reads and writes; one launch, one wait. VX_MEM_DEVICE (out aligned to 8 bytes): enqueued on the context's stream, returns after
 * enqueueing, ordered behind the commits made so far and earlier batch calls; later commits wait for it; the fence is vx_sync. out must not
 * overlap pos.
 * VX_ERR_INVALID_ARGUMENT (its message names the field; nothing is written): a null ctx; an unknown memory kind; null pos or out with
 * count > 0; a stride that breaks the rule, or a misaligned pos; count > 16777216 (2^24); a misaligned device out. count == 0: VX_OK,
 * whatever pos, pos_stride and out are (nothing is read or written).
 * Before the first commit: VX_ERR_STATE. */
int vx_block_points(vx_context* ctx, const void* pos, uint32_t pos_stride, uint32_t count, int memory, vx_block_cell* out);
/* The block ids of the box [lo, lo + size) in integer SVO coordinates as a dense array, x fastest: out[((z - lo[2]) * size[1] + (y - lo[1])) *
 * size[0] + (x - lo[0])] -- a navigation grid, a minimap slice, or the check that the device's world equals a dense array after a run of
 * commits; the reference would loop get_block (gameplay.rs:161-201) over its host world. Every voxel's value is exactly vx_block_points'
 * value for that voxel's centre. Cells outside the world are 0: lo may be negative and the box may overhang the world. A workgroup reads one
 * brick of 8 x 8 x 8 voxels aligned to the world grid: the levels above it once, the last three per voxel.
 * Memory kinds, ordering and fences are vx_raycast_batch's. VX_MEM_HOST: synchronous, through pinned memory; one launch, one wait.
 * VX_MEM_DEVICE (out aligned to 4 bytes): enqueued on the context's stream, returns after enqueueing, ordered behind the commits made so far
 * and earlier batch calls; later commits wait for it; the fence is vx_sync. lo and size themselves are read during the call.
 * VX_ERR_INVALID_ARGUMENT (its message names the field; nothing is written): a null ctx; an unknown memory kind; null lo or size; size[0] *
 * size[1] * size[2] > 16777216 (2^24: a 256^3 box; callers tile larger ones); a null out for a box that holds a voxel; a misaligned device
 * out. Any size component 0: VX_OK. Before the first commit: VX_ERR_STATE. */
int vx_read_region(vx_context* ctx, const int32_t lo[3], const uint32_t size[3], int memory, uint32_t* out);
/* The blocks the box [lo, lo + size) actually holds, as a compact list, with the faces of each that touch air: what a caller builds a collision
 * or render mesh from, exports a selection with, scatters particles on, or removes in an explosion -- the reference would loop get_block
 * (gameplay.rs:161-201) over the box, and over each block's six neighbours. A dense vx_read_region of terrain is almost all air and buried
 * rock; this is its non-zero voxels only, or -- VX_LIST_EXPOSED -- only those that can be seen.
 * Which voxels: a record for every voxel of the box whose vx_read_region value is not 0; under VX_LIST_EXPOSED only those of them with a
 * face bit set. A LOD voxel of side 2^k gives one record per fine voxel of it inside the box, as vx_read_region does; its inner voxels have
 * no open face.
 * Faces: a neighbour is judged by the world -- vx_block_points' value at that voxel's centre, and air outside [0, 2^depth)^3 -- whether or
 * not it lies in the box: the lists of two boxes that tile a larger one are the larger one's list with `where` re-based. Translucent blocks
 * count as blocks.
 * Order: fixed and reproducible, ascending by (z >> 3, y >> 3, x >> 3, z, y, x) in world coordinates: brick by brick of the 8 x 8 x 8 grid
 * vx_read_region's workgroups own, x fastest, and inside a brick in dense-index order.
 * total and capacity: *total receives the number of records the box has under `flags`, whatever `capacity` is; the first min(total, capacity)
 * records in that order are written to `out`, and nothing beyond them. capacity == 0 only counts; out may then be null.
 * Three launches on the context's stream, one wave a brick in the first and the last: the records of each brick counted, the counts summed
 * into offsets (no kernel waits for another workgroup), the records written.
 * `memory` is the kind of `out` and `total`; ordering and fences are vx_read_region's. VX_MEM_HOST: synchronous, through pinned memory; only
 * the records written are copied back. VX_MEM_DEVICE (out aligned to 8 bytes, total to 4): enqueued on the context's stream, returns after
 * enqueueing; later commits wait for it; the fence is vx_sync. lo and size themselves are read during the call.
 * VX_ERR_INVALID_ARGUMENT (its message names the field; nothing is written): a null ctx; an unknown memory kind; an unknown bit in flags;
 * null lo or size; size[0] * size[1] * size[2] > 16777216 (2^24, vx_read_region's limit: 24 bits hold the index); a null total for a box
 * that holds a voxel; a null out with capacity > 0 for such a box; a misaligned device out or total. Any size component 0: VX_OK, *total = 0
 * is written if total is not null, out is not touched. Before the first commit: VX_ERR_STATE. */
#define VX_LIST_FACES   1u  /* fill each record's face bits */
#define VX_LIST_EXPOSED 2u  /* keep only blocks with at least one face bit set; implies VX_LIST_FACES */
/* One block of a box; 8 bytes. */
typedef struct vx_block_at {
    uint32_t where;  /* bits 0..23: the voxel's index in vx_read_region's dense array for the same box,
                        ((z-lo[2])*size[1] + (y-lo[1]))*size[0] + (x-lo[0]);
                        bits 24..29: faces, bit f (numbered like face_id: -x,+x,-y,+y,-z,+z) set when the neighbouring voxel
                        on that side holds no block; 0 without VX_LIST_FACES; bits 30..31: 0 */
    uint32_t value;  /* its BlockId, never 0 */
} vx_block_at;
#define VX_AT_INDEX(where) ((where) & 0xFFFFFFu)
#define VX_AT_FACES(where) (((where) >> 24) & 0x3Fu)
int vx_list_region(vx_context* ctx, const int32_t lo[3], const uint32_t size[3], uint32_t flags, int memory,
                   vx_block_at* out, uint32_t capacity, uint32_t* total);
/* The first block below (above, beside) each of `count` positions: get_block (gameplay.rs:161-201) looped along an axis, asked of the world
 * the device holds -- the ground under every entity, the ceiling over it, which positions see the sky. Positions are gathered exactly as
 * vx_block_points gathers them (packed arrays, vx_entity.position, vx_ray_hit.pos in place). start = floor(p) per component, saturated to
 * int32; the scan visits the voxels start, start +- 1, ... along the axis of `direction` (VX_DIR_*), `reach` of them at the most (start
 * included; VX_SCAN_TO_EDGE: up to the world's far edge), and answers with the first whose value -- vx_block_points' value for the voxel's
 * centre; air outside [0, 2^depth)^3 -- is not 0: its coordinate on that axis, the value, and the leaf's cell_log2. The start voxel
 * counts: a scan that starts inside a block or a LOD voxel answers coord = start. A LOD voxel entered from outside answers with its near
 * face in travel order. No block: {VX_SCAN_NONE, 0, 0, 0}. A NaN or infinite component: {VX_SCAN_NONE, 0, VX_CELL_OUTSIDE, 0}. A finite
 * position outside the world is a valid start (the scan may enter the world). Integer-only and exact like vx_block_points; empty space is
 * stepped over a whole empty cell of the octree at a time, so a scan from the top of a deep world takes a few dozen descents, not one a
 * voxel. One column a lane.
 * Memory kinds, ordering and fences are vx_block_points'. VX_MEM_DEVICE: out aligned to 16 bytes. out must not overlap pos.
 * VX_ERR_INVALID_ARGUMENT (its message names the field; nothing is written): a null ctx; an unknown memory kind; a direction outside
 * 0..5; with count > 0: vx_block_points' stride, alignment and null rules, count > 16777216 (2^24), reach == 0, a misaligned device out.
 * count == 0: VX_OK. Before the first commit: VX_ERR_STATE. */
int vx_scan_points(vx_context* ctx, const void* pos, uint32_t pos_stride, uint32_t count, int direction, uint32_t reach, int memory,
                   vx_scan_hit* out);
/* The same scan for every column of the box [lo, lo + size) in integer SVO coordinates (as in vx_read_region: lo may be negative, the box
 * may overhang the world), as a dense array: a heightmap, a sky mask, an orthographic elevation along any axis. With a the axis of
 * `direction` and u < v the two other axes in x, y, z order there is one column per (u, v) of the box; it scans the box's extent along a
 * from the face it enters (start = lo[a] + size[a] - 1 for a negative direction, lo[a] for a positive one) and its record goes to
 * out[(v - lo[v]) * size[u] + (u - lo[u])]: a top-down heightmap (VX_DIR_NEG_Y) is [z][x]. A wave owns a tile of 8 x 8 columns aligned to
 * the world grid and walks the bricks along the axis: the levels above a brick once for the whole wave, empty cells stepped over by the whole
 * wave, the last three levels per lane.
 * Memory kinds, ordering and fences are vx_block_points'. VX_MEM_DEVICE: out aligned to 16 bytes.
 * VX_ERR_INVALID_ARGUMENT (its message names the field; nothing is written): a null ctx; an unknown memory kind; a direction outside
 * 0..5; null lo or size; size[u] * size[v] > 16777216 (2^24) columns; size[a] > 16777216; a null out for a box that holds a voxel; a
 * misaligned device out. Any size component 0: VX_OK. Before the first commit: VX_ERR_STATE. */
int vx_scan_columns(vx_context* ctx, const int32_t lo[3], const uint32_t size[3], int direction, int memory, vx_scan_hit* out);
/* What is inside each of `count` axis-aligned float boxes (vx_box_batch): does the box overlap a block, how many voxels of it, which block
 * first, and within which bounds -- the reference's test of the player's AABB against a voxel (handle_voxel_placement, gameplay.rs:211-222)
 * for a batch, asked of the world the device holds: spawn and placement checks, "is this entity stuck", "how much of it is under water"
 * (only_value), the bounds to push a penetrating entity out along, trigger volumes.
 * When a record is a box: every component of origin, offset and extents is finite, every extent is > 0 and <= 64, and mn and mx are finite.
 * Anything else gives {VX_BOX_INVALID, 0, {0,0,0}, {0,0,0}} in both memory kinds (vx_block_points' way with a position that is no position);
 * the call does not fail for it. The limit of 64 keeps a wave's walk to at most 9 bricks an axis: larger volumes are vx_list_region with
 * capacity == 0.
 * The cover: per axis the voxels v with v + 1 > mn and v < mx (overlap of positive length: a box resting exactly on a block's top does not
 * overlap it; a caller who wants touching to count grows the box) -- floor(mn) .. ceil(mx) - 1, then cut to the world [0, 2^depth): outside
 * the world is air. A cover with no voxel on some axis (outside the world; a huge coordinate whose add absorbs the extent) gives blocks = 0.
 * Coordinates such as 3e9, -3e9 and 1e30 are valid.
 * What a voxel holds: vx_block_points' value at its centre; a LOD voxel of side 2^k counts once for each fine voxel of it inside the cover, as
 * in vx_read_region; translucent blocks count. With only_value != 0 a voxel counts when its value equals it; the count, the first block and
 * the bounds all use that one rule.
 * One wave a box: the wave walks the bricks of 8 x 8 x 8 voxels the cover touches, the levels above a brick once for the wave, the last three
 * per lane, and folds its lanes' answers once at the end. One launch.
 * Memory kinds, ordering and fences are vx_block_points'. VX_MEM_HOST: synchronous; the three vectors of each box travel unchanged through
 * pinned memory (the kernel does the adds in both memory kinds); one launch, one wait. VX_MEM_DEVICE (out aligned to 16 bytes): enqueued on
 * the context's stream, returns after enqueueing, ordered behind the commits made so far and earlier batch calls (it may read the vx_entity
 * records an earlier vx_physics_step wrote); later commits wait for it; the fence is vx_sync. out must not overlap what `boxes` points to;
 * `boxes` itself is read during the call.
 * VX_ERR_INVALID_ARGUMENT (its message names the field; nothing is written): a null ctx; an unknown memory kind; with count > 0: null boxes,
 * out, origin or extents; a stride or an alignment that breaks vx_box_batch's rules; count > 16777216 (2^24); a misaligned device out.
 * count == 0: VX_OK (nothing is read or written). Before the first commit: VX_ERR_STATE. */
int vx_overlap_boxes(vx_context* ctx, const vx_box_batch* boxes, uint32_t count, int memory, vx_box_hit* out);
/* Each of `count` boxes (vx_box_batch, read as vx_overlap_boxes reads it, only_value included) moved by its motion through the world the
 * device holds and stopped by blocks: how far it gets, and what stopped it. Unlike the picker fan behind vx_physics_step (rays a voxel apart,
 * 10 long, all three axes clamped from the start position) every voxel ahead of the box's face counts, and the move goes axis by axis, each
 * axis judged from where the earlier ones left the box. One launch, one wave a box.
 * Motion: a float[3] at motion + i * motion_stride (a multiple of 4 and >= 12, or 0 = one motion for every box), 4-byte aligned, in the
 * memory kind of the call; the displacement is d = motion * shape->scale, one fp32 multiply a component.
 * Invalid records: a record that is no box (vx_overlap_boxes' rule), a motion with a non-finite component, or a displacement with a
 * non-finite component or one above VX_MOVE_MAX_TRAVEL in magnitude gives contacts = VX_MOVE_INVALID and every other word 0; the call does
 * not fail for it.
 * The rule. The passes run in the order shape->order gives; the pass of axis a uses the box as the earlier passes left it and ends with
 * origin[a] = origin[a] + m, mn[a] = origin[a] + offset[a], mx[a] = mn[a] + extents[a], one fp32 add each: what a later vx_overlap_boxes of
 * the new origin computes. d == 0 (or -0): m = 0, no scan, no contact bit, value[a] = 0. Else the cross-section is the cover (floor(mn) ..
 * ceil(mx) - 1, cut to the world) on the two other axes; an empty one finds nothing. The layers ahead, cut to [0, 2^depth) in float before
 * the conversion:
 *   d > 0: end = mx[a] + (d + skin); v in ceil(mx[a]) .. ceil(end) - 1; the nearest layer is the smallest v that holds a counted voxel within
 *          the cross-section; gap = float(v) - mx[a]; m = min(d, max(0, gap - skin)).
 *   d < 0: end = mn[a] + (d - skin); v in floor(end) .. floor(mn[a]) - 1; the nearest is the largest v; gap = mn[a] - float(v + 1);
 *          m = -min(-d, max(0, gap - skin)).
 * Voxels the box already overlaps along a lie behind its leading face and are never obstacles: a stuck box can move out. A face exactly on
 * an integer plane has that plane's layer ahead of it at gap 0. A voxel counts as in vx_overlap_boxes (its value is not 0, or equals
 * only_value; a LOD voxel once for each of its fine voxels; outside the world is air). Nothing found: m = d, no bit, value 0. Something
 * found: the contact bit is set, even when m == d, and value[a] is the first counted voxel of the nearest layer within the cross-section in
 * vx_read_region's order (z, then y, then x ascending).
 * Memory kinds, ordering and fences are vx_overlap_boxes': VX_MEM_HOST is synchronous through pinned memory; VX_MEM_DEVICE (out aligned to
 * 16 bytes) is enqueued on the context's stream behind commits and earlier batch calls. out overlaps no input: the origins are not written
 * back in place.
 * VX_ERR_INVALID_ARGUMENT (its message names the field; nothing is written): vx_overlap_boxes' list; a null shape; a null motion with
 * count > 0; a motion stride or alignment that breaks the rule; a non-finite scale; a skin outside [0, 1] or NaN; an order that is no
 * permutation or has other bits set; flags != 0. count == 0: VX_OK. Before the first commit: VX_ERR_STATE. */
int vx_move_boxes(vx_context* ctx, const vx_box_batch* boxes, const void* motion, uint32_t motion_stride, uint32_t count,
                  const vx_move_shape* shape, int memory, vx_move_hit* out);
/* Step distances through air around each of `count` positions: a breadth-first flood of a small box, asked of the world the device holds --
 * which cells a mob can reach and in how many steps (a flow field to walk down), how far a lamp's light gets around corners, whether a room
 * is sealed or the flood leaks out of the box, how big a cave is. The reference would loop get_block (gameplay.rs:161-201) over the
 * neighbourhood and search on the host. Everything is integer and exact.
 * Positions are gathered exactly as vx_block_points gathers them (packed arrays, vx_entity.position, vx_ray_hit.pos in place). The seed is
 * floor(p) per component, saturated to int32 as in vx_scan_points; the box of the query is [lo, lo + size) with lo = seed - seed_at (kept
 * modulo 2^32 as vx_read_region keeps a box: it may overhang the world, and finite positions such as 3e9 and -3e9 are valid). A NaN or
 * infinite component is no position: the field is all VX_FLOOD_NO_POSITION and the record {VX_FLOOD_INVALID, 0, 0, 0}; the call does not fail.
 * A cell is passable when vx_block_points' value at its centre is 0 or equals a non-zero pass_value; outside [0, 2^depth)^3 is air; a LOD
 * voxel blocks each of its fine voxels. Cells outside the box do not exist: the box bounds the flood.
 * Steps are 6-connected: a cell's byte is the length of the shortest path from the seed through passable cells of the box, when that is at
 * most max_steps; other passable cells are VX_FLOOD_UNREACHED, impassable ones VX_FLOOD_BLOCKED. A seed that is not passable reaches nothing
 * ({0, 0, 0, seed_value}); under VX_FLOOD_SEED_ALWAYS it is step 0 and spreads, and its own byte is 0.
 * At least one of `fields` and `info` is given. Query k's field is size[0] * size[1] * size[2] bytes at fields + k * field_stride, laid out as
 * vx_read_region lays a box out (x fastest). field_stride is a multiple of 16 and at least the voxel count; 0 means the voxel count rounded
 * up to 16. The bytes from the voxel count up to its multiple of 16 are written VX_FLOOD_BLOCKED (for every query, one without a position
 * too); bytes beyond are not touched. With fields == NULL only the records are written: the cheap "is it sealed, how big is it".
 * One workgroup of four waves a query: the box's passable cells as rows of 32 bits in LDS (each brick of 8 x 8 x 8 voxels entered once), a
 * flood step a handful of shifts and ORs a row. One launch; no workgroup waits for another.
 * Memory kinds, ordering and fences are vx_block_points'. VX_MEM_HOST: synchronous, through pinned memory; one launch, one wait.
 * VX_MEM_DEVICE (fields and info aligned to 16 bytes): enqueued on the context's stream, returns after enqueueing, ordered behind the commits
 * made so far and earlier batch calls (it may read the vx_entity records an earlier vx_physics_step wrote); later commits wait for it; the
 * fence is vx_sync. The outputs must not overlap pos or one another; `shape` itself is read during the call.
 * VX_ERR_INVALID_ARGUMENT (its message names the field; nothing is written): a null ctx; an unknown memory kind; with count > 0: a null
 * shape or pos; fields and info both null; vx_block_points' stride and alignment rules; a size component of 0 or above 32; seed_at >= size;
 * max_steps > VX_FLOOD_MAX_STEPS; an unknown flag bit; a field_stride that breaks the rule; count > 16777216 (2^24), or with fields count *
 * field_stride > 16777216 bytes; a misaligned device output. count == 0: VX_OK (nothing is read or written). Before the first commit:
 * VX_ERR_STATE. */
int vx_flood_points(vx_context* ctx, const void* pos, uint32_t pos_stride, uint32_t count, const vx_flood_shape* shape, int memory,
                    uint8_t* fields, uint32_t field_stride, vx_flood_info* info);
/* Sky and block light levels, 0..15 each, for every cell of `count` boxes of the world the device holds -- what mesh shading, mob spawning,
 * plant growth and "is this room dark" read, and what the reference's host would compute by looping get_block (gameplay.rs:161-201) over a
 * section and its margin and running two breadth-first searches. Everything is integer and exact.
 * Box k is [lo_k, lo_k + size): lo_k an int32[3] read at lo + k * lo_stride, in the memory kind of the call, 4-byte aligned, the stride a
 * multiple of 4 and at least 12 (a packed array, or a field of a larger record in place). It is kept modulo 2^32 as vx_read_region keeps a
 * box: it may be negative or overhang the world. A cell holds vx_block_points' value at its centre: outside [0, 2^depth)^3 is air, a LOD
 * voxel gives its value to each of its fine voxels. A cell is passable when its value is 0 or props[value] has VX_LIGHT_TRANSPARENT.
 * Sky (the high nibble): a cell is exposed when it is passable and every cell above it in the world -- the same x and z, larger y, inside the
 * box or beyond it, up to the world's top -- is passable. Exposed cells have 15; every other passable cell has max(0, the largest of its six
 * neighbours inside the box - 1); impassable cells have 0. Cells outside the box do not exist for the spread: only the exposure test looks
 * beyond the box, and only upwards.
 * Block (the low nibble): a cell whose block emits e > 0 has at least e whether or not it is passable (a lamp is a block); a passable cell
 * has the larger of its own emission and (the largest of its six neighbours inside the box - 1), floored at 0; an impassable cell has just
 * its emission: it lights its neighbours but lets nothing through.
 * Light falls off by one a step, so nothing farther than 15 cells matters: a caller who wants the levels of a 16^3 section to be independent
 * of the box asks for the section with 15 cells of margin on every side -- a box of 46 -- and keeps the middle.
 * At least one of `fields` and `info` is given. Query k's field is size[0] * size[1] * size[2] bytes at fields + k * field_stride, sky << 4 |
 * block a cell, laid out as vx_read_region lays a box out (x fastest). field_stride is a multiple of 16 and at least the voxel count; 0
 * means the voxel count rounded up to 16. The bytes from the voxel count up to its multiple of 16 are written 0; bytes beyond are not
 * touched. With fields == NULL only the records are written. A flag leaves its channel out: the nibble is 0 and so is the record's count
 * of it (open_columns, sources).
 * One workgroup of four waves a query: the box's passable cells and emissions as rows of 64 bits (each brick of 8 x 8 x 8 voxels entered
 * once), one upward scan a column above the box that steps over empty octree cells, a level-ordered flood of shifts and ORs a row and
 * channel. One launch; no workgroup waits for another.
 * Memory kinds, ordering and fences are vx_flood_points'. VX_MEM_HOST: synchronous, through pinned memory; one launch, one wait.
 * VX_MEM_DEVICE (fields and info aligned to 16 bytes): enqueued on the context's stream, returns after enqueueing, ordered behind the commits
 * made so far and earlier batch calls; later commits wait for it; the fence is vx_sync. The outputs must not overlap lo or one another.
 * `shape` and `props` are host memory read during the call: props travels through pinned memory ordered on the stream, and the caller may
 * overwrite it when the call returns.
 * VX_ERR_INVALID_ARGUMENT (its message names the field; nothing is written): a null ctx; an unknown memory kind; with count > 0: a null
 * shape or lo; fields and info both null; a stride or an alignment that breaks the rules above; a size component of 0 or above 48; an unknown
 * flag bit, or both flags; props_count > 4096, or null props with props_count > 0; a props byte with one of bits 5..7 set; a field_stride that
 * breaks the rule; count > 16777216 (2^24), or with fields count * field_stride > 16777216 bytes; a misaligned device output. count == 0:
 * VX_OK (nothing is read or written). Before the first commit: VX_ERR_STATE. */
int vx_light_boxes(vx_context* ctx, const void* lo, uint32_t lo_stride, uint32_t count, const vx_light_shape* shape, int memory,
                   uint8_t* fields, uint32_t field_stride, vx_light_info* info);
/* Walking distances and paths for ground agents around each of `count` positions: where vx_flood_points floods through air (a mob that
 * flies), this call searches the walking graph of the world the device holds -- cells with a floor under them and headroom for the agent,
 * steps of one block up, drops of a few blocks down -- and traces the path from the position to a goal. The reference would loop get_block
 * (gameplay.rs:161-201) over the neighbourhood and search on the host. Everything is integer and exact.
 * Cells. Positions, the box ([lo, lo + size), lo = floor(p) - seed_at modulo 2^32, floor saturated to int32) and the field layout are
 * vx_flood_points': a byte a cell, x fastest, at fields + k * field_stride; field_stride is 0 (the voxel count rounded up to 16) or a
 * multiple of 16 and at least the voxel count; the bytes from the voxel count up to its multiple of 16 are written VX_WALK_NO_STAND, bytes
 * beyond are not touched. A cell is passable when vx_block_points' value there is 0 or equals a non-zero pass_value; outside the world is
 * air; a LOD voxel blocks each of its fine voxels.
 * Standable. Cell (x, y, z) is standable when (x, y .. y + height - 1, z) are all passable and (x, y - 1, z) is not. This is judged by the
 * WORLD, also below the box's bottom layer and above its top: size[1] + height layers are read, one below the box and height - 1 above it
 * (the up and drop rules reach no higher), so size[1] + height <= 32. Nothing outside the world is a floor. Only cells of the box are
 * nodes.
 * Edges run from a standable cell c = (x, y, z) to a standable cell c' = (x', y', z') of a column next to it (x +- 1 or z +- 1, no
 * diagonals, inside the box), and each costs one step:
 *   level: y' = y;
 *   up, with climb == 1: y' = y + 1, and (x, y + height, z) is passable -- the agent rises in its own column first;
 *   down by d = 1..drop: y' = y - d, and (x', y' + height .. y + height - 1, z') are passable -- the agent moves over at its own level,
 *   then falls.
 * Settling. The seed is floor(p). If (x, s.y .. s.y + height - 1, z) are not all passable it stands nowhere. Otherwise it falls while the
 * cell below is passable and stands on the first standable cell; if it leaves the box's bottom first, it stands nowhere. A seed that
 * stands nowhere reaches nothing -- {0, 0, 0, seed_value, VX_WALK_NONE, goal_ry, VX_WALK_NONE, 0} -- and its field still tells standable
 * from not. `goal` may be NULL; otherwise a float[3] is read at goal + k * goal_stride under pos' own stride and alignment rules, a
 * goal_stride of 0 meaning one goal for all. The goal settles by the same rule, and must lie in the box before and after settling. A NaN
 * or infinite goal is "no goal" for that query, not an error. A NaN or infinite pos is no position: the field is all VX_WALK_NO_POSITION,
 * the record {VX_FLOOD_INVALID's value, 0, 0, 0, VX_WALK_NONE, VX_WALK_NONE, VX_WALK_NONE, 0} and the path all VX_WALK_NONE.
 * The field. Breadth-first step counts over that graph from the settled seed, up to max_steps; VX_WALK_UNREACHED for other standable
 * cells, VX_WALK_NO_STAND for the rest. The record's reached, farthest, faces and seed_value are vx_flood_info's, over standable cells
 * (seed_value is the value at floor(p), not where it settled).
 * VX_WALK_STOP_AT_GOAL: the flood ends after the whole step that reaches the settled goal; the field and the record are exactly those of
 * max_steps = min(max_steps, path_steps).
 * Paths. A path is written when goal, paths and path_capacity > 0 are all given: query k's entries are path_capacity uint32 at paths + k *
 * path_capacity. Entry i is the cell after i + 1 steps, as rx | ry << 8 | rz << 16 (entry 0 is the next cell to move to). The first
 * min(path_steps, path_capacity) entries are written; the rest, up to the capacity, are VX_WALK_NONE, and with no path every entry is.
 * The path is found backwards from the goal: from a cell of step k, the first cell of step k - 1 that has an edge to it, searched by the
 * side it lies on in the order -x, +x, -z, +z, and per side level, then from below (the up edge), then from above by d = 1, 2, 3. That
 * makes the path unique.
 * One workgroup of four waves a query, one launch; no workgroup waits for another.
 * At least one of fields, info and paths is given. Memory kinds, ordering and fences are vx_flood_points'. VX_MEM_HOST: synchronous,
 * through pinned memory. VX_MEM_DEVICE (fields, paths and info aligned to 16 bytes): enqueued on the context's stream, ordered behind the
 * commits made so far and earlier batch calls; later commits wait for it; the fence is vx_sync. The outputs must not overlap the inputs or
 * one another; `shape` itself is read during the call.
 * VX_ERR_INVALID_ARGUMENT (its message names the field; nothing is written): a null ctx; an unknown memory kind; with count > 0: a null
 * shape or pos; fields, info and paths all null; paths without goal; vx_block_points' stride and alignment rules for pos, and for goal
 * with a goal_stride of 0 allowed; a size, seed_at, max_steps, height, climb, drop, path_capacity or flags outside what vx_walk_shape
 * states; a field_stride that breaks the rule; count > 16777216 (2^24), or count * field_stride or count * path_capacity * 4 above
 * 16777216 bytes; a misaligned device output. count == 0: VX_OK (nothing is read or written). Before the first commit: VX_ERR_STATE. */
int vx_walk_points(vx_context* ctx, const void* pos, uint32_t pos_stride, const void* goal, uint32_t goal_stride, uint32_t count,
                   const vx_walk_shape* shape, int memory, uint8_t* fields, uint32_t field_stride, uint32_t* paths, vx_walk_info* info);
/* The loose pieces of the blocks in each of `count` boxes of the world the device holds: "a block was removed, so what no longer hangs on
 * anything?" -- after an explosion, a felled tree or a mined pillar, the connected pieces of solid blocks of a neighbourhood that the rest
 * of the world does not hold, each with its size and bounds, to fall or to become debris entities. The reference would loop get_block
 * (gameplay.rs:161-201) over the neighbourhood and label components on the host. Everything is integer and exact.
 * Boxes. Box k is [lo_k, lo_k + size): lo_k an int32[3] read at lo + k * lo_stride under vx_light_boxes' rules (4-byte aligned, the stride a
 * multiple of 4 and at least 12), kept modulo 2^32: the box may be negative or overhang the world.
 * Solid. A cell is solid when vx_block_points' value at its centre is non-zero and differs from a non-zero pass_value (the cells
 * vx_flood_points does not pass). Outside the world is air; a LOD voxel makes each of its fine voxels solid. Cells outside the box do not
 * exist.
 * Connectivity is 6-connected through solid cells of the box: contact along an edge or at a corner does not connect.
 * Floods and the budget. A flood starts from a set of seed cells; its layer k holds the cells at breadth-first distance k from the seeds
 * through solid cells that are not yet settled, and its depth is the largest k with a non-empty layer. `used` starts at 0. A flood is
 * complete when used + depth <= max_steps, and then used += depth. Otherwise it is cut: used = max_steps, VX_LABEL_CUT is set, and no further
 * flood is run.
 * Held. The first flood's seeds are the solid cells on the faces of the box that anchor_faces names. Its cells are VX_LABEL_HELD and
 * settled. If it is cut, the layers the budget still covered stay VX_LABEL_HELD: each of those cells really is connected to an anchor.
 * Pieces. While fewer than max_pieces pieces are labelled, nothing was cut and an unsettled solid cell exists: the seed is the unsettled
 * solid cell that comes first in the field's order (least rz, then ry, then rx); the flood from it, when complete, gives its cells the next
 * label -- 1, 2, ... -- settles them and writes the piece's record; when cut, none of its cells are labelled. Every solid cell still
 * unsettled at the end is VX_LABEL_MORE.
 * The record. solid, held, loose and more are cell counts, loose of the cells with labels 1..pieces: solid == held + loose + more. steps is
 * `used`; faces has bit f set when any solid cell lies on face f; flags is 0 or VX_LABEL_CUT. With max_pieces == 0 the call is the cheap
 * "does anything hang loose, and how much": `more` holds the answer.
 * Outputs. At least one of fields, pieces and info is given. Query k's field is a byte a cell in vx_read_region's layout (x fastest) at
 * fields + k * field_stride; field_stride follows vx_flood_points' rule (0: the voxel count rounded up to 16, else a multiple of 16 and at
 * least the voxel count); the bytes from the voxel count up to its multiple of 16 are written VX_LABEL_AIR, bytes beyond are not touched.
 * Query k's piece records are max_pieces records at pieces + k * max_pieces; those of pieces that do not exist are written all 0. `pieces`
 * together with max_pieces == 0 is an error.
 * One workgroup of four waves a query, one launch: the box's solid cells as rows of 32 bits (each brick of 8 x 8 x 8 voxels entered once), a
 * flood step a handful of shifts and ORs a row; no workgroup waits for another.
 * Memory kinds, ordering and fences are vx_flood_points'. VX_MEM_HOST: synchronous, through pinned memory; one launch, one wait.
 * VX_MEM_DEVICE (fields, pieces and info aligned to 16 bytes): enqueued on the context's stream, ordered behind the commits made so far and
 * earlier batch calls; later commits wait for it; the fence is vx_sync. `shape` itself is read during the call.
 * VX_ERR_INVALID_ARGUMENT (its message names the field; nothing is written): a null ctx; an unknown memory kind; with count > 0: a null
 * shape or lo; fields, pieces and info all null; a stride or an alignment that breaks the rules above; a size component of 0 or above 32; an
 * anchor_faces bit above bit 5; max_pieces > VX_LABEL_MAX_PIECES; max_steps > VX_LABEL_MAX_STEPS; flags != 0; pieces with max_pieces == 0;
 * a field_stride that breaks the rule; count > 1048576 (2^20) -- not the other calls' 2^24: a query may run thousands of steps, and the
 * launch must end in bounded time --; count * field_stride or count * max_pieces * 16 above 16777216 (2^24) bytes; a misaligned device
 * output; an output whose bytes, from its first to its last, overlap those of lo or of another output. count == 0: VX_OK (nothing is read
 * or written). Before the first commit: VX_ERR_STATE. */
int vx_label_boxes(vx_context* ctx, const void* lo, uint32_t lo_stride, uint32_t count, const vx_label_shape* shape, int memory,
                   uint8_t* fields, uint32_t field_stride, vx_label_piece* pieces, vx_label_info* info);
/* The squared distance to the nearest block, per cell, in each of `count` boxes of the world the device holds: "does a creature of radius r
 * fit here, and where is the roomiest cell", "how deep inside the rock is this ore", "how far is the nearest lava" -- the straight-line
 * metric from every block at once, where vx_flood_points counts 6-connected steps from one seed. The reference would loop get_block
 * (gameplay.rs:161-201) over the neighbourhood and run a distance transform on the host. Everything is integer and exact.
 * Boxes. Box k is [lo_k, lo_k + size): lo_k an int32[3] read at lo + k * lo_stride under vx_light_boxes' rules (4-byte aligned, the stride a
 * multiple of 4 and at least 12, the memory kind of the call), kept modulo 2^32: the box may be negative or overhang the world. Each size
 * component is 1..32. Cells outside the box do not exist: the box bounds the search.
 * Targets. A cell holds vx_block_points' value at its centre; outside the world is 0; a LOD voxel gives its value to each of its fine
 * voxels. With match_value == 0 a cell is a target when it is solid by vx_label_boxes' rule: non-zero and different from a non-zero
 * pass_value. With match_value != 0 a cell is a target when its value equals match_value; pass_value must then be 0. Under
 * VX_DISTANCE_TO_AIR the target set is complemented within the box: the distance to the nearest cell that is NOT such a block, which is
 * the depth inside rock.
 * The field. `fields` points at uint16_t entries (a void*, as a binding may hold them as either 16-bit integer kind): one a cell, x fastest, in
 * vx_read_region's layout, the least (rx-tx)^2 + (ry-ty)^2 + (rz-tz)^2 over the target cells (tx, ty, tz) of the box. A target cell has 0; the
 * largest possible value is 3 * 31^2 = 2883. With no target in the box every cell is VX_DISTANCE_NONE. Query k's field is at (uint8_t*)fields +
 * k * field_stride; field_stride is in BYTES, a multiple of 16 and at least 2 * voxels, or 0: 2 * voxels rounded up to 16. The entries from the
 * voxel count up to that multiple of 16 bytes are written VX_DISTANCE_NONE; bytes beyond are not touched.
 * What holds across box choices. Let g be a cell's distance in cells to the outside of the box: the least of rx + 1, size.x - rx and the
 * same for y and z. A value v <= g^2 is the value ANY larger box would give -- a nearer target outside the box would lie at least g cells
 * away along some axis. A caller who wants exact values up to radius r inside a section asks for the section with a margin of r, as
 * vx_light_boxes' caller asks for a margin of 15.
 * The record. targets: the number of target cells. farthest: the largest value of the field, VX_DISTANCE_NONE with no target. where: rx |
 * ry << 8 | rz << 16 of the first cell in the field's order (least rz, then ry, then rx) that holds `farthest` -- the roomiest cell; with
 * no target that is cell 0. faces: bit f set when a target lies on face f of the box, numbered like vx_flood_info.faces.
 * Outputs. At least one of fields and info is given; with fields == NULL only the records are written.
 * One workgroup of four waves a box, one launch: the box's targets as rows of 32 bits (each brick of 8 x 8 x 8 voxels entered once), the
 * distance along x read off a row's bits, then one exact min-plus pass along y and one along z (squared Euclidean distance separates
 * exactly in integers). No loop depends on the world: a query's time is bounded whatever the world holds. No workgroup waits for another.
 * Memory kinds, ordering and fences are vx_label_boxes'. VX_MEM_HOST: synchronous, through pinned memory; one launch, one wait.
 * VX_MEM_DEVICE (fields and info aligned to 16 bytes): enqueued on the context's stream, ordered behind the commits made so far and
 * earlier batch calls; later commits wait for it; the fence is vx_sync. `shape` itself is read during the call.
 * VX_ERR_INVALID_ARGUMENT (its message names the field; nothing is written): a null ctx; an unknown memory kind; with count > 0: a null
 * shape or lo; fields and info both null; a stride or an alignment that breaks the rules above; a size component of 0 or above 32; an
 * unknown flag bit; match_value != 0 together with pass_value != 0; a field_stride that breaks the rule; count > 1048576 (2^20); count *
 * field_stride above 16777216 (2^24) bytes; a misaligned device output; an output whose bytes, from its first to its last, overlap those
 * of lo or of the other output. count == 0: VX_OK (nothing is read or written). Before the first commit: VX_ERR_STATE. */
int vx_distance_boxes(vx_context* ctx, const void* lo, uint32_t lo_stride, uint32_t count, const vx_distance_shape* shape, int memory,
                      void* fields, uint32_t field_stride, vx_distance_info* info);
/* Physics::step_many (src/systems/physics.rs:122-136) `steps` times over `count` entities in ONE kernel launch, against the world as last
 * committed: per step and entity the AABB's fan of axis-parallel picker rays (Aabb::generate_picker_tasks, svo_picker.rs:183-243: max_dst
 * 10), folded into six contact distances (parse_picker_results, svo_picker.rs:245-299), then Physics::update_entity and
 * apply_axial_physics (physics.rs:139-185). One wave per entity; the entity stays in registers over all the steps and no task or result
 * array crosses the boundary. Results are bit for bit what Physics::step_many over Svo::raycast gives (the same fp32 operations in the
 * same order). steps <= 1024 and count <= 16777216 (2^24), else VX_ERR_INVALID_ARGUMENT; steps == 0 moves nothing and only fills `contacts`: a batched AABB distance query
 * (PickerBatch::add_aabb, svo_picker.rs:57-59).
 * `contacts` (optional, `count` records, the same memory kind as `entities`) receives the AabbResult each entity's last step was
 * computed from (steps == 0: the fan at the current position).
 * memory = VX_MEM_HOST: synchronous like Svo::raycast (svo.rs:248-249); the records travel through pinned memory the kernel reads and
 * writes directly. VX_MEM_DEVICE: enqueued on the context's stream, returns after enqueueing; ordered like every other launch on that
 * stream, behind the commits made so far; the fence is Fence::wait (src/graphics/fence.rs:8-42) for the whole context.
 * An entity can be stepped when every extent is finite, > 0 and <= 8 (the reference divides by ceil(extent); the fan has
 * (ceil(extent) + 1) points per axis). Host memory: a record that cannot makes the call return VX_ERR_INVALID_ARGUMENT, which names its
 * index, with nothing changed. Device memory: the kernel leaves such a record's bytes as they are and writes -1 contacts for it. */
int vx_physics_step(vx_context* ctx, vx_entity* entities, uint32_t count, int memory, float delta_time, uint32_t steps,
                    vx_aabb_result* contacts);
/* svo.test.glsl (assets/shaders/svo.test.glsl:63-76): one ray with a StackFrame per loop iteration.
 * n_frames receives the number of iterations (may exceed max_frames). Host pointers. */
int vx_debug_trace(vx_context* ctx, const float pos[3], const float dir[3], float max_dst, int cast_translucent, vx_result* result,
                   vx_frame* frames, uint32_t max_frames, uint32_t* n_frames);
/* Fence::wait for everything enqueued on this context (src/graphics/fence.rs:8-42). */
int vx_sync(vx_context* ctx);
/* Frames in flight. vx_render of an image (no hit records) into DEVICE memory returns after enqueueing and consecutive
 * frames rotate over a few internal streams (two by default), so that frame k+1 starts on the compute units frame k's last rays leave
 * idle. Two calls order such a render against the caller's own streams:
 *   vx_wait_event(ctx, e)           the NEXT vx_render waits for the hipEvent_t `e` (e.g. "the buffer I am about to
 *                                   render into has been consumed"); one-shot
 *   vx_stream_wait_render(ctx, s)   the caller's hipStream_t `s` waits for the most recently issued vx_render
 * vx_sync waits for everything; vx_commit orders uploads after every frame in flight (Svo::update's fence, svo.rs:178). */
/* 1 = every render on the context's stream again; 2 (default) .. 8 = that many frame streams in rotation. More frames in
 * flight hide more of each frame's tail, which matters when a context renders only a share of the tiles (multi-GPU:
 * an eighth of a 1080p frame takes 0.24 ms per frame with 1, 0.085 ms with 3, 0.068 ms with 4 or more frames in flight). */
int vx_set_frames_in_flight(vx_context* ctx, int frames);
int vx_wait_event(vx_context* ctx, void* hip_event);
int vx_stream_wait_render(vx_context* ctx, void* stream);

/* ---- pipelined presentation --------------------------------------------------------------------------------- */

/* For an embedder that shows every frame (the reference blits its framebuffer, src/gamelogic/world.rs:269-283): vx_present_begin
 * enqueues the frame on one of the frame streams and its read-back into pinned host memory on a copy stream behind it, and
 * returns a slot (0..3, in rotation); vx_present_wait blocks until that slot's image is in place and returns it (valid until the
 * slot comes round again, i.e. for the next three vx_present_begin calls). Begin frame k+1, then wait for frame k: the read-back
 * of one frame runs beside the kernel of the next. */
int vx_present_begin(vx_context* ctx, const vx_uniforms* uniforms, uint32_t width, uint32_t height, int format, int* out_slot);
int vx_present_wait(vx_context* ctx, int slot, const void** pixels, size_t* bytes);

/* ---- multi-GPU: tiles, gather, assembly ------------------------------------------------------------------------- */

/* The shared sequence of an image's tiles: out[j] = row-major id (ty * tiles_x + tx, from the bottom-left) of the tile at place j
 * of the Morton order. Returns the number of tiles; fills `out` when capacity suffices. Pure host function. */
uint32_t vx_tile_order(uint32_t width, uint32_t height, uint32_t* out, uint32_t capacity);

/* Which RCCL to open: by default the library is opened by its soname (librccl.so.1: the copy the process already has loaded, if any) when the
 * first communicator is asked for. A deployment that ships its own build -- and the tests, whose stand-in lets several ranks share one GPU
 * (tests/stub_rccl) -- names the file here, before the first vx_comm_* call. Process-wide. No counterpart in the reference (one GL context). */
int vx_comm_library(const char* path);
/* The handle owns the RCCL communicator the finished tiles travel over (SURVEY.md 8b "Ownership"; one process per GPU):
 *   vx_comm_unique_id   on ONE rank: a fresh 128-byte id (ncclGetUniqueId), which the caller hands to every rank by its own means
 *   vx_comm_init        on every rank, collectively: ncclCommInitRank on this context's device
 *   vx_gather_tiles     the one exchange step of the path: this rank's compact tile list (`bytes_per_rank` bytes of device
 *                       memory, the same on every rank) goes to `root`, which receives rank r's list at gathered + r *
 *                       bytes_per_rank (the root's own list is copied there unless it already is there:
 *                       tiles == gathered + root * bytes_per_rank) -- grouped ncclSend / ncclRecv, every peer straight to the root over its own xGMI link, on
 *                       the communicator's stream and ordered behind every vx_render issued so far (the list's among them). Returns
 *                       after enqueueing; *out_ticket (optional) names the gather for vx_wait_gather
 *   vx_wait_gather      the NEXT vx_render waits (on the device) for that gather: call it before rendering into a tile list a
 *                       gather may still be reading
 *   vx_comm_stream      the communicator's hipStream_t: vx_assemble_tiles_on(.., vx_comm_stream(ctx)) is ordered behind the gather
 * RCCL is opened at run time (dlopen of librccl.so.1) by the first of these calls; a single-GPU deployment needs none. */
#define VX_COMM_ID_BYTES 128
int vx_comm_unique_id(void* out_id, size_t bytes);
int vx_comm_init(vx_context* ctx, int nranks, int rank, const void* unique_id);
int vx_comm_destroy(vx_context* ctx);
int vx_comm_info(const vx_context* ctx, int* nranks, int* rank);
/* Wave slots per CU that a context with a communicator of more than one rank leaves to RCCL's own workgroups (its persistent render waves would
 * otherwise fill every CU's LDS, and a communication kernel would find room only when a whole frame has drained). 0 .. 8; default 4 (or
 * VX_COMM_HEADROOM at vx_create). Read by the next render: a caller can time a few frames at each setting and keep the best (bench.py does,
 * at world_size > 1). No counterpart in the reference (one GL context, src/graphics/svo.rs:196-229). */
int vx_set_comm_headroom(vx_context* ctx, int waves_per_cu);
int vx_gather_tiles(vx_context* ctx, const void* tiles, uint64_t bytes_per_rank, void* gathered, int root, int* out_ticket);
int vx_wait_gather(vx_context* ctx, int ticket);
/* Has that gather (and an assembly issued behind it on the communicator's stream: see vx_assemble_tiles_format) finished? 1 = yes,
 * 0 = not yet, -1 = bad ticket or a device error. Never blocks: a caller that must not hang on a collective a peer never joins polls
 * this against a deadline instead of calling vx_sync. */
int vx_gather_query(vx_context* ctx, int ticket);
void* vx_comm_stream(vx_context* ctx);
/* One sharded frame in ONE call -- what a rank does per frame, in the order it has to be done: vx_wait_gather(wait_ticket) unless wait_ticket < 0 (the
 * exchange that last read this tile list), vx_render of this rank's tiles into `target` (device memory; tile_rank / tile_count / format as for
 * vx_render), vx_gather_tiles of the list (bytes_per_rank of it) to `root`, and, on the root, vx_assemble_tiles_format of the gathered lists
 * (`gathered`: [ranks][bytes_per_rank]; the root's own list should be target->rgba32f = gathered + root * bytes_per_rank: rendered in place)
 * into `image` on the communicator's stream (image NULL: no assembly). *out_ticket names the exchange (and covers the assembly). Saves the
 * caller three of four trips through the ABI: at eight ranks a rank's share of a 1080p frame is 0.03 ms of GPU time, and a frame loop
 * that spends longer than that per frame on calls is the bound (bench.py's host_issue_ms_per_step). The reference has no counterpart. */
int vx_render_gather(vx_context* ctx, const vx_uniforms* uniforms, uint32_t width, uint32_t height, const vx_target* target, uint64_t bytes_per_rank,
                     void* gathered, int root, void* image, int wait_ticket, int* out_ticket);
/* vx_assemble_tiles for either pixel format: stride in PIXELS between the ranks' lists; an RGBA8 image comes out top row first.
 * Issued on vx_comm_stream(ctx), it extends the ticket of every gather issued since the last assembly on that stream: vx_wait_gather(ticket)
 * then also waits for this kernel, which reads every rank's list -- the root's own included, which the root renders into in place. Lists and
 * image must be aligned to a pixel (16 bytes RGBA32F, 4 bytes RGBA8). */
int vx_assemble_tiles_format(vx_context* ctx, const void* tiles, uint64_t stride_pixels, uint32_t tile_count, uint32_t width, uint32_t height, void* out,
                             int format, void* stream);

/* Scatters `tile_count` gathered compact tile lists (rank r's list at tiles + r*stride_floats) into a
 * width*height RGBA32F image; all pointers are device memory on this context's device. */
int vx_assemble_tiles(vx_context* ctx, const float* tiles, uint64_t stride_floats, uint32_t tile_count, uint32_t width, uint32_t height,
                      float* out_rgba32f);
/* The same on a caller-supplied hipStream_t (e.g. the stream the gather ran on, so that the context's own stream is free to
 * render the next frame meanwhile); NULL = the legacy default stream. */
int vx_assemble_tiles_on(vx_context* ctx, const float* tiles, uint64_t stride_floats, uint32_t tile_count, uint32_t width, uint32_t height,
                         float* out_rgba32f, void* stream);
/* The traversal image of a world: the octant tree a context traverses instead of the world's own bytes.
 * `world_frame` = the world as committed ([f32 scale][ESVO: 5-word preamble | CSVO: u32 root_ptr][arena]), `used_bytes` = arena
 * bytes in use. layout 1 = what the renderer walks ([64-byte header][octants: a {pointer | value, masks} entry per EXISTING child, child 7
 * first, or just the existing children's values when every child is a voxel -- behind a unit that says where the node lies in a CSVO world's bytes], everything
 * addressed in 8-byte units); layout 2 = the same bytes, walked through a 64-bit pointer instead of a buffer resource: what the renderer switches to when
 * the image outgrows 4 GiB; layout 0 = the same tree as an ESVO frame ([f32 2^-depth][5-word preamble][12-word octants], esvo.rs:74-101),
 * which any ESVO traversal can walk (the tests do, with the oracle). Returns the image size in 32-bit words (0 = cannot be
 * imaged) and fills `out_words` when it is large enough. Pure host function (no device needed): vx_commit does this itself. */
uint64_t vx_traversal_image(int svo_type, const uint8_t* world_frame, uint64_t used_bytes, int layout, uint32_t* out_words, uint64_t capacity_words);
/* Rounds 3-5 kept an ORIGIN TABLE beside the image of a CSVO world and this call returned it. Since round 6 the origin of a voxel-parent octant -- where
 * that node (a leaf-mask byte, svo.csvo.glsl:114-115) lies in the world's own bytes: [0] = its byte pointer, [1] = k << 29 | (pointer - the chunk's material
 * section), k = its place among its depth-2 parent's leaf-mask bytes -- is the 8-byte unit of the image in front of the octant's values, and this call is
 * vx_traversal_image (nothing is written to `out_origin_words`). The renderer consults the origin when a ray that started inside a voxel is led into it
 * (svo.csvo.glsl:293-295): that walk is format specific and is made on the world's bytes. */
uint64_t vx_traversal_image_with_origin(int svo_type, const uint8_t* world_frame, uint64_t used_bytes, int layout, uint32_t* out_words,
                                        uint64_t capacity_words, uint32_t* out_origin_words, uint64_t origin_capacity_words);
/* 2x2 ordered-grid supersampling (BASELINE.json C5): box-filters a (2*width) x (2*height) RGBA32F render down to
 * width x height, both in device memory, on the caller's hipStream_t (NULL = legacy default stream). Render the large
 * image with vx_render first (order it with vx_stream_wait_render). */
int vx_resolve_2x2(vx_context* ctx, const float* src_rgba32f, uint32_t width, uint32_t height, float* dst_rgba32f, void* stream);
/* Number of tiles (32x32) rank `tile_rank` of `tile_count` owns for a width x height image. */
uint32_t vx_local_tile_count(uint32_t width, uint32_t height, uint32_t tile_rank, uint32_t tile_count);

/* ---- measurement ------------------------------------------------------------------------------------------ */

/* Instrumented variant of vx_render (same rays, per-phase step counters, no image kept). */
int vx_render_counters(vx_context* ctx, const vx_uniforms* uniforms, uint32_t width, uint32_t height, uint32_t tile_rank, uint32_t tile_count,
                       vx_counters* out);
/* While enabled, every render-kernel launch is bracketed by HIP events on the stream it is launched on. */
int vx_profile_enable(vx_context* ctx, int enabled);
/* Sum of the bracketed kernel durations (ms) and their count since the last call; synchronises. */
int vx_profile_read(vx_context* ctx, double* kernel_ms_sum, uint32_t* launches);
/* The shader clock the device runs at while this call lasts, in MHz: a one-lane kernel on a stream of its own, beside whatever the context
 * has in flight, compares the shader-clock counter with the device's constant 100 MHz counter over `microseconds` (10 .. 100000). Blocks the
 * calling thread until the probe has run; may be called from a second thread while the context's own thread renders (it takes the
 * context's lock only to launch). No counterpart in the reference: bench.py samples it during its sustained block. */
int vx_clock_probe(vx_context* ctx, uint32_t microseconds, double* shader_mhz);
/* The same for the exchanges (vx_gather_tiles calls made while profiling was enabled): time on the communicator's stream from the
 * first send / receive to the last, i.e. including the wait for the slowest peer. Synchronises the communicator's stream. */
int vx_comm_profile_read(vx_context* ctx, double* gather_ms_sum, uint32_t* gathers);
/* Measurement (contexts created with VX_TIMELINE=1 in the environment by the library's timeline build, lib/lib_tl; else returns 0): per wave of the most recent render launch
 * EIGHT words -- [0] when it started, [1] when it found the sub-tile queue empty, [2] when it left (all in 10 ns ticks of the device's
 * constant clock), [3] sub-tiles taken | service phases << 20 | ticks spent in them << 32, [4] its life in shader-clock cycles
 * (s_memtime: [4] / ([2] - [0]) x 100 MHz is the clock the kernel ran at), [5] the cycles of it spent in the traversal loop, [6] the
 * loop's trips | those in which every traversing lane ADVANCEd << 20 | those in which every one PUSHed << 40 (20 bits each), [7] the walks inside voxels (images of CSVO worlds): walk phases << 52 | trips of the walk's loop << 32 | shader-clock cycles
 * in the walks. `out` holds capacity_waves x 8 words. Returns the number of waves copied. Waits for every frame in flight. */
uint32_t vx_timeline_read(vx_context* ctx, uint64_t* out, uint32_t capacity_waves);
/* What vx_render walks after the last commit: [0] 0 = the world's own bytes (no image: switched off, or the world cannot be
 * imaged), 1 = the traversal image walked through a buffer resource, 2 = walked through a 64-bit pointer (images beyond 4 GiB);
 * [1] bytes of the image, [2] 0 (rounds 3-5: bytes of a CSVO world's origin table; the origins are units of the image now), [3] chunks it holds. */
int vx_image_info(const vx_context* ctx, uint64_t out[4]);
/* The scheduling knobs this context runs with (they reorder a frame's work and change no pixel): [0] refill threshold, [1] service threshold, [2] cap on
 * the persistent waves per CU (0 = none), [3] length of the sub-tile queue's stretches (0 = by the launch), [4] width of the tile numbering's strips, [5] cost-ordered
 * queue on / off, [6] wave slots per CU left to RCCL (vx_set_comm_headroom), [7] bit 0 = this is the library's measurement build (the only one that reads the
 * VX_REFILL_MIN / VX_WAVES_PER_CU / VX_QUEUE_STRIPE / VX_TILE_STRIP / VX_HOT_FIRST environment variables), bit 1 = whole frames run the render kernel's
 * whole-frame build (VX_PLAIN_FRAME, default on). For the tests. */
int vx_debug_knobs(const vx_context* ctx, uint32_t out[8]);
/* CSVO worlds rendered from their traversal image: since creation (or the last reset), [0] rays that were led into the voxel they
 * started in and made that walk on the world's own bytes, [1] those of them whose pixel was rendered again on the bytes (the walk
 * overwrote cursor state the rest of the ray depends on), [2] service phases of the render kernel that ran such walks (the rays of a
 * wave go together), [3] loop iterations made on the world's own bytes. Waits for every frame in flight. Counting costs frame time (atomics
 * on one line from every wave) and is OFF until asked for: reset = 1 zeroes the counters and counts from now on, 2 zeroes them and stops
 * counting, 0 only reads. */
int vx_excursion_counters(vx_context* ctx, uint64_t out[4], int reset);
/* hipStream_t the context launches on (as void*), for callers that order their own work after it. */
void* vx_stream(vx_context* ctx);
int vx_device(const vx_context* ctx);

const char* vx_last_error(void);
const char* vx_version(void);

#ifdef __cplusplus
}
#endif
#endif

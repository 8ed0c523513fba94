// What blocks_runtime.cpp knows of the kernels of csrc/blocks (kernels_*.hip): one launcher a kernel, with what it asks of its arguments.
#pragma once

#include <hip/hip_runtime_api.h>

#include "vx_args.hpp"
#include "vx_blocks.hpp"
#include "vx_boxes.hpp"
#include "vx_distance.hpp"
#include "vx_flood.hpp"
#include "vx_label.hpp"
#include "vx_light.hpp"
#include "vx_list.hpp"
#include "vx_move.hpp"
#include "vx_scan.hpp"
#include "vx_walk.hpp"

namespace vxk {

// ceil(count / 64) workgroups of one wave, one point a lane: a float[3] at pos + i * pos_stride (4-byte aligned, stride >= 12);
// out: `count` records of device-visible memory, 8-byte aligned, that overlaps no input
hipError_t launch_block_points(int svo, hipStream_t stream, const vxd::SceneArgs& sc, const void* pos, uint32_t pos_stride, uint32_t count, vx_block_cell* out);

// one workgroup of one wave a brick of `r` (vxb::plan_region of a box of at least one and at most 2^24 voxels); out: the box's voxels, x
// fastest, in device-visible memory
hipError_t launch_read_region(int svo, hipStream_t stream, const vxd::SceneArgs& sc, const vxb::Region& r, uint32_t* out);

// ceil(count / 64) workgroups of one wave, one position a lane, read as launch_block_points reads it; direction 0..5, reach >= 1;
// out: `count` records of device-visible memory, 16-byte aligned, that overlaps no input
hipError_t launch_scan_points(int svo, hipStream_t stream, const vxd::SceneArgs& sc, const void* pos, uint32_t pos_stride, uint32_t count, int direction,
                              uint32_t reach, vx_scan_hit* out);

// one workgroup of one wave a tile of `p` (vxb::plan_columns of a box that holds a voxel, at most 2^24 columns); out: the footprint's
// records, u fastest, in device-visible memory, 16-byte aligned
hipError_t launch_scan_columns(int svo, hipStream_t stream, const vxd::SceneArgs& sc, const vxb::Columns& p, vx_scan_hit* out);

// vx_list_region's three launches (kernels_list.hip), in this order on one stream. `r`: vxb::plan_region of a box of at least one and at most
// 2^24 voxels; counts: vxb::region_bricks(r) + 1 dwords of device memory, 16-byte aligned, which the three launches own from the first
// one's start to the last one's end.
//   count: one workgroup of one wave a brick; counts[brick] = the records the brick gives under `flags`
//   offsets: one workgroup; an exclusive prefix sum over counts[0..bricks) in place, counts[bricks] = *total = the sum (total: device-visible)
//   write: one workgroup of one wave a brick; the brick's records to out[counts[brick]...], those below `capacity`; out: device-visible,
//   8-byte aligned
hipError_t launch_list_count(int svo, hipStream_t stream, const vxd::SceneArgs& sc, const vxb::Region& r, uint32_t flags, uint32_t* counts);
hipError_t launch_list_offsets(hipStream_t stream, uint32_t* counts, uint32_t bricks, uint32_t* total);
hipError_t launch_list_write(int svo, hipStream_t stream, const vxd::SceneArgs& sc, const vxb::Region& r, uint32_t flags, uint32_t* counts, vx_block_at* out,
                             uint32_t capacity);

// `count` (1..2^24) workgroups of one wave, one box a wave: float[3]s at origin + i * origin_stride, offset + i * offset_stride (offset may be
// null: no add) and extents + i * extents_stride (4-byte aligned; strides multiples of 4, >= 12, offset's and extents' may be 0 = one vector for
// every box); only_value: 0 = every block counts; out: `count` records of device-visible memory, 16-byte aligned, that overlaps no input
hipError_t launch_overlap_boxes(int svo, hipStream_t stream, const vxd::SceneArgs& sc, const void* origin, const void* offset, const void* extents,
                                uint32_t origin_stride, uint32_t offset_stride, uint32_t extents_stride, uint32_t only_value, uint32_t count,
                                vx_box_hit* out);

// `count` (1..2^24) workgroups of one wave, one box a wave: the boxes as launch_overlap_boxes reads them, a float[3] at motion + i *
// motion_stride (4-byte aligned; the stride a multiple of 4 and >= 12, or 0 = one motion for every box); shape: within vxb::check_move's
// rules; out: `count` records of device-visible memory, 16-byte aligned, that overlaps no input
hipError_t launch_move_boxes(int svo, hipStream_t stream, const vxd::SceneArgs& sc, const void* origin, const void* offset, const void* extents,
                             const void* motion, uint32_t origin_stride, uint32_t offset_stride, uint32_t extents_stride, uint32_t motion_stride,
                             uint32_t only_value, const vx_move_shape& shape, uint32_t count, vx_move_hit* out);

// `count` (1..2^24) workgroups of 256 threads, one query a workgroup: a float[3] at pos + i * pos_stride, read as launch_block_points reads it;
// shape: within vxb::check_flood's rules (refused here too: the kernel indexes LDS by it); fields (may be null: records only): 16-byte aligned,
// query i's bytes at fields + i * field_stride, field_stride a multiple of 16 and at least the voxel count, of which the voxel count rounded
// up to 16 are written; info (may be null, not both): `count` records, 16-byte aligned. Device-visible memory that overlaps no input.
hipError_t launch_flood_points(int svo, hipStream_t stream, const vxd::SceneArgs& sc, const void* pos, uint32_t pos_stride, uint32_t count, const vx_flood_shape& shape,
                               uint8_t* fields, uint32_t field_stride, vx_flood_info* info);

// `count` (1..2^24) workgroups of 256 threads, one box a workgroup: an int32[3] at lo + i * lo_stride (4-byte aligned, the stride a multiple of
// 4 and at least 12); size, flags: within vxb::check_light's rules (refused here too: the kernel indexes LDS by them); props: the table as the
// kernel reads it, VX_LIGHT_MAX_PROPS bytes, 4-byte aligned, zeros behind props_count; fields (may be null: records only): 16-byte aligned,
// box i's bytes at fields + i * field_stride, field_stride a multiple of 16 and at least the voxel count, of which the voxel count rounded up
// to 16 are written; info (may be null, not both): `count` records, 16-byte aligned. Device-visible memory that overlaps no input.
hipError_t launch_light_boxes(int svo, hipStream_t stream, const vxd::SceneArgs& sc, const void* lo, uint32_t lo_stride, uint32_t count, const uint32_t size[3],
                              uint32_t flags, const void* props, uint8_t* fields, uint32_t field_stride, vx_light_info* info);

// `count` (1..2^24) workgroups of 256 threads, one query a workgroup: positions as launch_flood_points reads them; goal (may be null: no goal):
// a float[3] at goal + i * goal_stride, goal_stride 0: one for all; shape: within vxb::check_walk's rules (refused here too: the kernel
// indexes LDS by it); fields as launch_flood_points'; paths (may be null; ignored without a goal or with path_capacity == 0): 16-byte
// aligned, query i's shape.path_capacity entries at paths + i * shape.path_capacity; info (may be null, not all three): `count` records of 32
// bytes, 16-byte aligned. Device-visible memory that overlaps no input.
hipError_t launch_walk_points(int svo, hipStream_t stream, const vxd::SceneArgs& sc, const void* pos, uint32_t pos_stride, const void* goal, uint32_t goal_stride,
                              uint32_t count, const vx_walk_shape& shape, uint8_t* fields, uint32_t field_stride, uint32_t* paths, vx_walk_info* info);

// `count` (1..2^20) workgroups of 256 threads, one box a workgroup: an int32[3] at lo + i * lo_stride (4-byte aligned, the stride a multiple of
// 4 and at least 12); shape: within vxb::check_label's rules (refused here too: the kernel indexes LDS by its size and ends its loops by
// max_steps and max_pieces); fields as launch_flood_points'; pieces (may be null; not with shape.max_pieces == 0): 16-byte aligned, box i's
// shape.max_pieces records at pieces + i * shape.max_pieces, all of them written; info (may be null, not all three): `count` records of 32
// bytes, 16-byte aligned. Device-visible memory that overlaps no input.
hipError_t launch_label_boxes(int svo, hipStream_t stream, const vxd::SceneArgs& sc, const void* lo, uint32_t lo_stride, uint32_t count, const vx_label_shape& shape,
                              uint8_t* fields, uint32_t field_stride, vx_label_piece* pieces, vx_label_info* info);

// `count` (1..2^20) workgroups of 256 threads, one box a workgroup: an int32[3] at lo + i * lo_stride (4-byte aligned, the stride a multiple of
// 4 and at least 12); shape: within vxb::check_distance's rules (refused here too: the kernel indexes LDS by its size); fields (may be null:
// records only): 16-byte aligned, box i's entries at (uint8_t*)fields + i * field_stride, field_stride in bytes, a multiple of 16 and at least
// twice the voxel count, of which twice the voxel count rounded up to 16 are written; info (may be null, not both): `count` records of 16
// bytes, 16-byte aligned. Device-visible memory that overlaps no input.
hipError_t launch_distance_boxes(int svo, hipStream_t stream, const vxd::SceneArgs& sc, const void* lo, uint32_t lo_stride, uint32_t count,
                                 const vx_distance_shape& shape, uint16_t* fields, uint32_t field_stride, vx_distance_info* info);

}  // namespace vxk

// What blocks_runtime.cpp knows of the block lookup kernels (kernels_blocks.hip) and of the scans along an axis (kernels_scan.hip).
#pragma once

#include <hip/hip_runtime_api.h>

#include "vx_args.hpp"
#include "vx_blocks.hpp"
#include "vx_scan.hpp"

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

}  // namespace vxk

// What blocks_runtime.cpp knows of the block lookup kernels (kernels_blocks.hip).
#pragma once

#include <hip/hip_runtime_api.h>

#include "vx_args.hpp"
#include "vx_blocks.hpp"

namespace vxk {

// ceil(count / 64) workgroups of one wave, one point a lane: a float[3] at pos + i * pos_stride (4-byte aligned, stride >= 12);
// out: `count` records of device-visible memory, 8-byte aligned, that overlaps no input
hipError_t launch_block_points(int svo, hipStream_t stream, const vxd::SceneArgs& sc, const void* pos, uint32_t pos_stride, uint32_t count, vx_block_cell* out);

// one workgroup of one wave a brick of `r` (vxb::plan_region of a box of at least one and at most 2^24 voxels); out: the box's voxels, x
// fastest, in device-visible memory
hipError_t launch_read_region(int svo, hipStream_t stream, const vxd::SceneArgs& sc, const vxb::Region& r, uint32_t* out);

}  // namespace vxk

// What raycast_runtime.cpp knows of the ray batch kernel (kernels_raycast.hip).
#pragma once

#include <hip/hip_runtime_api.h>

#include "vx_args.hpp"

namespace vxk {

// A vx_ray_batch as the kernel takes it: device-visible pointers, strides in bytes (0 = one value for every ray; the runtime has checked
// them). has_max_dst = 0: max_dst is not read and every ray gets max_dst_all. translucent picks the kernel: cast_translucent is a
// constant of its code.
struct RayBatchArgs {
    const void* origin;
    const void* dir;
    const void* max_dst;
    uint32_t origin_stride, dir_stride, max_dst_stride;
    float max_dst_all;
    uint32_t has_max_dst;
    uint32_t translucent;
};

// ceil(count / 64) workgroups of one wave, one ray a lane; hits: `count` records of device-visible memory that overlaps no input
hipError_t launch_raycast_batch(int svo, hipStream_t stream, const vxd::SceneArgs& sc, const RayBatchArgs& rays, uint32_t count, vx_ray_hit* hits);

}  // namespace vxk

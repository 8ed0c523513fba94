// What raycast_runtime.cpp knows of the ray batch kernel (kernels_raycast.hip).
#pragma once

#include <hip/hip_runtime_api.h>

#include "vx_args.hpp"
#include "vx_ray_batch.hpp"

namespace vxk {

// ceil(count / 64) workgroups of one wave, one ray a lane; rays: vx_ray_batch.hpp's; hits: `count` records of device-visible memory that overlaps no input
hipError_t launch_raycast_batch(int svo, hipStream_t stream, const vxd::SceneArgs& sc, const RayBatchArgs& rays, uint32_t count, vx_ray_hit* hits);

}  // namespace vxk

// What trace_runtime.cpp knows of the shaded ray batch kernel (kernels_trace.hip).
#pragma once

#include <hip/hip_runtime_api.h>

#include "kernels_raycast.h"
#include "vx_args.hpp"

namespace vxk {

// ceil(count / 64) workgroups of one wave, one ray a lane. `rays` as for launch_raycast_batch (vx_ray_batch.hpp; its `translucent` is not read: trace_ray casts
// translucent, world.glsl:29). rgba (`count` pixels in `format`: 16 bytes each, or 4) and hits (`count` records) are device-visible memory that
// overlaps no input, aligned to 16 bytes (RGBA8 pixels: 4); either may be null, not both.
hipError_t launch_trace_rays(int svo, hipStream_t stream, const vxd::SceneArgs& sc, const vx_uniforms& uniforms, const RayBatchArgs& rays, uint32_t count,
                             void* rgba, int format, vx_hit* hits);

}  // namespace vxk

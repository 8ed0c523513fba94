// What physics_runtime.cpp knows of the physics kernel (kernels_physics.hip).
#pragma once

#include <hip/hip_runtime_api.h>

#include "vx_args.hpp"

namespace vxk {

// `count` workgroups of one wave; entities / contacts: device-visible memory (contacts may be null)
hipError_t launch_physics(int svo, hipStream_t stream, const vxd::SceneArgs& sc, vx_entity* entities, uint32_t count, float delta_time, uint32_t steps,
                          vx_aabb_result* contacts);

}  // namespace vxk

// vx_physics_step's limits and the rule for a record that can be stepped: ONE statement of them for the runtime's host check
// (physics_runtime.cpp) and the kernel's (vx_physics.hpp). Plain constexpr C++: usable from host and device code alike.
#pragma once

#include <stdint.h>

namespace vxp {

constexpr float kMaxExtent = 8.0f;            // the largest box edge (9 grid points an axis, 2,187 slots at most)
constexpr uint32_t kMaxSteps = 1024;          // steps of one call
constexpr uint32_t kMaxEntities = 1u << 24;   // entities of one call (one workgroup each: far inside the grid's limit; 1 GiB of records)

// every extent finite, > 0 and <= kMaxExtent (NaN fails every comparison, +inf the second): the reference divides by ceil(extent)
// (svo_picker.rs:184-195), and the fan has ceil(extent) + 1 points an axis
constexpr bool steppable_extents(const float extents[3]) {
    return extents[0] > 0.0f && extents[0] <= kMaxExtent && extents[1] > 0.0f && extents[1] <= kMaxExtent && extents[2] > 0.0f && extents[2] <= kMaxExtent;
}

}  // namespace vxp

// What views_runtime.cpp knows of the many-views kernel (kernels_views.hip).
#pragma once

#include <hip/hip_runtime_api.h>

#include "vx_args.hpp"
#include "vx_view_params.hpp"

namespace vxk {

// count * ceil(width / 8) * ceil(height / 8) workgroups of one wave, each an 8 x 8 tile of one view. `views`: `count` records in device-visible
// memory, aligned to 16 bytes, valid until the launch has ended. rgba (count * width * height pixels in `format`: 16 bytes each, or 4) and hits
// (as many records) are device-visible memory, aligned to 16 bytes (RGBA8 pixels: 4); either may be null, not both. `format` decides the row
// order of both (vx_render's: RGBA8 has the top row first). count * width * height <= 2^24.
hipError_t launch_trace_views(int svo, hipStream_t stream, const vxd::SceneArgs& sc, const vxd::ViewParams* views, uint32_t count, uint32_t width,
                              uint32_t height, void* rgba, int format, vx_hit* hits);

}  // namespace vxk

// One camera of vx_trace_views' table (kernels_views.hip), shared by views_runtime.cpp, which fills it, and vx_views.hpp, which reads it. Plain
// data and host code, no HIP header: the host test harness compiles it.
#pragma once

#include <cmath>

#include "vx_args.hpp"

namespace vxd {

// A view's uniforms and what primary_ray needs of a camera beside them: what RenderParams holds of a camera without what it holds of a launch.
// 144 bytes, read through wave-uniform addresses.
struct ViewParams {
    vx_uniforms u;
    float tan_half_fovy;
    float ray_origin[3];
    uint32_t affine_view;
    uint32_t _pad;
};
static_assert(sizeof(ViewParams) == 144, "a multiple of 16 bytes");

// The three camera constants, evaluated on the HOST: the device's tanf is not the host's, and a view's rays are vx_render's bit for bit only
// when these are. They are fill_params' three lines (csrc/hip/runtime.cpp: p.tan_half_fovy, view_origin, p.affine_view), stated a second
// time so that csrc/hip, on whose bytes the committed counter files are keyed (_pkg.csrc_hash), stays as it is: change both together.
inline ViewParams view_params_of(const vx_uniforms& u) {
    ViewParams v = {};
    v.u = u;
    v.tan_half_fovy = tanf(u.fovy * 0.5f);
    view_origin(u.view, v.ray_origin);
    v.affine_view = (u.view[3] == 0.0f && u.view[7] == 0.0f && u.view[11] == 0.0f && u.view[15] == 1.0f && std::isfinite(v.tan_half_fovy) &&
                     std::isfinite(u.aspect)) ? 1u : 0u;
    return v;
}

}  // namespace vxd

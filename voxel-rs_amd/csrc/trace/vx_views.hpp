// vx_trace_views' per-lane code: world.glsl:110-141 -- main: the pixel's primary ray (:110-129), trace_ray or the sky (:132-138), the store (:140) -- for
// one pixel of one of many small views. The ray is primary_ray's (vx_device.hpp), from camera constants the host evaluated per view
// (vx_view_params.hpp: view_params_of); what becomes of it is vx_trace.hpp's three steps and finish, with no limit on the primary cast. So a pixel's
// colour and vx_hit are vx_render's for that view, the record bit for bit. A workgroup is 64 lanes on one 8 x 8 tile of one view; which view
// and which tile follows from the workgroup's number alone. Device code; tests/cpp/views_on_host.cpp compiles it for the host.
#pragma once

#include "vx_trace.hpp"
#include "vx_view_params.hpp"

namespace vxv {

using namespace vxd;

constexpr uint32_t kViewTile = 8;  // pixels per edge of a workgroup's tile

// A launch's workgroups: view after view, a view's tiles row by row from the bottom left
inline uint32_t tiles_across(uint32_t pixels) { return (pixels + kViewTile - 1u) / kViewTile; }

// The pixel of lane `lane` of workgroup `block`: rows of eight lanes, so a wave stores eight runs of eight adjacent pixels. x or y may lie outside
// the image in the tiles of its right and top edges.
struct Pixel {
    uint32_t view, x, y;
};
__device__ __forceinline__ Pixel pixel_of(uint32_t block, uint32_t lane, uint32_t tiles_x, uint32_t tiles_per_view) {
    Pixel px;
    px.view = block / tiles_per_view;
    const uint32_t tile = block - px.view * tiles_per_view, ty = tile / tiles_x, tx = tile - ty * tiles_x;
    px.x = tx * kViewTile + (lane & (kViewTile - 1u));
    px.y = ty * kViewTile + lane / kViewTile;
    return px;
}

// What primary_ray, shade_primary, apply_light and image_index read of RenderParams: the view's record, the size and format all views share
__device__ __forceinline__ RenderParams params_of(const ViewParams& v, uint32_t width, uint32_t height, uint32_t rgba8) {
    RenderParams p = {};
    p.u = v.u;
    p.tan_half_fovy = v.tan_half_fovy;
    p.ray_origin[0] = v.ray_origin[0]; p.ray_origin[1] = v.ray_origin[1]; p.ray_origin[2] = v.ray_origin[2];
    p.affine_view = v.affine_view;
    p.width = width;
    p.height = height;
    p.rgba8 = rgba8;
    return p;
}

// Where a pixel and its record go: view k's image at k * width * height, inside it vx_render's place for a whole-image target of that format
__device__ __forceinline__ size_t out_index(const RenderParams& p, uint32_t view, uint32_t x, uint32_t y) {
    return size_t(view) * (p.width * p.height) + image_index(p, x, y);
}

// world.glsl:110-138 for pixel (x, y) of the view p describes
template <int SVO, class ST>
__device__ __forceinline__ void trace_pixel(const DevScene& sc, const RenderParams& p, uint32_t x, uint32_t y, const ST& st, float color[4], vx_hit& rec) {
    float ro[3], rd[3];
    primary_ray(p, x, y, ro, rd);
    vxt::Traced r;
    vxt::cast_primary<SVO>(sc, ro, rd, -1.0f, st, r);  // 1: every lane
    shade_primary<false>(sc, p, r.res, r.o);           // 2: the lanes that hit
    vxt::cast_shadow<SVO>(sc, p, st, r);               // 3: the lanes that asked for a shadow ray
    vxt::finish(rd, r, color, rec);
}

}  // namespace vxv

// vx_trace_rays' per-ray code: world.glsl:132-138 -- trace_ray (world.glsl:27-90) and, where nothing was hit, get_sky_color (world.glsl:92-108)
// -- for a ray that comes from memory instead of from the camera. Written from vx_device.hpp's device functions and nothing else, in the order
// shade_pixel runs them after its primary_ray call, so a ray that IS a pixel's primary ray gives that pixel's colour and vx_hit bit for bit.
// Three steps, which the kernel runs one after the other for the whole wave (no traversal loop sits inside divergent shading code):
//   1. cast_primary  every lane's primary cast (cast_translucent = true, world.glsl:29), ended by the batch's max_dst
//   2. shade_primary (vx_device.hpp) for the lanes that hit: highlight outline, normal map, diffuse and specular light
//   3. cast_shadow   at most one shadow ray along -light_dir for the lanes that asked for one (never limited), then the light
// and finish() paints the sky for the lanes that hit nothing. Device code; tests/cpp/trace_on_host.cpp compiles it for the host.
#pragma once

#include "vx_device.hpp"

namespace vxt {

using namespace vxd;

// What shade_primary and apply_light read of RenderParams is `u` alone (ambient, light_dir, cam_pos, render_shadows, shadow_distance,
// highlight_pos); view, fovy and aspect describe a camera and a batch has none.
__device__ __forceinline__ RenderParams params_of(const vx_uniforms& u) {
    RenderParams p = {};
    p.u = u;
    return p;
}

// A ray between its steps.
struct Traced {
    Result res;        // the primary cast's
    PrimaryOutcome o;  // what shading made of it
    float shadow_t;    // -1 = unoccluded / not cast
    uint32_t steps;    // loop iterations, primary + shadow
};

// 1. world.glsl:29. A ray its max_dst ends is a miss (t = -1) like one that leaves the octree; max_dst < 0: no limit, the shader's own cast.
template <int SVO, class ST>
__device__ __forceinline__ void cast_primary(const DevScene& sc, const float ro[3], const float rd[3], float max_dst, const ST& st, Traced& r) {
    r.steps = 0;
    r.shadow_t = -1.0f;
    intersect<SVO, false, false, true>(sc, ro, rd, max_dst, true, st, r.res, r.steps, nullptr, nullptr);
}

// 3. world.glsl:79-88 for a lane whose shading asked for a shadow ray; the others keep what shade_primary gave them.
template <int SVO, class ST>
__device__ __forceinline__ void cast_shadow(const DevScene& sc, const RenderParams& p, const ST& st, Traced& r) {
    if (r.o.final_color) return;
    const float neg_l[3] = {-p.u.light_dir[0], -p.u.light_dir[1], -p.u.light_dir[2]};
    Result sres;
    intersect<SVO, false, false, false>(sc, r.o.shadow_origin, neg_l, -1.0f, true, st, sres, r.steps, nullptr, nullptr);
    const bool lit = sres.t < 0.0f;
    if (!lit) r.o.flags |= 4u;
    r.shadow_t = sres.t;
    apply_light(p, r.o.color, r.o.ds, lit ? 1.0f : 0.0f);
}

// world.glsl:135-138: the pixel, and the record vx_render keeps of it
__device__ __forceinline__ void finish(const float rd[3], const Traced& r, float color[4], vx_hit& rec) {
    if (r.res.t == -1.0f) {
        float sky[3];
        sky_color(rd, sky);
        color[0] = sky[0]; color[1] = sky[1]; color[2] = sky[2]; color[3] = 1.0f;
    } else {
        color[0] = r.o.color[0]; color[1] = r.o.color[1]; color[2] = r.o.color[2]; color[3] = r.o.color[3];
    }
    rec.t = r.res.t;
    rec.value = r.res.value;
    rec.face_id = r.res.face_id;
    rec.flags = r.o.flags;
    rec.pos[0] = r.res.pos[0]; rec.pos[1] = r.res.pos[1]; rec.pos[2] = r.res.pos[2];
    rec.lod = r.res.lod;
    rec.uv[0] = r.res.uv[0]; rec.uv[1] = r.res.uv[1];
    rec.shadow_t = r.shadow_t;
    rec.steps = r.steps;
}

// The three steps for one ray, in the kernel's order.
template <int SVO, class ST>
__device__ __forceinline__ void trace_ray(const DevScene& sc, const RenderParams& p, const float ro[3], const float rd[3], float max_dst, const ST& st,
                                          float color[4], vx_hit& rec) {
    Traced r;
    cast_primary<SVO>(sc, ro, rd, max_dst, st, r);
    shade_primary<false>(sc, p, r.res, r.o);
    cast_shadow<SVO>(sc, p, st, r);
    finish(rd, r, color, rec);
}

// A vx_hit as the three 16-byte words it is stored in
__device__ __forceinline__ void hit_words(const vx_hit& h, uint4 w[3]) {
    w[0] = make_uint4(__float_as_uint(h.t), h.value, uint32_t(h.face_id), h.flags);
    w[1] = make_uint4(__float_as_uint(h.pos[0]), __float_as_uint(h.pos[1]), __float_as_uint(h.pos[2]), __float_as_uint(h.lod));
    w[2] = make_uint4(__float_as_uint(h.uv[0]), __float_as_uint(h.uv[1]), __float_as_uint(h.shadow_t), h.steps);
}

}  // namespace vxt

// vx_trace_rays' kernel (gfx950): world.glsl:132-138 -- trace_ray, or the sky -- for a batch of rays read where they lie, gathered through byte
// strides exactly as raycast_batch_kernel gathers them (csrc/raycast/vx_ray_batch.hpp: gather_ray), and answered with a pixel and / or the vx_hit
// record vx_render keeps of a pixel. 64 lanes a workgroup, one ray a lane, on the world's own bytes like the picker path and render_kernel;
// the per-ray code is vx_trace.hpp's. The world is read-only for the whole launch.
#include <hip/hip_runtime.h>

#include "kernels_trace.h"
#include "vx_trace.hpp"

using namespace vxd;

namespace {

// What is written is decided on kernel arguments (out_rgba: 0 none, 1 RGBA32F, 2 RGBA8; out_hits), like the strides: scalar branches, no lane
// looks at a pointer.
template <int SVO>
__global__ __launch_bounds__(64) void trace_rays_kernel(SceneArgs sa, vx_uniforms u, const uint8_t* __restrict__ origin, const uint8_t* __restrict__ dir,
                                                        const uint8_t* __restrict__ max_dst, uint32_t origin_stride, uint32_t dir_stride,
                                                        uint32_t max_dst_stride, float max_dst_all, uint32_t has_max_dst, uint32_t n,
                                                        uint32_t out_rgba, uint32_t out_hits, void* __restrict__ rgba, vx_hit* __restrict__ hits) {
    const DevScene sc = make_scene(sa);
    const RenderParams p = vxt::params_of(u);
    StackSpill spill;
    Stack<64> st;
    st.init(threadIdx.x, &spill);
    const uint32_t i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    float ro[3], rd[3], limit;
    vxk::gather_ray(origin, dir, max_dst, origin_stride, dir_stride, max_dst_stride, max_dst_all, has_max_dst, i, ro, rd, limit);

    vxt::Traced r;
    vxt::cast_primary<SVO>(sc, ro, rd, limit, st, r);  // 1: every lane
    shade_primary<false>(sc, p, r.res, r.o);           // 2: the lanes that hit
    vxt::cast_shadow<SVO>(sc, p, st, r);               // 3: the lanes that asked for a shadow ray
    float color[4];
    vx_hit rec;
    vxt::finish(rd, r, color, rec);

    if (out_rgba == 1u) reinterpret_cast<float4*>(rgba)[i] = make_float4(color[0], color[1], color[2], color[3]);
    else if (out_rgba == 2u) reinterpret_cast<uint32_t*>(rgba)[i] = pack_rgba8(color);
    if (out_hits) {
        uint4 w[3];
        vxt::hit_words(rec, w);
        uint4* out = reinterpret_cast<uint4*>(hits + i);
        out[0] = w[0];
        out[1] = w[1];
        out[2] = w[2];
    }
}

}  // namespace

namespace vxk {

hipError_t launch_trace_rays(int svo, hipStream_t stream, const SceneArgs& sc, const vx_uniforms& u, const RayBatchArgs& r, uint32_t count, void* rgba,
                             int format, vx_hit* hits) {
    static_assert(sizeof(vx_hit) == 48, "three 16-byte stores");
    const size_t lds = Stack<64>::kBytes;
    const dim3 grid((count + 63u) / 64u), block(64);
    const uint8_t *o = static_cast<const uint8_t*>(r.origin), *d = static_cast<const uint8_t*>(r.dir), *m = static_cast<const uint8_t*>(r.max_dst);
    const uint32_t out_rgba = !rgba ? 0u : (format == VX_FORMAT_RGBA8 ? 2u : 1u), out_hits = hits ? 1u : 0u;
#define VX_LAUNCH_TRACE(S)                                                                                                                        \
    hipLaunchKernelGGL((trace_rays_kernel<S>), grid, block, lds, stream, sc, u, o, d, m, r.origin_stride, r.dir_stride, r.max_dst_stride, r.max_dst_all, \
                       r.has_max_dst, count, out_rgba, out_hits, rgba, hits)
    if (svo == VX_SVO_ESVO_BIG) VX_LAUNCH_TRACE(VX_SVO_ESVO_BIG);
    else if (svo == VX_SVO_ESVO) VX_LAUNCH_TRACE(VX_SVO_ESVO);
    else if (svo == VX_SVO_CSVO) VX_LAUNCH_TRACE(VX_SVO_CSVO);
    else return hipErrorInvalidValue;
#undef VX_LAUNCH_TRACE
    return hipGetLastError();
}

}  // namespace vxk

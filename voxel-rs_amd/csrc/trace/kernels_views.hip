// vx_trace_views' kernel (gfx950): world.glsl:110-141 for every pixel of `count` small views in one launch. 64 lanes a workgroup, one 8 x 8 tile of
// one view; the view and the tile's origin come from blockIdx alone, so the view's record (vx_view_params.hpp: ViewParams) is read through wave-uniform
// addresses and no lane chases a pointer to find its camera. One pixel a lane on the world's own bytes, like trace_rays_kernel, whose LDS stack,
// three steps and stores these are; the per-lane code is vx_views.hpp's. The world and the table are read-only for the whole launch.
#include <hip/hip_runtime.h>

#include "kernels_views.h"
#include "vx_views.hpp"

using namespace vxd;

namespace {

// What is written is decided on kernel arguments (out_rgba: 0 none, 1 RGBA32F, 2 RGBA8; out_hits), and so is the row order (rgba8, which holds for
// the records too): scalar branches.
template <int SVO>
__global__ __launch_bounds__(64) void trace_views_kernel(SceneArgs sa, const ViewParams* __restrict__ views, uint32_t width, uint32_t height, uint32_t tiles_x,
                                                         uint32_t tiles_per_view, uint32_t rgba8, uint32_t out_rgba, uint32_t out_hits,
                                                         void* __restrict__ rgba, vx_hit* __restrict__ hits) {
    const DevScene sc = make_scene(sa);
    StackSpill spill;
    Stack<64> st;
    st.init(threadIdx.x, &spill);
    const vxv::Pixel px = vxv::pixel_of(blockIdx.x, threadIdx.x, tiles_x, tiles_per_view);
    if (px.x >= width || px.y >= height) return;  // partial tiles at the right and top edges
    const RenderParams p = vxv::params_of(views[px.view], width, height, rgba8);

    float color[4];
    vx_hit rec;
    vxv::trace_pixel<SVO>(sc, p, px.x, px.y, st, color, rec);

    const size_t i = vxv::out_index(p, px.view, px.x, px.y);
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

hipError_t launch_trace_views(int svo, hipStream_t stream, const SceneArgs& sc, const ViewParams* views, uint32_t count, uint32_t width, uint32_t height,
                              void* rgba, int format, vx_hit* hits) {
    static_assert(sizeof(vx_hit) == 48, "three 16-byte stores");
    const size_t lds = Stack<64>::kBytes;
    const uint32_t tiles_x = vxv::tiles_across(width), tiles_per_view = tiles_x * vxv::tiles_across(height);
    if (uint64_t(count) * tiles_per_view > 0x7fffffffu) return hipErrorInvalidValue;  // (2^24 pixels: at most 2^24 workgroups)
    const dim3 grid(count * tiles_per_view), block(64);
    const uint32_t rgba8 = format == VX_FORMAT_RGBA8 ? 1u : 0u, out_rgba = !rgba ? 0u : (rgba8 ? 2u : 1u), out_hits = hits ? 1u : 0u;
#define VX_LAUNCH_VIEWS(S) \
    hipLaunchKernelGGL((trace_views_kernel<S>), grid, block, lds, stream, sc, views, width, height, tiles_x, tiles_per_view, rgba8, out_rgba, out_hits, rgba, hits)
    if (svo == VX_SVO_ESVO_BIG) VX_LAUNCH_VIEWS(VX_SVO_ESVO_BIG);
    else if (svo == VX_SVO_ESVO) VX_LAUNCH_VIEWS(VX_SVO_ESVO);
    else if (svo == VX_SVO_CSVO) VX_LAUNCH_VIEWS(VX_SVO_CSVO);
    else return hipErrorInvalidValue;
#undef VX_LAUNCH_VIEWS
    return hipGetLastError();
}

}  // namespace vxk

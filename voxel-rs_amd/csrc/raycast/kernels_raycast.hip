// vx_raycast_batch's kernel (gfx950): picker.glsl:30-51 for a batch of rays read where they lie -- origins, directions and distances
// gathered through byte strides (vx_ray_batch.hpp's gather_ray: PickerBatch::add_ray's rays without the std430 PickerTask around them) -- and answered with 32-byte hits
// that keep OctreeResult.value (svo.glsl:31-40), the block id. 64 lanes a workgroup, one ray a lane, each through vxd::intersect on the
// world's own bytes exactly as picker_kernel casts it (kernels_aux.hip). The world is read-only for the whole launch.
#include <hip/hip_runtime.h>

#include "kernels_raycast.h"
#include "vx_device.hpp"

using namespace vxd;

namespace {

// TRANSLUCENT is part of the kernel's type: the opaque cast then compiles to picker_kernel's walk (no texture sampling in the leaf test,
// about half the vector registers), and that is the cast nearly every batch asks for.
template <int SVO, bool TRANSLUCENT>
__global__ __launch_bounds__(64) void raycast_batch_kernel(SceneArgs sa, const uint8_t* __restrict__ origin, const uint8_t* __restrict__ dir,
                                                           const uint8_t* __restrict__ max_dst, uint32_t origin_stride, uint32_t dir_stride,
                                                           uint32_t max_dst_stride, float max_dst_all, uint32_t has_max_dst, uint32_t n,
                                                           vx_ray_hit* __restrict__ hits) {
    const DevScene sc = make_scene(sa);
    StackSpill spill;
    Stack<64> st;
    st.init(threadIdx.x, &spill);
    const uint32_t i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    float ro[3], rd[3], limit;
    vxk::gather_ray(origin, dir, max_dst, origin_stride, dir_stride, max_dst_stride, max_dst_all, has_max_dst, i, ro, rd, limit);
    // picker.glsl:30-51, cast_translucent as the batch asks
    Result res;
    uint32_t steps = 0;
    intersect<SVO, false, false, true>(sc, ro, rd, limit, TRANSLUCENT, st, res, steps, nullptr, nullptr);
    const bool hit = res.t > 0.0f;
    // the 32-byte record as two 16-byte stores: {dst, value, face_id, inside_voxel} {pos, 0}; a miss is -1 and zeros
    uint4 a, b;
    a.x = __float_as_uint(hit ? res.t : -1.0f);
    a.y = hit ? res.value : 0u;
    a.z = hit ? uint32_t(res.face_id) : 0u;
    a.w = hit && res.inside_voxel ? 1u : 0u;
    b.x = hit ? __float_as_uint(res.pos[0]) : 0u;
    b.y = hit ? __float_as_uint(res.pos[1]) : 0u;
    b.z = hit ? __float_as_uint(res.pos[2]) : 0u;
    b.w = 0u;
    uint4* out = reinterpret_cast<uint4*>(hits + i);
    out[0] = a;
    out[1] = b;
}

}  // namespace

namespace vxk {

hipError_t launch_raycast_batch(int svo, hipStream_t stream, const SceneArgs& sc, const RayBatchArgs& r, uint32_t count, vx_ray_hit* hits) {
    static_assert(sizeof(vx_ray_hit) == 32, "two 16-byte stores");
    const size_t lds = Stack<64>::kBytes;
    const dim3 grid((count + 63u) / 64u), block(64);
    const uint8_t *o = static_cast<const uint8_t*>(r.origin), *d = static_cast<const uint8_t*>(r.dir), *m = static_cast<const uint8_t*>(r.max_dst);
#define VX_LAUNCH_RAYS_T(S, T)                                                                                                           \
    hipLaunchKernelGGL((raycast_batch_kernel<S, T>), grid, block, lds, stream, sc, o, d, m, r.origin_stride, r.dir_stride, r.max_dst_stride, \
                       r.max_dst_all, r.has_max_dst, count, hits)
#define VX_LAUNCH_RAYS(S)                        \
    do {                                         \
        if (r.translucent) VX_LAUNCH_RAYS_T(S, true); \
        else VX_LAUNCH_RAYS_T(S, false);         \
    } while (0)
    if (svo == VX_SVO_ESVO_BIG) VX_LAUNCH_RAYS(VX_SVO_ESVO_BIG);
    else if (svo == VX_SVO_ESVO) VX_LAUNCH_RAYS(VX_SVO_ESVO);
    else if (svo == VX_SVO_CSVO) VX_LAUNCH_RAYS(VX_SVO_CSVO);
    else return hipErrorInvalidValue;
#undef VX_LAUNCH_RAYS
#undef VX_LAUNCH_RAYS_T
    return hipGetLastError();
}

}  // namespace vxk

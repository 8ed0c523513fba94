// vx_physics_step's kernel (gfx950): K fixed steps of systems::Physics::step_many (src/systems/physics.rs:122-136) for N entities in one
// launch. ONE WAVE PER ENTITY, one wave per workgroup: the lanes share out the entity's fan of axis-parallel picker rays
// (svo_picker.rs:183-243; the player's 0.8 x 1.8 x 0.8 box: 36 slots, 32 rays, one trip), each through vxd::intersect on the world's own
// bytes exactly as picker_kernel casts it (kernels_aux.hip), fold their hit distances into six minima, the wave reduces those across its
// lanes, and every lane then makes the identical update of the entity (vx_physics.hpp) -- which lives in registers over all the steps. The
// world is read-only for the whole launch; nothing but the entity records and the contact distances is read or written besides.
#include <hip/hip_runtime.h>

#include "kernels_physics.h"
#include "vx_physics.hpp"

using namespace vxd;
using namespace vxp;

namespace {

// the minimum over the wave's 64 lanes, in every lane (xor butterfly: 32, 16, .. 1); the operands are never NaN
__device__ __forceinline__ float wave_min(float v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v = gmin(v, __shfl_xor(v, d, 64));
    return v;
}

template <int SVO>
__global__ __launch_bounds__(64) void physics_kernel(SceneArgs sa, vx_entity* __restrict__ entities, uint32_t count, float delta_time, uint32_t steps,
                                                     vx_aabb_result* __restrict__ contacts) {
    const DevScene sc = make_scene(sa);
    StackSpill spill;
    Stack<64> st;
    st.init(threadIdx.x, &spill);
    const uint32_t i = blockIdx.x, lane = threadIdx.x;
    if (i >= count) return;
    vx_entity e = entities[i];  // (the same 64 bytes in every lane: one request)
    if (!steppable(e)) {        // wave-uniform: the record stays as it is
        if (lane == 0) write_back_unsteppable(contacts, i);
        return;
    }
    const Fan fan = make_fan(e);
    vx_aabb_result result = no_result();
    for (uint32_t k = 0, rounds = rounds_of(steps); k < rounds; ++k) {
        Contacts c = lane_contacts<SVO>(sc, fan, e, lane, st);  // trips of 64 slots
#pragma unroll
        for (int m = 0; m < 6; ++m) c.m[m] = wave_min(c.m[m]);
        result = finish_round(e, c, delta_time, steps);  // every lane: the identical update
    }
    if (lane == 0) write_back(entities, contacts, i, e, result, steps);
}

}  // namespace

namespace vxk {

hipError_t launch_physics(int svo, hipStream_t stream, const SceneArgs& sc, vx_entity* entities, uint32_t count, float delta_time, uint32_t steps,
                          vx_aabb_result* contacts) {
    const size_t lds = Stack<64>::kBytes;
    const dim3 grid(count), block(64);
    if (svo == VX_SVO_ESVO_BIG) hipLaunchKernelGGL((physics_kernel<VX_SVO_ESVO_BIG>), grid, block, lds, stream, sc, entities, count, delta_time, steps, contacts);
    else if (svo == VX_SVO_ESVO) hipLaunchKernelGGL((physics_kernel<VX_SVO_ESVO>), grid, block, lds, stream, sc, entities, count, delta_time, steps, contacts);
    else if (svo == VX_SVO_CSVO) hipLaunchKernelGGL((physics_kernel<VX_SVO_CSVO>), grid, block, lds, stream, sc, entities, count, delta_time, steps, contacts);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

}  // namespace vxk

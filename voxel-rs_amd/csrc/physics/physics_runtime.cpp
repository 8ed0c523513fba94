// libvoxelhip.so, entity physics: vx_physics_step (include/voxel_hip.h) -- argument checks, the validation of host records, the pinned
// scratch host records travel through (csrc/vx_pinned_pool.hpp), and the launch of kernels_physics.hip. A second translation unit on the
// context, like comm.cpp: what it needs of the context is vx_context.hpp's (runtime.cpp).
#include <cstring>
#include <mutex>

#include "kernels_physics.h"
#include "vx_context.hpp"
#include "vx_physics_rules.h"
#include "vx_pinned_pool.hpp"

using vxrt::fail;

int vx_physics_step(vx_context* ctx, vx_entity* entities, uint32_t count, int memory, float delta_time, uint32_t steps, vx_aabb_result* contacts) {
    static_assert(sizeof(vx_entity) == 64 && sizeof(vx_aabb_result) == 24, "the ABI's record sizes");
    if (memory != VX_MEM_HOST && memory != VX_MEM_DEVICE) return fail(VX_ERR_INVALID_ARGUMENT, "physics_step: memory is neither VX_MEM_HOST nor VX_MEM_DEVICE");
    if (steps > vxp::kMaxSteps) return fail(VX_ERR_INVALID_ARGUMENT, "physics_step: more than 1024 steps in one call");
    if (count > vxp::kMaxEntities) return fail(VX_ERR_INVALID_ARGUMENT, "physics_step: more than 16777216 entities in one call");
    if (!ctx) return fail(VX_ERR_INVALID_ARGUMENT, "null context");
    if (count && !entities) return fail(VX_ERR_INVALID_ARGUMENT, "physics_step: null entities");
    if (int rc = vxrt::check_ready(ctx)) return rc;
    VX_LOCK(ctx);
    if (count == 0) return VX_OK;
    const int svo = ctx->big ? VX_SVO_ESVO_BIG : ctx->svo_type;  // the kernel variant, as vx_raycast picks it

    if (memory == VX_MEM_DEVICE) {
        HIP_TRY(vxk::launch_physics(svo, ctx->stream, vxrt::scene_on_bytes(ctx), entities, count, delta_time, steps, contacts));
        return vxrt::mark_world_read(ctx);
    }

    for (uint32_t i = 0; i < count; ++i)
        if (!vxp::steppable_extents(entities[i].aabb_extents))
            return fail(VX_ERR_INVALID_ARGUMENT, "physics_step: entity " + std::to_string(i) + " cannot be stepped: every extent must be finite, > 0 and <= 8");
    const size_t entity_bytes = size_t(count) * sizeof(vx_entity), contact_bytes = contacts ? size_t(count) * sizeof(vx_aabb_result) : 0;
    vxrt::PinnedPool& pool = vxrt::pinned_pool_of(ctx->device);
    std::lock_guard<std::mutex> pool_lock(pool.mutex);
    if (int rc = vxrt::pinned_pool_reserve(pool, entity_bytes + contact_bytes)) return rc;
    std::memcpy(pool.host, entities, entity_bytes);
    HIP_TRY(vxk::launch_physics(svo, ctx->stream, vxrt::scene_on_bytes(ctx), reinterpret_cast<vx_entity*>(pool.dev), count, delta_time, steps,
                                contacts ? reinterpret_cast<vx_aabb_result*>(pool.dev + entity_bytes) : nullptr));
    HIP_TRY(hipStreamSynchronize(ctx->stream));  // synchronous, like vx_raycast (svo.rs:248-249)
    if (steps) std::memcpy(entities, pool.host, entity_bytes);
    if (contacts) std::memcpy(contacts, pool.host + entity_bytes, contact_bytes);
    return VX_OK;
}

// libvoxelhip.so, entity physics: vx_physics_step (include/voxel_hip.h) -- argument checks, the validation of host records, the pinned
// scratch host records travel through (csrc/vx_pinned_pool.hpp), and the launch of kernels_physics.hip. A second translation unit on the
// context, like comm.cpp.
#include <cstring>
#include <mutex>

#include "kernels_physics.h"
#include "vx_context.hpp"
#include "vx_physics_rules.h"
#include "vx_pinned_pool.hpp"

using vxrt::fail;

namespace {

// What the kernel sees of the context: runtime.cpp's scene_of (runtime.cpp:47-62) for a walk on the world's OWN bytes -- the picker
// path never reads the traversal image.
vxd::SceneArgs scene_of(const vx_context* c) {
    vxd::SceneArgs s = {};
    s.world = c->d_world;
    s.world_bytes = uint64_t(c->capacity) + 16;  // (kWorldPad: the zero bytes a context keeps behind the world buffer)
    s.materials = c->d_materials;
    s.n_materials = c->n_materials;
    s.tex = c->d_tex;
    s.tex_bytes = c->tex_bytes;
    s.width = c->tex.width; s.height = c->tex.height; s.layers = c->tex.layers; s.levels = c->tex.levels;
    for (int l = 0; l < 16; ++l) s.level_offset[l] = c->tex.level_offset[l];
    s.image = nullptr;
    s.image_bytes = 0;
    s.origin = nullptr;
    return s;
}

// runtime.cpp:179-184 (the context is not null here)
int check_ready(vx_context* ctx) {
    HIP_TRY(hipSetDevice(ctx->device));
    if (!ctx->committed) return fail(VX_ERR_STATE, "no SVO committed yet (call vx_commit / vx_commit_all first)");
    return VX_OK;
}

}  // namespace

int vx_physics_step(vx_context* ctx, vx_entity* entities, uint32_t count, int memory, float delta_time, uint32_t steps, vx_aabb_result* contacts) {
    static_assert(sizeof(vx_entity) == 64 && sizeof(vx_aabb_result) == 24, "the ABI's record sizes");
    if (memory != VX_MEM_HOST && memory != VX_MEM_DEVICE) return fail(VX_ERR_INVALID_ARGUMENT, "physics_step: memory is neither VX_MEM_HOST nor VX_MEM_DEVICE");
    if (steps > vxp::kMaxSteps) return fail(VX_ERR_INVALID_ARGUMENT, "physics_step: more than 1024 steps in one call");
    if (count > vxp::kMaxEntities) return fail(VX_ERR_INVALID_ARGUMENT, "physics_step: more than 16777216 entities in one call");
    if (!ctx) return fail(VX_ERR_INVALID_ARGUMENT, "null context");
    if (count && !entities) return fail(VX_ERR_INVALID_ARGUMENT, "physics_step: null entities");
    if (int rc = check_ready(ctx)) return rc;
    VX_LOCK(ctx);
    if (count == 0) return VX_OK;
    const int svo = ctx->big ? VX_SVO_ESVO_BIG : ctx->svo_type;  // the kernel variant, as vx_raycast picks it

    if (memory == VX_MEM_DEVICE) {
        HIP_TRY(vxk::launch_physics(svo, ctx->stream, scene_of(ctx), entities, count, delta_time, steps, contacts));
        // the kernel reads the world: a later commit's uploads wait for it like for a frame in flight (vx_commit: render_fence.wait())
        HIP_TRY(hipEventRecord(ctx->render_done, ctx->stream));
        ctx->render_recorded = true;
        return VX_OK;
    }

    for (uint32_t i = 0; i < count; ++i)
        if (!vxp::steppable_extents(entities[i].aabb_extents))
            return fail(VX_ERR_INVALID_ARGUMENT, "physics_step: entity " + std::to_string(i) + " cannot be stepped: every extent must be finite, > 0 and <= 8");
    const size_t entity_bytes = size_t(count) * sizeof(vx_entity), contact_bytes = contacts ? size_t(count) * sizeof(vx_aabb_result) : 0;
    vxrt::PinnedPool& pool = vxrt::pinned_pool_of(ctx->device);
    std::lock_guard<std::mutex> pool_lock(pool.mutex);
    if (int rc = vxrt::pinned_pool_reserve(pool, entity_bytes + contact_bytes)) return rc;
    std::memcpy(pool.host, entities, entity_bytes);
    HIP_TRY(vxk::launch_physics(svo, ctx->stream, scene_of(ctx), reinterpret_cast<vx_entity*>(pool.dev), count, delta_time, steps,
                                contacts ? reinterpret_cast<vx_aabb_result*>(pool.dev + entity_bytes) : nullptr));
    HIP_TRY(hipStreamSynchronize(ctx->stream));  // synchronous, like vx_raycast (svo.rs:248-249)
    if (steps) std::memcpy(entities, pool.host, entity_bytes);
    if (contacts) std::memcpy(contacts, pool.host + entity_bytes, contact_bytes);
    return VX_OK;
}

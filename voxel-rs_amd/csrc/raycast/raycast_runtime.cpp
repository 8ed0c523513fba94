// libvoxelhip.so, ray batches: vx_raycast_batch (include/voxel_hip.h) -- argument checks, the packing of strided host arrays (vx_ray_batch.hpp) into
// the pinned scratch the kernel reads and writes (csrc/vx_pinned_pool.hpp), and the launch of kernels_raycast.hip. A further translation unit on
// the context, like physics_runtime.cpp: what it needs of the context is vx_context.hpp's (runtime.cpp).
#include <cstring>
#include <mutex>

#include "kernels_raycast.h"
#include "vx_context.hpp"
#include "vx_pinned_pool.hpp"

using vxrt::fail;

int vx_raycast_batch(vx_context* ctx, const vx_ray_batch* rays, uint32_t count, int memory, vx_ray_hit* hits) {
    static_assert(sizeof(vx_ray_hit) == 32 && sizeof(vx_ray_batch) == 48, "the ABI's record sizes");
    if (memory != VX_MEM_HOST && memory != VX_MEM_DEVICE) return fail(VX_ERR_INVALID_ARGUMENT, "raycast_batch: memory is neither VX_MEM_HOST nor VX_MEM_DEVICE");
    if (rays)
        if (int rc = vxrt::check_ray_batch(*rays, "raycast_batch")) return rc;
    if (!ctx) return fail(VX_ERR_INVALID_ARGUMENT, "null context");
    if (count && !rays) return fail(VX_ERR_INVALID_ARGUMENT, "raycast_batch: null rays");
    if (count && !hits) return fail(VX_ERR_INVALID_ARGUMENT, "raycast_batch: null hits");
    if (int rc = vxrt::check_ready(ctx)) return rc;
    VX_LOCK(ctx);
    if (count == 0) return VX_OK;
    const int svo = ctx->big ? VX_SVO_ESVO_BIG : ctx->svo_type;  // the kernel variant, as vx_raycast picks it

    if (memory == VX_MEM_DEVICE) {
        HIP_TRY(vxk::launch_raycast_batch(svo, ctx->stream, vxrt::scene_on_bytes(ctx), vxrt::rays_in_place(*rays), count, hits));
        return vxrt::mark_world_read(ctx);
    }

    // Host arrays, packed as vx_ray_batch.hpp lays them out | the hits (at a multiple of 16)
    const vxrt::RayPlan plan = vxrt::plan_rays(*rays, count);
    const size_t at_hits = plan.end, hit_bytes = size_t(count) * sizeof(vx_ray_hit);
    vxrt::PinnedPool& pool = vxrt::pinned_pool_of(ctx->device);
    std::lock_guard<std::mutex> pool_lock(pool.mutex);
    if (int rc = vxrt::pinned_pool_reserve(pool, at_hits + hit_bytes)) return rc;
    const vxk::RayBatchArgs a = vxrt::pack_rays(*rays, count, plan, pool.host, pool.dev);
    HIP_TRY(vxk::launch_raycast_batch(svo, ctx->stream, vxrt::scene_on_bytes(ctx), a, count, reinterpret_cast<vx_ray_hit*>(pool.dev + at_hits)));
    HIP_TRY(hipStreamSynchronize(ctx->stream));  // synchronous, like vx_raycast (svo.rs:248-249)
    std::memcpy(hits, pool.host + at_hits, hit_bytes);
    return VX_OK;
}

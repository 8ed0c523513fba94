// libvoxelhip.so, shaded ray batches: vx_trace_rays (include/voxel_hip.h) -- argument checks, the packing of strided host arrays (vx_ray_batch.hpp)
// into the pinned scratch the kernel reads and writes (csrc/vx_pinned_pool.hpp), and the launch of kernels_trace.hip. A further translation unit
// on the context, like raycast_runtime.cpp, whose batch rules, memory kinds, ordering and fences it shares.
#include <cstring>
#include <mutex>

#include "kernels_trace.h"
#include "vx_context.hpp"
#include "vx_pinned_pool.hpp"

using vxrt::fail;

namespace {

constexpr uint32_t kMaxRays = 1u << 24;

}  // namespace

int vx_trace_rays(vx_context* ctx, const vx_uniforms* uniforms, const vx_ray_batch* rays, uint32_t count, int memory, void* rgba, int format,
                  vx_hit* hits) {
    static_assert(sizeof(vx_hit) == 48 && sizeof(vx_ray_batch) == 48, "the ABI's record sizes");
    // what needs no device comes first: the call itself, then the batch, then what is missing
    if (memory != VX_MEM_HOST && memory != VX_MEM_DEVICE) return fail(VX_ERR_INVALID_ARGUMENT, "trace_rays: memory is neither VX_MEM_HOST nor VX_MEM_DEVICE");
    if (format != VX_FORMAT_RGBA32F && format != VX_FORMAT_RGBA8) return fail(VX_ERR_INVALID_ARGUMENT, "trace_rays: format is neither VX_FORMAT_RGBA32F nor VX_FORMAT_RGBA8");
    if (count > kMaxRays) return fail(VX_ERR_INVALID_ARGUMENT, "trace_rays: count exceeds 16777216 (2^24) rays");
    if (rays)
        if (int rc = vxrt::check_ray_batch(*rays, "trace_rays")) return rc;
    if (!ctx) return fail(VX_ERR_INVALID_ARGUMENT, "null context");
    if (count && !uniforms) return fail(VX_ERR_INVALID_ARGUMENT, "trace_rays: null uniforms");
    if (count && !rays) return fail(VX_ERR_INVALID_ARGUMENT, "trace_rays: null rays");
    if (count && !rgba && !hits) return fail(VX_ERR_INVALID_ARGUMENT, "trace_rays: null rgba and null hits (one of the two outputs is needed)");
    const size_t pixel = format == VX_FORMAT_RGBA8 ? 4 : 16;
    if (count && memory == VX_MEM_DEVICE) {  // the kernel stores whole pixels and 16-byte thirds of a record
        if (reinterpret_cast<uintptr_t>(rgba) % pixel) return fail(VX_ERR_INVALID_ARGUMENT, "trace_rays: rgba in device memory must be aligned to a pixel");
        if (reinterpret_cast<uintptr_t>(hits) % 16) return fail(VX_ERR_INVALID_ARGUMENT, "trace_rays: hits in device memory must be aligned to 16 bytes");
    }
    if (int rc = vxrt::check_ready(ctx)) return rc;
    VX_LOCK(ctx);
    if (count == 0) return VX_OK;
    const int svo = ctx->big ? VX_SVO_ESVO_BIG : ctx->svo_type;  // the kernel variant, as vx_raycast picks it

    if (memory == VX_MEM_DEVICE) {
        HIP_TRY(vxk::launch_trace_rays(svo, ctx->stream, vxrt::scene_on_bytes(ctx), *uniforms, vxrt::rays_in_place(*rays), count, rgba, format, hits));
        return vxrt::mark_world_read(ctx);
    }

    // Host arrays, packed as vx_ray_batch.hpp lays them out | the pixels | the records (both at a multiple of 16)
    const vxrt::RayPlan plan = vxrt::plan_rays(*rays, count);
    const size_t rgba_bytes = rgba ? count * pixel : 0, hit_bytes = hits ? size_t(count) * sizeof(vx_hit) : 0;
    const size_t at_rgba = plan.end, at_hits = vxrt::round16(at_rgba + rgba_bytes);
    vxrt::PinnedPool& pool = vxrt::pinned_pool_of(ctx->device);
    std::lock_guard<std::mutex> pool_lock(pool.mutex);
    if (int rc = vxrt::pinned_pool_reserve(pool, at_hits + hit_bytes)) return rc;
    const vxk::RayBatchArgs a = vxrt::pack_rays(*rays, count, plan, pool.host, pool.dev);
    HIP_TRY(vxk::launch_trace_rays(svo, ctx->stream, vxrt::scene_on_bytes(ctx), *uniforms, a, count, rgba ? pool.dev + at_rgba : nullptr, format,
                                   hits ? reinterpret_cast<vx_hit*>(pool.dev + at_hits) : nullptr));
    HIP_TRY(hipStreamSynchronize(ctx->stream));  // synchronous, like vx_raycast_batch
    if (rgba) std::memcpy(rgba, pool.host + at_rgba, rgba_bytes);
    if (hits) std::memcpy(hits, pool.host + at_hits, hit_bytes);
    return VX_OK;
}

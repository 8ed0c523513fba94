// libvoxelhip.so, shaded ray batches: vx_trace_rays (include/voxel_hip.h) -- argument checks, the packing of strided host arrays into the pinned
// scratch the kernel reads and writes (csrc/vx_pinned_pool.hpp), and the launch of kernels_trace.hip. A further translation unit on the
// context, like raycast_runtime.cpp, whose memory kinds, ordering and fences it shares.
#include <cstring>
#include <mutex>

#include "kernels_trace.h"
#include "vx_context.hpp"
#include "vx_pinned_pool.hpp"

using vxrt::fail;

namespace {

constexpr uint32_t kMaxRays = 1u << 24;

// raycast_runtime.cpp's scene_of: a walk on the world's OWN bytes, the traversal image is never read
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

int check_ready(vx_context* ctx) {
    HIP_TRY(hipSetDevice(ctx->device));
    if (!ctx->committed) return fail(VX_ERR_STATE, "no SVO committed yet (call vx_commit / vx_commit_all first)");
    return VX_OK;
}

// vx_ray_batch's rules (voxel_hip.h), as vx_raycast_batch applies them; needs no device
int check_batch(const vx_ray_batch& r) {
    if (r.flags & ~uint32_t(VX_RAYS_TRANSLUCENT)) return fail(VX_ERR_INVALID_ARGUMENT, "trace_rays: flags has a bit other than VX_RAYS_TRANSLUCENT");
    if (!r.origin) return fail(VX_ERR_INVALID_ARGUMENT, "trace_rays: null origin");
    if (!r.dir) return fail(VX_ERR_INVALID_ARGUMENT, "trace_rays: null dir");
    if (r.origin_stride % 4 || r.origin_stride < 12) return fail(VX_ERR_INVALID_ARGUMENT, "trace_rays: origin_stride must be a multiple of 4 and >= 12");
    if (r.dir_stride % 4 || (r.dir_stride && r.dir_stride < 12))
        return fail(VX_ERR_INVALID_ARGUMENT, "trace_rays: dir_stride must be 0 or a multiple of 4 and >= 12");
    if (r.max_dst && r.max_dst_stride % 4) return fail(VX_ERR_INVALID_ARGUMENT, "trace_rays: max_dst_stride must be 0 or a multiple of 4");
    return VX_OK;
}

size_t round16(size_t v) { return (v + 15) & ~size_t(15); }

}  // namespace

int vx_trace_rays(vx_context* ctx, const vx_uniforms* uniforms, const vx_ray_batch* rays, uint32_t count, int memory, void* rgba, int format,
                  vx_hit* hits) {
    static_assert(sizeof(vx_hit) == 48 && sizeof(vx_ray_batch) == 48, "the ABI's record sizes");
    // what needs no device comes first: the call itself, then the batch, then what is missing
    if (memory != VX_MEM_HOST && memory != VX_MEM_DEVICE) return fail(VX_ERR_INVALID_ARGUMENT, "trace_rays: memory is neither VX_MEM_HOST nor VX_MEM_DEVICE");
    if (format != VX_FORMAT_RGBA32F && format != VX_FORMAT_RGBA8) return fail(VX_ERR_INVALID_ARGUMENT, "trace_rays: format is neither VX_FORMAT_RGBA32F nor VX_FORMAT_RGBA8");
    if (count > kMaxRays) return fail(VX_ERR_INVALID_ARGUMENT, "trace_rays: count exceeds 16777216 (2^24) rays");
    if (rays)
        if (int rc = check_batch(*rays)) return rc;
    if (!ctx) return fail(VX_ERR_INVALID_ARGUMENT, "null context");
    if (count && !uniforms) return fail(VX_ERR_INVALID_ARGUMENT, "trace_rays: null uniforms");
    if (count && !rays) return fail(VX_ERR_INVALID_ARGUMENT, "trace_rays: null rays");
    if (count && !rgba && !hits) return fail(VX_ERR_INVALID_ARGUMENT, "trace_rays: null rgba and null hits (one of the two outputs is needed)");
    const size_t pixel = format == VX_FORMAT_RGBA8 ? 4 : 16;
    if (count && memory == VX_MEM_DEVICE) {  // the kernel stores whole pixels and 16-byte thirds of a record
        if (reinterpret_cast<uintptr_t>(rgba) % pixel) return fail(VX_ERR_INVALID_ARGUMENT, "trace_rays: rgba in device memory must be aligned to a pixel");
        if (reinterpret_cast<uintptr_t>(hits) % 16) return fail(VX_ERR_INVALID_ARGUMENT, "trace_rays: hits in device memory must be aligned to 16 bytes");
    }
    if (int rc = check_ready(ctx)) return rc;
    VX_LOCK(ctx);
    if (count == 0) return VX_OK;
    const int svo = ctx->big ? VX_SVO_ESVO_BIG : ctx->svo_type;  // the kernel variant, as vx_raycast picks it

    vxk::RayBatchArgs a = {};
    a.max_dst_all = rays->max_dst_all;
    a.has_max_dst = rays->max_dst ? 1u : 0u;
    a.translucent = 1u;  // (not read: trace_ray casts translucent whatever the flag says, world.glsl:29)

    if (memory == VX_MEM_DEVICE) {
        a.origin = rays->origin; a.dir = rays->dir; a.max_dst = rays->max_dst;
        a.origin_stride = rays->origin_stride; a.dir_stride = rays->dir_stride; a.max_dst_stride = rays->max_dst_stride;
        HIP_TRY(vxk::launch_trace_rays(svo, ctx->stream, scene_of(ctx), *uniforms, a, count, rgba, format, hits));
        // the kernel reads the world: a later commit's uploads wait for it like for a frame in flight (vx_commit: render_fence.wait())
        HIP_TRY(hipEventRecord(ctx->render_done, ctx->stream));
        ctx->render_recorded = true;
        return VX_OK;
    }

    // Host arrays, packed: origins at stride 12 | directions at stride 12, or the one | distances at stride 4, the one, or none | the pixels | the
    // records (both at a multiple of 16)
    const size_t n = count;
    const size_t n_dir = rays->dir_stride ? n : 1, n_dst = !rays->max_dst ? 0 : (rays->max_dst_stride ? n : 1);
    const size_t rgba_bytes = rgba ? n * pixel : 0, hit_bytes = hits ? n * sizeof(vx_hit) : 0;
    const size_t at_dir = 12 * n, at_dst = at_dir + 12 * n_dir, at_rgba = round16(at_dst + 4 * n_dst), at_hits = round16(at_rgba + rgba_bytes);
    vxrt::PinnedPool& pool = vxrt::pinned_pool_of(ctx->device);
    std::lock_guard<std::mutex> pool_lock(pool.mutex);
    if (int rc = vxrt::pinned_pool_reserve(pool, at_hits + hit_bytes)) return rc;
    const uint8_t *o = static_cast<const uint8_t*>(rays->origin), *d = static_cast<const uint8_t*>(rays->dir), *m = static_cast<const uint8_t*>(rays->max_dst);
    const auto pack = [](uint8_t* to, const uint8_t* from, size_t stride, size_t width, size_t items) {
        if (stride == width || items == 1) std::memcpy(to, from, width * items);
        else for (size_t i = 0; i < items; ++i) std::memcpy(to + width * i, from + stride * i, width);
    };
    pack(pool.host, o, rays->origin_stride, 12, n);
    pack(pool.host + at_dir, d, rays->dir_stride, 12, n_dir);
    if (n_dst) pack(pool.host + at_dst, m, rays->max_dst_stride, 4, n_dst);
    a.origin = pool.dev; a.dir = pool.dev + at_dir; a.max_dst = pool.dev + at_dst;
    a.origin_stride = 12; a.dir_stride = n_dir == 1 ? 0 : 12; a.max_dst_stride = n_dst == n ? 4 : 0;
    HIP_TRY(vxk::launch_trace_rays(svo, ctx->stream, scene_of(ctx), *uniforms, a, count, rgba ? pool.dev + at_rgba : nullptr, format,
                                   hits ? reinterpret_cast<vx_hit*>(pool.dev + at_hits) : nullptr));
    HIP_TRY(hipStreamSynchronize(ctx->stream));  // synchronous, like vx_raycast_batch
    if (rgba) std::memcpy(rgba, pool.host + at_rgba, rgba_bytes);
    if (hits) std::memcpy(hits, pool.host + at_hits, hit_bytes);
    return VX_OK;
}

// libvoxelhip.so, block ids read from the device: vx_block_points and vx_read_region, and the first block along an axis: vx_scan_points and
// vx_scan_columns (include/voxel_hip.h) -- argument checks (vx_blocks.hpp's and vx_scan.hpp's rules), the pinned scratch the host-memory calls
// read and write through (csrc/vx_pinned_pool.hpp), and the launches of kernels_blocks.hip and kernels_scan.hip.
// A further translation unit on the context, like raycast_runtime.cpp: what it needs of the context is vx_context.hpp's (runtime.cpp).
#include <cstring>
#include <mutex>

#include "kernels_blocks.h"
#include "vx_context.hpp"
#include "vx_pinned_pool.hpp"

using vxrt::fail;

namespace {

inline size_t round16(size_t v) { return (v + 15) & ~size_t(15); }
inline int kernel_variant(const vx_context* ctx) { return ctx->big ? VX_SVO_ESVO_BIG : ctx->svo_type; }  // as vx_raycast picks it

}  // namespace

int vx_block_points(vx_context* ctx, const void* pos, uint32_t pos_stride, uint32_t count, int memory, vx_block_cell* out) {
    static_assert(sizeof(vx_block_cell) == 8, "the ABI's record size");
    if (memory != VX_MEM_HOST && memory != VX_MEM_DEVICE) return fail(VX_ERR_INVALID_ARGUMENT, "block_points: memory is neither VX_MEM_HOST nor VX_MEM_DEVICE");
    if (const char* what = vxb::check_points(pos, pos_stride, count, out)) return fail(VX_ERR_INVALID_ARGUMENT, std::string("block_points: ") + what);
    if (count && memory == VX_MEM_DEVICE && reinterpret_cast<uintptr_t>(out) % 8) return fail(VX_ERR_INVALID_ARGUMENT, "block_points: out in device memory must be aligned to 8 bytes");
    if (!ctx) return fail(VX_ERR_INVALID_ARGUMENT, "null context");
    if (int rc = vxrt::check_ready(ctx)) return rc;
    VX_LOCK(ctx);
    if (count == 0) return VX_OK;

    if (memory == VX_MEM_DEVICE) {
        HIP_TRY(vxk::launch_block_points(kernel_variant(ctx), ctx->stream, vxrt::scene_on_bytes(ctx), pos, pos_stride, count, out));
        return vxrt::mark_world_read(ctx);
    }

    // the positions packed at stride 12 | the records (at a multiple of 16)
    const size_t at_out = round16(size_t(count) * 12), out_bytes = size_t(count) * sizeof(vx_block_cell);
    vxrt::PinnedPool& pool = vxrt::pinned_pool_of(ctx->device);
    std::lock_guard<std::mutex> pool_lock(pool.mutex);
    if (int rc = vxrt::pinned_pool_reserve(pool, at_out + out_bytes)) return rc;
    const uint8_t* from = static_cast<const uint8_t*>(pos);
    if (pos_stride == 12) std::memcpy(pool.host, from, size_t(count) * 12);
    else for (size_t i = 0; i < count; ++i) std::memcpy(pool.host + 12 * i, from + size_t(pos_stride) * i, 12);  // (exactly a position's bytes: an array may end with its last one)
    HIP_TRY(vxk::launch_block_points(kernel_variant(ctx), ctx->stream, vxrt::scene_on_bytes(ctx), pool.dev, 12, count,
                                     reinterpret_cast<vx_block_cell*>(pool.dev + at_out)));
    HIP_TRY(hipStreamSynchronize(ctx->stream));  // synchronous, like vx_raycast_batch's host-memory call
    std::memcpy(out, pool.host + at_out, out_bytes);
    return VX_OK;
}

int vx_read_region(vx_context* ctx, const int32_t lo[3], const uint32_t size[3], int memory, uint32_t* out) {
    if (memory != VX_MEM_HOST && memory != VX_MEM_DEVICE) return fail(VX_ERR_INVALID_ARGUMENT, "read_region: memory is neither VX_MEM_HOST nor VX_MEM_DEVICE");
    if (const char* what = vxb::check_region(lo, size)) return fail(VX_ERR_INVALID_ARGUMENT, std::string("read_region: ") + what);
    const size_t voxels = size_t(size[0]) * size[1] * size[2];  // (at most 2^24, or 0)
    if (voxels && !out) return fail(VX_ERR_INVALID_ARGUMENT, "read_region: null out");
    if (memory == VX_MEM_DEVICE && reinterpret_cast<uintptr_t>(out) % 4) return fail(VX_ERR_INVALID_ARGUMENT, "read_region: out in device memory must be aligned to 4 bytes");
    if (!ctx) return fail(VX_ERR_INVALID_ARGUMENT, "null context");
    if (int rc = vxrt::check_ready(ctx)) return rc;
    VX_LOCK(ctx);
    if (voxels == 0) return VX_OK;
    const vxb::Region r = vxb::plan_region(lo, size);

    if (memory == VX_MEM_DEVICE) {
        HIP_TRY(vxk::launch_read_region(kernel_variant(ctx), ctx->stream, vxrt::scene_on_bytes(ctx), r, out));
        return vxrt::mark_world_read(ctx);
    }

    vxrt::PinnedPool& pool = vxrt::pinned_pool_of(ctx->device);
    std::lock_guard<std::mutex> pool_lock(pool.mutex);
    if (int rc = vxrt::pinned_pool_reserve(pool, voxels * 4)) return rc;
    HIP_TRY(vxk::launch_read_region(kernel_variant(ctx), ctx->stream, vxrt::scene_on_bytes(ctx), r, reinterpret_cast<uint32_t*>(pool.dev)));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    std::memcpy(out, pool.host, voxels * 4);
    return VX_OK;
}

int vx_scan_points(vx_context* ctx, const void* pos, uint32_t pos_stride, uint32_t count, int direction, uint32_t reach, int memory, vx_scan_hit* out) {
    static_assert(sizeof(vx_scan_hit) == 16, "the ABI's record size");
    if (memory != VX_MEM_HOST && memory != VX_MEM_DEVICE) return fail(VX_ERR_INVALID_ARGUMENT, "scan_points: memory is neither VX_MEM_HOST nor VX_MEM_DEVICE");
    if (const char* what = vxb::check_scan_points(pos, pos_stride, count, direction, reach, out)) return fail(VX_ERR_INVALID_ARGUMENT, std::string("scan_points: ") + what);
    if (count && memory == VX_MEM_DEVICE && reinterpret_cast<uintptr_t>(out) % 16) return fail(VX_ERR_INVALID_ARGUMENT, "scan_points: out in device memory must be aligned to 16 bytes");
    if (!ctx) return fail(VX_ERR_INVALID_ARGUMENT, "null context");
    if (int rc = vxrt::check_ready(ctx)) return rc;
    VX_LOCK(ctx);
    if (count == 0) return VX_OK;

    if (memory == VX_MEM_DEVICE) {
        HIP_TRY(vxk::launch_scan_points(kernel_variant(ctx), ctx->stream, vxrt::scene_on_bytes(ctx), pos, pos_stride, count, direction, reach, out));
        return vxrt::mark_world_read(ctx);
    }

    // the positions packed at stride 12 | the records (at a multiple of 16)
    const size_t at_out = round16(size_t(count) * 12), out_bytes = size_t(count) * sizeof(vx_scan_hit);
    vxrt::PinnedPool& pool = vxrt::pinned_pool_of(ctx->device);
    std::lock_guard<std::mutex> pool_lock(pool.mutex);
    if (int rc = vxrt::pinned_pool_reserve(pool, at_out + out_bytes)) return rc;
    const uint8_t* from = static_cast<const uint8_t*>(pos);
    if (pos_stride == 12) std::memcpy(pool.host, from, size_t(count) * 12);
    else for (size_t i = 0; i < count; ++i) std::memcpy(pool.host + 12 * i, from + size_t(pos_stride) * i, 12);
    HIP_TRY(vxk::launch_scan_points(kernel_variant(ctx), ctx->stream, vxrt::scene_on_bytes(ctx), pool.dev, 12, count, direction, reach,
                                    reinterpret_cast<vx_scan_hit*>(pool.dev + at_out)));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    std::memcpy(out, pool.host + at_out, out_bytes);
    return VX_OK;
}

int vx_scan_columns(vx_context* ctx, const int32_t lo[3], const uint32_t size[3], int direction, int memory, vx_scan_hit* out) {
    if (memory != VX_MEM_HOST && memory != VX_MEM_DEVICE) return fail(VX_ERR_INVALID_ARGUMENT, "scan_columns: memory is neither VX_MEM_HOST nor VX_MEM_DEVICE");
    if (const char* what = vxb::check_scan_columns(lo, size, direction)) return fail(VX_ERR_INVALID_ARGUMENT, std::string("scan_columns: ") + what);
    const vxb::Columns p = vxb::plan_columns(lo, size, direction);
    const bool any = size[0] && size[1] && size[2];
    const size_t columns = any ? size_t(p.size_u) * p.size_v : 0;  // (at most 2^24)
    if (columns && !out) return fail(VX_ERR_INVALID_ARGUMENT, "scan_columns: null out");
    if (memory == VX_MEM_DEVICE && reinterpret_cast<uintptr_t>(out) % 16) return fail(VX_ERR_INVALID_ARGUMENT, "scan_columns: out in device memory must be aligned to 16 bytes");
    if (!ctx) return fail(VX_ERR_INVALID_ARGUMENT, "null context");
    if (int rc = vxrt::check_ready(ctx)) return rc;
    VX_LOCK(ctx);
    if (columns == 0) return VX_OK;

    if (memory == VX_MEM_DEVICE) {
        HIP_TRY(vxk::launch_scan_columns(kernel_variant(ctx), ctx->stream, vxrt::scene_on_bytes(ctx), p, out));
        return vxrt::mark_world_read(ctx);
    }

    vxrt::PinnedPool& pool = vxrt::pinned_pool_of(ctx->device);
    std::lock_guard<std::mutex> pool_lock(pool.mutex);
    if (int rc = vxrt::pinned_pool_reserve(pool, columns * sizeof(vx_scan_hit))) return rc;
    HIP_TRY(vxk::launch_scan_columns(kernel_variant(ctx), ctx->stream, vxrt::scene_on_bytes(ctx), p, reinterpret_cast<vx_scan_hit*>(pool.dev)));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    std::memcpy(out, pool.host, columns * sizeof(vx_scan_hit));
    return VX_OK;
}

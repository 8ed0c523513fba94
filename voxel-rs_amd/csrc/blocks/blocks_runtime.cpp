// libvoxelhip.so, block ids read from the device: vx_block_points and vx_read_region, the first block along an axis: vx_scan_points and
// vx_scan_columns, the blocks of a box as a list: vx_list_region, what a batch of float boxes holds: vx_overlap_boxes, such boxes moved through the world: vx_move_boxes, step distances
// through air around a batch of positions: vx_flood_points, the light levels of a batch of boxes: vx_light_boxes, and walking distances and
// paths for ground agents: vx_walk_points (include/voxel_hip.h)
// -- argument checks (vx_blocks.hpp's, vx_scan.hpp's, vx_list.hpp's, vx_boxes.hpp's, vx_move.hpp's, vx_flood.hpp's, vx_light.hpp's and vx_walk.hpp's rules),
// the pinned scratch the host-memory calls read and write through (csrc/vx_pinned_pool.hpp), and the launches of kernels_blocks.hip,
// kernels_scan.hip, kernels_list.hip, kernels_boxes.hip, kernels_move.hip, kernels_flood.hip, kernels_light.hip and kernels_walk.hip.
// A further translation unit on the context, like raycast_runtime.cpp: what it needs of the context is vx_context.hpp's (runtime.cpp).
#include <cstring>
#include <map>
#include <mutex>
#include <utility>

#include "kernels_blocks.h"
#include "vx_context.hpp"
#include "vx_pinned_pool.hpp"

using vxrt::fail;

namespace {

inline size_t round16(size_t v) { return (v + 15) & ~size_t(15); }
inline int kernel_variant(const vx_context* ctx) { return ctx->big ? VX_SVO_ESVO_BIG : ctx->svo_type; }  // as vx_raycast picks it

// vx_list_region's workspace: a dword a brick of the box and one more, the records counted and then the offset of each brick's first record.
// It belongs to a context's stream -- every launch that uses it is queued there, so two calls never hold it at once -- but not to vx_context,
// which cannot grow (vx_pinned_pool.hpp): the table lives here, keyed by device and stream, under a mutex, and is kept for the life of the
// process like the pinned pool. vx_destroy drains and destroys the stream and leaves the entry: nothing can still be running on it, and a
// later context whose stream receives the same handle takes the buffer over. At most 4 bytes a brick of the largest box a stream has
// listed (fewer than 2^22 bricks in 2^24 voxels: 16 MiB, for the worst box of 1 x 1 x 2^24; 128 KiB for 256^3).
struct ListScratch {
    uint32_t* counts = nullptr;
    size_t entries = 0;
};

// At least `entries` dwords for the stream of `ctx`, under the context's lock. The buffer only grows; before the old one is freed the
// stream is waited for, so that no queued launch of an earlier call loses it (hipFree would wait as well: the wait is spelled out). A
// caller pays that wait only when a box has more bricks than any the stream has listed before.
int reserve_list_counts(vx_context* ctx, size_t entries, uint32_t** counts) {
    static std::mutex table_mutex;
    static std::map<std::pair<int, hipStream_t>, ListScratch> table;
    std::lock_guard<std::mutex> lock(table_mutex);
    ListScratch& s = table[{ctx->device, ctx->stream}];
    if (s.entries < entries) {
        if (s.counts) {
            HIP_TRY(hipStreamSynchronize(ctx->stream));
            (void)hipFree(s.counts);
            s.counts = nullptr;
            s.entries = 0;
        }
        size_t cap = 4096;
        while (cap < entries) cap *= 2;
        HIP_TRY(hipMalloc(reinterpret_cast<void**>(&s.counts), cap * sizeof(uint32_t)));
        s.entries = cap;
    }
    *counts = s.counts;
    return VX_OK;
}

// vx_light_boxes' table of props for a device-memory call, which returns before the launch has read it: a small ring of pinned buffers the
// kernel reads in place (no copy command), each guarded by an event, as views_runtime.cpp keeps its camera tables -- a call takes the next
// slot after waiting for the launch that read it four calls ago. One ring a device, kept for the life of the process; a slot's event is
// recorded on a stream of the ring's own, which is never destroyed and waits for the launch through an event that lives for the call alone
// (an event may not be waited for once the stream it was recorded on is gone with its context).
struct PropsSlot {
    uint8_t* host = nullptr;
    uint8_t* dev = nullptr;
    hipEvent_t done = nullptr;
    bool used = false;
};
struct PropsRing {
    static constexpr unsigned kSlots = 4;
    std::mutex mutex;
    PropsSlot slot[kSlots];
    unsigned next = 0;
    hipStream_t fence = nullptr;  // carries the slots' events; no work of its own
};

PropsRing& props_ring_of(int device) {
    static std::mutex rings_mutex;
    static std::map<int, PropsRing> rings;  // (node-based: a ring's address is stable)
    std::lock_guard<std::mutex> lock(rings_mutex);
    return rings[device];
}

// the ring's next slot, idle, under the ring's mutex
int props_slot_acquire(PropsRing& ring, PropsSlot** out) {
    PropsSlot& s = ring.slot[ring.next++ % PropsRing::kSlots];
    if (!s.done) HIP_TRY(hipEventCreateWithFlags(&s.done, hipEventDisableTiming));
    if (s.used) HIP_TRY(hipEventSynchronize(s.done));
    s.used = false;
    if (!s.host) {
        void *h = nullptr, *d = nullptr;
        HIP_TRY(hipHostMalloc(&h, VX_LIGHT_MAX_PROPS, hipHostMallocMapped));
        if (const hipError_t e = hipHostGetDevicePointer(&d, h, 0); e != hipSuccess) {
            (void)hipHostFree(h);
            HIP_TRY(e);
        }
        s.host = static_cast<uint8_t*>(h);
        s.dev = static_cast<uint8_t*>(d);
    }
    *out = &s;
    return VX_OK;
}

// slot.done follows everything queued on `stream` so far, without belonging to it
hipError_t props_slot_guard(PropsRing& ring, PropsSlot& slot, hipStream_t stream) {
    if (!ring.fence)
        if (const hipError_t e = hipStreamCreateWithFlags(&ring.fence, hipStreamNonBlocking); e != hipSuccess) return e;
    hipEvent_t queued = nullptr;
    if (const hipError_t e = hipEventCreateWithFlags(&queued, hipEventDisableTiming); e != hipSuccess) return e;
    hipError_t e = hipEventRecord(queued, stream);
    if (e == hipSuccess) e = hipStreamWaitEvent(ring.fence, queued, 0);
    if (e == hipSuccess) e = hipEventRecord(slot.done, ring.fence);
    (void)hipEventDestroy(queued);  // (released once it has happened)
    if (e != hipSuccess) {
        // no guard: the slot may not be handed out again before the launch is through with it
        (void)hipStreamSynchronize(stream);
        slot.used = false;
    }
    return e;
}

// the table as the kernel reads it: props_count bytes, zeros up to VX_LIGHT_MAX_PROPS
void fill_props(const vx_light_shape& s, uint8_t* at) {
    if (s.props_count) std::memcpy(at, s.props, s.props_count);
    std::memset(at + s.props_count, 0, VX_LIGHT_MAX_PROPS - s.props_count);
}

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

int vx_list_region(vx_context* ctx, const int32_t lo[3], const uint32_t size[3], uint32_t flags, int memory, vx_block_at* out, uint32_t capacity,
                   uint32_t* total) {
    static_assert(sizeof(vx_block_at) == 8, "the ABI's record size");
    if (memory != VX_MEM_HOST && memory != VX_MEM_DEVICE) return fail(VX_ERR_INVALID_ARGUMENT, "list_region: memory is neither VX_MEM_HOST nor VX_MEM_DEVICE");
    if (const char* what = vxb::check_list(lo, size, flags, out, capacity, total)) return fail(VX_ERR_INVALID_ARGUMENT, std::string("list_region: ") + what);
    if (memory == VX_MEM_DEVICE && reinterpret_cast<uintptr_t>(out) % 8) return fail(VX_ERR_INVALID_ARGUMENT, "list_region: out in device memory must be aligned to 8 bytes");
    if (memory == VX_MEM_DEVICE && reinterpret_cast<uintptr_t>(total) % 4) return fail(VX_ERR_INVALID_ARGUMENT, "list_region: total in device memory must be aligned to 4 bytes");
    if (!ctx) return fail(VX_ERR_INVALID_ARGUMENT, "null context");
    if (int rc = vxrt::check_ready(ctx)) return rc;
    VX_LOCK(ctx);
    const size_t voxels = size_t(size[0]) * size[1] * size[2];  // (at most 2^24, or 0)
    if (voxels == 0) {  // no record: only the count is written
        if (total && memory == VX_MEM_DEVICE) HIP_TRY(hipMemsetAsync(total, 0, sizeof(uint32_t), ctx->stream));
        else if (total) *total = 0;
        return VX_OK;
    }
    const vxb::Region r = vxb::plan_region(lo, size);
    const uint32_t bricks = uint32_t(vxb::region_bricks(r));  // (fewer than 2^24)
    uint32_t* counts = nullptr;
    if (int rc = reserve_list_counts(ctx, size_t(bricks) + 1, &counts)) return rc;
    const int variant = kernel_variant(ctx);
    const vxd::SceneArgs scene = vxrt::scene_on_bytes(ctx);

    if (memory == VX_MEM_DEVICE) {
        HIP_TRY(vxk::launch_list_count(variant, ctx->stream, scene, r, flags, counts));
        HIP_TRY(vxk::launch_list_offsets(ctx->stream, counts, bricks, total));
        if (capacity) HIP_TRY(vxk::launch_list_write(variant, ctx->stream, scene, r, flags, counts, out, capacity));
        return vxrt::mark_world_read(ctx);
    }

    // the total (16 bytes) | the records. Two waits: the total decides how many records the pool has to hold and the host copies back
    vxrt::PinnedPool& pool = vxrt::pinned_pool_of(ctx->device);
    std::lock_guard<std::mutex> pool_lock(pool.mutex);
    if (int rc = vxrt::pinned_pool_reserve(pool, 16)) return rc;
    HIP_TRY(vxk::launch_list_count(variant, ctx->stream, scene, r, flags, counts));
    HIP_TRY(vxk::launch_list_offsets(ctx->stream, counts, bricks, reinterpret_cast<uint32_t*>(pool.dev)));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    uint32_t found = 0;
    std::memcpy(&found, pool.host, sizeof found);
    const uint32_t written = found < capacity ? found : capacity;
    if (written) {
        if (int rc = vxrt::pinned_pool_reserve(pool, 16 + size_t(written) * sizeof(vx_block_at))) return rc;
        HIP_TRY(vxk::launch_list_write(variant, ctx->stream, scene, r, flags, counts, reinterpret_cast<vx_block_at*>(pool.dev + 16), written));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        std::memcpy(out, pool.host + 16, size_t(written) * sizeof(vx_block_at));
    }
    *total = found;
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

int vx_overlap_boxes(vx_context* ctx, const vx_box_batch* boxes, uint32_t count, int memory, vx_box_hit* out) {
    static_assert(sizeof(vx_box_hit) == 32, "the ABI's record size");
    if (memory != VX_MEM_HOST && memory != VX_MEM_DEVICE) return fail(VX_ERR_INVALID_ARGUMENT, "overlap_boxes: memory is neither VX_MEM_HOST nor VX_MEM_DEVICE");
    if (const char* what = vxb::check_boxes(boxes, count, out)) return fail(VX_ERR_INVALID_ARGUMENT, std::string("overlap_boxes: ") + what);
    if (count && memory == VX_MEM_DEVICE && reinterpret_cast<uintptr_t>(out) % 16) return fail(VX_ERR_INVALID_ARGUMENT, "overlap_boxes: out in device memory must be aligned to 16 bytes");
    if (!ctx) return fail(VX_ERR_INVALID_ARGUMENT, "null context");
    if (int rc = vxrt::check_ready(ctx)) return rc;
    VX_LOCK(ctx);
    if (count == 0) return VX_OK;

    if (memory == VX_MEM_DEVICE) {
        HIP_TRY(vxk::launch_overlap_boxes(kernel_variant(ctx), ctx->stream, vxrt::scene_on_bytes(ctx), boxes->origin, boxes->offset, boxes->extents,
                                          boxes->origin_stride, boxes->offset_stride, boxes->extents_stride, boxes->only_value, count, out));
        return vxrt::mark_world_read(ctx);
    }

    // the origins packed at stride 12 | the offsets (none; one; one a box) | the extents (one; one a box) | the records (at a multiple of 16):
    // each vector's bytes unchanged -- the kernel does the adds, as for device memory
    const auto packed = [count](const void* p, uint32_t stride) { return !p ? size_t(0) : (stride ? size_t(count) * 12 : size_t(12)); };
    const size_t at_offset = packed(boxes->origin, boxes->origin_stride), at_extents = at_offset + packed(boxes->offset, boxes->offset_stride);
    const size_t at_out = round16(at_extents + packed(boxes->extents, boxes->extents_stride)), out_bytes = size_t(count) * sizeof(vx_box_hit);
    vxrt::PinnedPool& pool = vxrt::pinned_pool_of(ctx->device);
    std::lock_guard<std::mutex> pool_lock(pool.mutex);
    if (int rc = vxrt::pinned_pool_reserve(pool, at_out + out_bytes)) return rc;
    const auto pack = [count, &pool](size_t at, const void* p, uint32_t stride) {
        const uint8_t* from = static_cast<const uint8_t*>(p);
        if (!p) return;
        if (stride == 12 || stride == 0) std::memcpy(pool.host + at, from, stride ? size_t(count) * 12 : size_t(12));
        else for (size_t i = 0; i < count; ++i) std::memcpy(pool.host + at + 12 * i, from + size_t(stride) * i, 12);  // (exactly a vector's bytes)
    };
    pack(0, boxes->origin, boxes->origin_stride);
    pack(at_offset, boxes->offset, boxes->offset_stride);
    pack(at_extents, boxes->extents, boxes->extents_stride);
    HIP_TRY(vxk::launch_overlap_boxes(kernel_variant(ctx), ctx->stream, vxrt::scene_on_bytes(ctx), pool.dev, boxes->offset ? pool.dev + at_offset : nullptr,
                                      pool.dev + at_extents, 12, boxes->offset_stride ? 12u : 0u, boxes->extents_stride ? 12u : 0u, boxes->only_value, count,
                                      reinterpret_cast<vx_box_hit*>(pool.dev + at_out)));
    HIP_TRY(hipStreamSynchronize(ctx->stream));  // synchronous, like vx_block_points' host-memory call
    std::memcpy(out, pool.host + at_out, out_bytes);
    return VX_OK;
}

int vx_move_boxes(vx_context* ctx, const vx_box_batch* boxes, const void* motion, uint32_t motion_stride, uint32_t count, const vx_move_shape* shape,
                  int memory, vx_move_hit* out) {
    static_assert(sizeof(vx_move_hit) == 48 && sizeof(vx_move_shape) == 16, "the ABI's record sizes");
    if (memory != VX_MEM_HOST && memory != VX_MEM_DEVICE) return fail(VX_ERR_INVALID_ARGUMENT, "move_boxes: memory is neither VX_MEM_HOST nor VX_MEM_DEVICE");
    if (const char* what = vxb::check_move(boxes, motion, motion_stride, count, shape, out)) return fail(VX_ERR_INVALID_ARGUMENT, std::string("move_boxes: ") + what);
    if (count && memory == VX_MEM_DEVICE && reinterpret_cast<uintptr_t>(out) % 16) return fail(VX_ERR_INVALID_ARGUMENT, "move_boxes: out in device memory must be aligned to 16 bytes");
    if (!ctx) return fail(VX_ERR_INVALID_ARGUMENT, "null context");
    if (int rc = vxrt::check_ready(ctx)) return rc;
    VX_LOCK(ctx);
    if (count == 0) return VX_OK;

    if (memory == VX_MEM_DEVICE) {
        HIP_TRY(vxk::launch_move_boxes(kernel_variant(ctx), ctx->stream, vxrt::scene_on_bytes(ctx), boxes->origin, boxes->offset, boxes->extents, motion,
                                       boxes->origin_stride, boxes->offset_stride, boxes->extents_stride, motion_stride, boxes->only_value, *shape, count, out));
        return vxrt::mark_world_read(ctx);
    }

    // vx_overlap_boxes' layout with the motions (one; one a box) behind the extents: each vector's bytes unchanged
    const auto packed = [count](const void* p, uint32_t stride) { return !p ? size_t(0) : (stride ? size_t(count) * 12 : size_t(12)); };
    const size_t at_offset = packed(boxes->origin, boxes->origin_stride), at_extents = at_offset + packed(boxes->offset, boxes->offset_stride);
    const size_t at_motion = at_extents + packed(boxes->extents, boxes->extents_stride);
    const size_t at_out = round16(at_motion + packed(motion, motion_stride)), out_bytes = size_t(count) * sizeof(vx_move_hit);
    vxrt::PinnedPool& pool = vxrt::pinned_pool_of(ctx->device);
    std::lock_guard<std::mutex> pool_lock(pool.mutex);
    if (int rc = vxrt::pinned_pool_reserve(pool, at_out + out_bytes)) return rc;
    const auto pack = [count, &pool](size_t at, const void* p, uint32_t stride) {
        const uint8_t* from = static_cast<const uint8_t*>(p);
        if (!p) return;
        if (stride == 12 || stride == 0) std::memcpy(pool.host + at, from, stride ? size_t(count) * 12 : size_t(12));
        else for (size_t i = 0; i < count; ++i) std::memcpy(pool.host + at + 12 * i, from + size_t(stride) * i, 12);  // (exactly a vector's bytes)
    };
    pack(0, boxes->origin, boxes->origin_stride);
    pack(at_offset, boxes->offset, boxes->offset_stride);
    pack(at_extents, boxes->extents, boxes->extents_stride);
    pack(at_motion, motion, motion_stride);
    HIP_TRY(vxk::launch_move_boxes(kernel_variant(ctx), ctx->stream, vxrt::scene_on_bytes(ctx), pool.dev, boxes->offset ? pool.dev + at_offset : nullptr,
                                   pool.dev + at_extents, pool.dev + at_motion, 12, boxes->offset_stride ? 12u : 0u, boxes->extents_stride ? 12u : 0u,
                                   motion_stride ? 12u : 0u, boxes->only_value, *shape, count, reinterpret_cast<vx_move_hit*>(pool.dev + at_out)));
    HIP_TRY(hipStreamSynchronize(ctx->stream));  // synchronous, like vx_overlap_boxes' host-memory call
    std::memcpy(out, pool.host + at_out, out_bytes);
    return VX_OK;
}

int vx_flood_points(vx_context* ctx, const void* pos, uint32_t pos_stride, uint32_t count, const vx_flood_shape* shape, int memory, uint8_t* fields,
                    uint32_t field_stride, vx_flood_info* info) {
    static_assert(sizeof(vx_flood_info) == 16 && sizeof(vx_flood_shape) == 36, "the ABI's record sizes");
    if (memory != VX_MEM_HOST && memory != VX_MEM_DEVICE) return fail(VX_ERR_INVALID_ARGUMENT, "flood_points: memory is neither VX_MEM_HOST nor VX_MEM_DEVICE");
    if (const char* what = vxb::check_flood(pos, pos_stride, count, shape, fields, field_stride, info)) return fail(VX_ERR_INVALID_ARGUMENT, std::string("flood_points: ") + what);
    if (count && memory == VX_MEM_DEVICE && reinterpret_cast<uintptr_t>(fields) % 16) return fail(VX_ERR_INVALID_ARGUMENT, "flood_points: fields in device memory must be aligned to 16 bytes");
    if (count && memory == VX_MEM_DEVICE && reinterpret_cast<uintptr_t>(info) % 16) return fail(VX_ERR_INVALID_ARGUMENT, "flood_points: info in device memory must be aligned to 16 bytes");
    if (!ctx) return fail(VX_ERR_INVALID_ARGUMENT, "null context");
    if (int rc = vxrt::check_ready(ctx)) return rc;
    VX_LOCK(ctx);
    if (count == 0) return VX_OK;
    const uint32_t voxels = vxb::flood_voxels(*shape), packed = vxb::flood_round16(voxels);
    const uint32_t stride = field_stride ? field_stride : packed;

    if (memory == VX_MEM_DEVICE) {
        HIP_TRY(vxk::launch_flood_points(kernel_variant(ctx), ctx->stream, vxrt::scene_on_bytes(ctx), pos, pos_stride, count, *shape, fields, stride, info));
        return vxrt::mark_world_read(ctx);
    }

    // the positions packed at stride 12 | the records (at a multiple of 16) | the fields, each the voxel count rounded up to 16: the bytes a
    // query writes, which go to the caller's stride from there
    const size_t at_info = round16(size_t(count) * 12), info_bytes = info ? size_t(count) * sizeof(vx_flood_info) : 0;
    const size_t at_fields = at_info + info_bytes, field_bytes = fields ? size_t(count) * packed : 0;
    vxrt::PinnedPool& pool = vxrt::pinned_pool_of(ctx->device);
    std::lock_guard<std::mutex> pool_lock(pool.mutex);
    if (int rc = vxrt::pinned_pool_reserve(pool, at_fields + field_bytes)) return rc;
    const uint8_t* from = static_cast<const uint8_t*>(pos);
    if (pos_stride == 12) std::memcpy(pool.host, from, size_t(count) * 12);
    else for (size_t i = 0; i < count; ++i) std::memcpy(pool.host + 12 * i, from + size_t(pos_stride) * i, 12);
    HIP_TRY(vxk::launch_flood_points(kernel_variant(ctx), ctx->stream, vxrt::scene_on_bytes(ctx), pool.dev, 12, count, *shape, fields ? pool.dev + at_fields : nullptr,
                                     packed, info ? reinterpret_cast<vx_flood_info*>(pool.dev + at_info) : nullptr));
    HIP_TRY(hipStreamSynchronize(ctx->stream));  // synchronous, like vx_block_points' host-memory call
    if (info) std::memcpy(info, pool.host + at_info, info_bytes);
    if (fields && stride == packed) std::memcpy(fields, pool.host + at_fields, field_bytes);
    else if (fields) for (size_t i = 0; i < count; ++i) std::memcpy(fields + i * stride, pool.host + at_fields + i * packed, packed);
    return VX_OK;
}

int vx_light_boxes(vx_context* ctx, const void* lo, uint32_t lo_stride, uint32_t count, const vx_light_shape* shape, int memory, uint8_t* fields,
                   uint32_t field_stride, vx_light_info* info) {
    static_assert(sizeof(vx_light_info) == 16 && sizeof(vx_light_shape) == 32, "the ABI's record sizes");
    if (memory != VX_MEM_HOST && memory != VX_MEM_DEVICE) return fail(VX_ERR_INVALID_ARGUMENT, "light_boxes: memory is neither VX_MEM_HOST nor VX_MEM_DEVICE");
    if (const char* what = vxb::check_light(lo, lo_stride, count, shape, fields, field_stride, info)) return fail(VX_ERR_INVALID_ARGUMENT, std::string("light_boxes: ") + what);
    if (count && memory == VX_MEM_DEVICE && reinterpret_cast<uintptr_t>(fields) % 16) return fail(VX_ERR_INVALID_ARGUMENT, "light_boxes: fields in device memory must be aligned to 16 bytes");
    if (count && memory == VX_MEM_DEVICE && reinterpret_cast<uintptr_t>(info) % 16) return fail(VX_ERR_INVALID_ARGUMENT, "light_boxes: info in device memory must be aligned to 16 bytes");
    if (!ctx) return fail(VX_ERR_INVALID_ARGUMENT, "null context");
    if (int rc = vxrt::check_ready(ctx)) return rc;
    VX_LOCK(ctx);
    if (count == 0) return VX_OK;
    const uint32_t voxels = vxb::light_voxels(shape->size), packed = vxb::light_round16(voxels);
    const uint32_t stride = field_stride ? field_stride : packed;

    if (memory == VX_MEM_DEVICE) {
        PropsRing& ring = props_ring_of(ctx->device);
        std::lock_guard<std::mutex> ring_lock(ring.mutex);
        PropsSlot* slot = nullptr;
        if (int rc = props_slot_acquire(ring, &slot)) return rc;
        fill_props(*shape, slot->host);
        slot->used = true;  // (from here on the stream may hold work that reads the slot)
        const hipError_t launched = vxk::launch_light_boxes(kernel_variant(ctx), ctx->stream, vxrt::scene_on_bytes(ctx), lo, lo_stride, count, shape->size, shape->flags,
                                                            slot->dev, fields, stride, info);
        HIP_TRY(props_slot_guard(ring, *slot, ctx->stream));
        HIP_TRY(launched);
        return vxrt::mark_world_read(ctx);
    }

    // the props | the boxes packed at stride 12 | the records (at a multiple of 16) | the fields, each the voxel count rounded up to 16: the
    // bytes a query writes, which go to the caller's stride from there
    const size_t at_lo = VX_LIGHT_MAX_PROPS, at_info = at_lo + round16(size_t(count) * 12), info_bytes = info ? size_t(count) * sizeof(vx_light_info) : 0;
    const size_t at_fields = at_info + info_bytes, field_bytes = fields ? size_t(count) * packed : 0;
    vxrt::PinnedPool& pool = vxrt::pinned_pool_of(ctx->device);
    std::lock_guard<std::mutex> pool_lock(pool.mutex);
    if (int rc = vxrt::pinned_pool_reserve(pool, at_fields + field_bytes)) return rc;
    fill_props(*shape, pool.host);
    const uint8_t* from = static_cast<const uint8_t*>(lo);
    if (lo_stride == 12) std::memcpy(pool.host + at_lo, from, size_t(count) * 12);
    else for (size_t i = 0; i < count; ++i) std::memcpy(pool.host + at_lo + 12 * i, from + size_t(lo_stride) * i, 12);
    HIP_TRY(vxk::launch_light_boxes(kernel_variant(ctx), ctx->stream, vxrt::scene_on_bytes(ctx), pool.dev + at_lo, 12, count, shape->size, shape->flags, pool.dev,
                                    fields ? pool.dev + at_fields : nullptr, packed, info ? reinterpret_cast<vx_light_info*>(pool.dev + at_info) : nullptr));
    HIP_TRY(hipStreamSynchronize(ctx->stream));  // synchronous, like vx_flood_points' host-memory call
    if (info) std::memcpy(info, pool.host + at_info, info_bytes);
    if (fields && stride == packed) std::memcpy(fields, pool.host + at_fields, field_bytes);
    else if (fields) for (size_t i = 0; i < count; ++i) std::memcpy(fields + i * stride, pool.host + at_fields + i * packed, packed);
    return VX_OK;
}

int vx_walk_points(vx_context* ctx, const void* pos, uint32_t pos_stride, const void* goal, uint32_t goal_stride, uint32_t count, const vx_walk_shape* shape, int memory,
                   uint8_t* fields, uint32_t field_stride, uint32_t* paths, vx_walk_info* info) {
    static_assert(sizeof(vx_walk_info) == 32 && sizeof(vx_walk_shape) == 52, "the ABI's record sizes");
    if (memory != VX_MEM_HOST && memory != VX_MEM_DEVICE) return fail(VX_ERR_INVALID_ARGUMENT, "walk_points: memory is neither VX_MEM_HOST nor VX_MEM_DEVICE");
    if (const char* what = vxb::check_walk(pos, pos_stride, goal, goal_stride, count, shape, fields, field_stride, paths, info))
        return fail(VX_ERR_INVALID_ARGUMENT, std::string("walk_points: ") + what);
    if (count && memory == VX_MEM_DEVICE && reinterpret_cast<uintptr_t>(fields) % 16) return fail(VX_ERR_INVALID_ARGUMENT, "walk_points: fields in device memory must be aligned to 16 bytes");
    if (count && memory == VX_MEM_DEVICE && reinterpret_cast<uintptr_t>(paths) % 16) return fail(VX_ERR_INVALID_ARGUMENT, "walk_points: paths in device memory must be aligned to 16 bytes");
    if (count && memory == VX_MEM_DEVICE && reinterpret_cast<uintptr_t>(info) % 16) return fail(VX_ERR_INVALID_ARGUMENT, "walk_points: info in device memory must be aligned to 16 bytes");
    if (!ctx) return fail(VX_ERR_INVALID_ARGUMENT, "null context");
    if (int rc = vxrt::check_ready(ctx)) return rc;
    VX_LOCK(ctx);
    if (count == 0) return VX_OK;
    const uint32_t voxels = vxb::walk_voxels(*shape), packed = vxb::flood_round16(voxels);
    const uint32_t stride = field_stride ? field_stride : packed;
    if (!shape->path_capacity) paths = nullptr;  // (no entry to write)
    if (!fields && !info && !paths) return VX_OK;  // (paths alone, of no entries: nothing is written)

    if (memory == VX_MEM_DEVICE) {
        HIP_TRY(vxk::launch_walk_points(kernel_variant(ctx), ctx->stream, vxrt::scene_on_bytes(ctx), pos, pos_stride, goal, goal_stride, count, *shape, fields, stride, paths, info));
        return vxrt::mark_world_read(ctx);
    }

    // the positions packed at stride 12 | the goals packed at stride 12, or the one goal | the records | the paths | the fields, each the
    // voxel count rounded up to 16: the bytes a query writes, which go to the caller's stride from there (every part at a multiple of 16)
    const size_t goals = goal ? (goal_stride ? size_t(count) : 1u) : 0u;
    const size_t at_goal = round16(size_t(count) * 12), at_info = at_goal + round16(goals * 12), info_bytes = info ? size_t(count) * sizeof(vx_walk_info) : 0;
    const size_t at_paths = at_info + info_bytes, path_bytes = paths ? size_t(count) * shape->path_capacity * 4u : 0;
    const size_t at_fields = at_paths + path_bytes, field_bytes = fields ? size_t(count) * packed : 0;
    vxrt::PinnedPool& pool = vxrt::pinned_pool_of(ctx->device);
    std::lock_guard<std::mutex> pool_lock(pool.mutex);
    if (int rc = vxrt::pinned_pool_reserve(pool, at_fields + field_bytes)) return rc;
    const uint8_t* from = static_cast<const uint8_t*>(pos);
    if (pos_stride == 12) std::memcpy(pool.host, from, size_t(count) * 12);
    else for (size_t i = 0; i < count; ++i) std::memcpy(pool.host + 12 * i, from + size_t(pos_stride) * i, 12);
    from = static_cast<const uint8_t*>(goal);
    if (goals && (goal_stride == 12 || goal_stride == 0)) std::memcpy(pool.host + at_goal, from, goals * 12);
    else for (size_t i = 0; i < goals; ++i) std::memcpy(pool.host + at_goal + 12 * i, from + size_t(goal_stride) * i, 12);
    HIP_TRY(vxk::launch_walk_points(kernel_variant(ctx), ctx->stream, vxrt::scene_on_bytes(ctx), pool.dev, 12, goal ? pool.dev + at_goal : nullptr, goal_stride ? 12u : 0u, count,
                                    *shape, fields ? pool.dev + at_fields : nullptr, packed, paths ? reinterpret_cast<uint32_t*>(pool.dev + at_paths) : nullptr,
                                    info ? reinterpret_cast<vx_walk_info*>(pool.dev + at_info) : nullptr));
    HIP_TRY(hipStreamSynchronize(ctx->stream));  // synchronous, like vx_flood_points' host-memory call
    if (info) std::memcpy(info, pool.host + at_info, info_bytes);
    if (paths) std::memcpy(paths, pool.host + at_paths, path_bytes);
    if (fields && stride == packed) std::memcpy(fields, pool.host + at_fields, field_bytes);
    else if (fields) for (size_t i = 0; i < count; ++i) std::memcpy(fields + i * stride, pool.host + at_fields + i * packed, packed);
    return VX_OK;
}

// libvoxelhip.so, the block entry points of include/voxel_hip.h (vx_block_points to vx_distance_boxes): each one's argument checks (the rules of
// the vx_*.hpp beside this file), the launches of its kernel (kernels_blocks.h), and for a host-memory call the pinned scratch the kernel
// reads and writes through (csrc/vx_pinned_pool.hpp), laid out and packed by vx_block_scratch.hpp: lay out, pack, launch, wait, copy out.
// A further translation unit on the context, like raycast_runtime.cpp: what it needs of the context is vx_context.hpp's (runtime.cpp).
#include <cstring>
#include <initializer_list>
#include <map>
#include <mutex>
#include <utility>

#include "kernels_blocks.h"
#include "vx_block_scratch.hpp"
#include "vx_context.hpp"
#include "vx_pinned_pool.hpp"

using vxrt::fail;

namespace {

// What every launch here takes of the context, picked once a call: the kernel variant, as vx_raycast picks it, and the world's own bytes.
struct OnBytes {
    int variant;
    vxd::SceneArgs scene;
    explicit OnBytes(const vx_context* ctx) : variant(ctx->big ? VX_SVO_ESVO_BIG : ctx->svo_type), scene(vxrt::scene_on_bytes(ctx)) {}
};

// The head of an entry point, its refusals in the order the ABI keeps, `who` in front of each: the memory kind; the entry point's own rule
// (`refused`: what its vxb::check_* says, or null); for a call `in_place` -- one in device memory that uses them -- each of `stored`, an
// output the kernel stores through where it lies, at a multiple of its `n`; a null context, or one that is not ready (vxrt::check_ready).
// The caller takes the context's lock next.
struct Stored { const void* p; uintptr_t n; const char* name; };
int enter(const char* who, int memory, const char* refused, bool in_place, std::initializer_list<Stored> stored, vx_context* ctx) {
    const auto refuse = [who](const std::string& what) { return fail(VX_ERR_INVALID_ARGUMENT, std::string(who) + ": " + what); };
    if (memory != VX_MEM_HOST && memory != VX_MEM_DEVICE) return refuse("memory is neither VX_MEM_HOST nor VX_MEM_DEVICE");
    if (refused) return refuse(refused);
    for (const Stored& s : stored)
        if (in_place && reinterpret_cast<uintptr_t>(s.p) % s.n) return refuse(std::string(s.name) + " in device memory must be aligned to " + std::to_string(s.n) + " bytes");
    return vxrt::check_ready(ctx);
}
// The tail of a device-memory call: its launch is queued on the context's stream, and a later commit waits for it.
int enqueued(vx_context* ctx, hipError_t launched) {
    HIP_TRY(launched);
    return vxrt::mark_world_read(ctx);
}

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
    if (int rc = enter("block_points", memory, vxb::check_points(pos, pos_stride, count, out), count && memory == VX_MEM_DEVICE, {{out, 8, "out"}}, ctx)) return rc;
    VX_LOCK(ctx);
    if (count == 0) return VX_OK;
    const OnBytes w(ctx);

    if (memory == VX_MEM_DEVICE) return enqueued(ctx, vxk::launch_block_points(w.variant, ctx->stream, w.scene, pos, pos_stride, count, out));

    // the positions packed at stride 12 | the records (at a multiple of 16)
    vxb::ScratchLayout lay;
    const size_t at_pos = lay.take(vxb::packed3_bytes(pos, pos_stride, count)), out_bytes = size_t(count) * sizeof(vx_block_cell), at_out = lay.take(out_bytes, 16);
    vxrt::PinnedScratch s(ctx);
    if (int rc = s.reserve(lay.end)) return rc;
    vxb::pack3(s.host() + at_pos, pos, pos_stride, count);
    HIP_TRY(vxk::launch_block_points(w.variant, ctx->stream, w.scene, s.dev() + at_pos, 12, count, reinterpret_cast<vx_block_cell*>(s.dev() + at_out)));
    if (int rc = s.wait()) return rc;  // synchronous, like vx_raycast_batch's host-memory call
    std::memcpy(out, s.host() + at_out, out_bytes);
    return VX_OK;
}

int vx_read_region(vx_context* ctx, const int32_t lo[3], const uint32_t size[3], int memory, uint32_t* out) {
    const char* refused = vxb::check_region(lo, size);
    const size_t voxels = refused ? 0 : size_t(size[0]) * size[1] * size[2];  // (at most 2^24, or 0)
    if (voxels && !out) refused = "null out";
    if (int rc = enter("read_region", memory, refused, memory == VX_MEM_DEVICE, {{out, 4, "out"}}, ctx)) return rc;
    VX_LOCK(ctx);
    if (voxels == 0) return VX_OK;
    const vxb::Region r = vxb::plan_region(lo, size);
    const OnBytes w(ctx);

    if (memory == VX_MEM_DEVICE) return enqueued(ctx, vxk::launch_read_region(w.variant, ctx->stream, w.scene, r, out));

    vxrt::PinnedScratch s(ctx);
    if (int rc = s.reserve(voxels * 4)) return rc;
    HIP_TRY(vxk::launch_read_region(w.variant, ctx->stream, w.scene, r, reinterpret_cast<uint32_t*>(s.dev())));
    if (int rc = s.wait()) return rc;
    std::memcpy(out, s.host(), voxels * 4);
    return VX_OK;
}

int vx_list_region(vx_context* ctx, const int32_t lo[3], const uint32_t size[3], uint32_t flags, int memory, vx_block_at* out, uint32_t capacity,
                   uint32_t* total) {
    static_assert(sizeof(vx_block_at) == 8, "the ABI's record size");
    if (int rc = enter("list_region", memory, vxb::check_list(lo, size, flags, out, capacity, total), memory == VX_MEM_DEVICE, {{out, 8, "out"}, {total, 4, "total"}}, ctx))
        return rc;
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
    const OnBytes w(ctx);

    if (memory == VX_MEM_DEVICE) {
        HIP_TRY(vxk::launch_list_count(w.variant, ctx->stream, w.scene, r, flags, counts));
        HIP_TRY(vxk::launch_list_offsets(ctx->stream, counts, bricks, total));
        if (capacity) HIP_TRY(vxk::launch_list_write(w.variant, ctx->stream, w.scene, r, flags, counts, out, capacity));
        return vxrt::mark_world_read(ctx);
    }

    // the total (16 bytes) | the records. Two waits: the total decides how many records the pool has to hold and the host copies back. The
    // second reserve may move the pool: the total has been read by then, and nothing of the first 16 bytes is needed afterwards.
    vxrt::PinnedScratch s(ctx);
    if (int rc = s.reserve(16)) return rc;
    HIP_TRY(vxk::launch_list_count(w.variant, ctx->stream, w.scene, r, flags, counts));
    HIP_TRY(vxk::launch_list_offsets(ctx->stream, counts, bricks, reinterpret_cast<uint32_t*>(s.dev())));
    if (int rc = s.wait()) return rc;
    uint32_t found = 0;
    std::memcpy(&found, s.host(), sizeof found);
    const uint32_t written = found < capacity ? found : capacity;
    if (written) {
        if (int rc = s.reserve(16 + size_t(written) * sizeof(vx_block_at))) return rc;
        HIP_TRY(vxk::launch_list_write(w.variant, ctx->stream, w.scene, r, flags, counts, reinterpret_cast<vx_block_at*>(s.dev() + 16), written));
        if (int rc = s.wait()) return rc;
        std::memcpy(out, s.host() + 16, size_t(written) * sizeof(vx_block_at));
    }
    *total = found;
    return VX_OK;
}

int vx_scan_points(vx_context* ctx, const void* pos, uint32_t pos_stride, uint32_t count, int direction, uint32_t reach, int memory, vx_scan_hit* out) {
    static_assert(sizeof(vx_scan_hit) == 16, "the ABI's record size");
    const char* refused = vxb::check_scan_points(pos, pos_stride, count, direction, reach, out);
    if (int rc = enter("scan_points", memory, refused, count && memory == VX_MEM_DEVICE, {{out, 16, "out"}}, ctx)) return rc;
    VX_LOCK(ctx);
    if (count == 0) return VX_OK;
    const OnBytes w(ctx);

    if (memory == VX_MEM_DEVICE) return enqueued(ctx, vxk::launch_scan_points(w.variant, ctx->stream, w.scene, pos, pos_stride, count, direction, reach, out));

    // the positions packed at stride 12 | the records (at a multiple of 16)
    vxb::ScratchLayout lay;
    const size_t at_pos = lay.take(vxb::packed3_bytes(pos, pos_stride, count)), out_bytes = size_t(count) * sizeof(vx_scan_hit), at_out = lay.take(out_bytes, 16);
    vxrt::PinnedScratch s(ctx);
    if (int rc = s.reserve(lay.end)) return rc;
    vxb::pack3(s.host() + at_pos, pos, pos_stride, count);
    HIP_TRY(vxk::launch_scan_points(w.variant, ctx->stream, w.scene, s.dev() + at_pos, 12, count, direction, reach, reinterpret_cast<vx_scan_hit*>(s.dev() + at_out)));
    if (int rc = s.wait()) return rc;
    std::memcpy(out, s.host() + at_out, out_bytes);
    return VX_OK;
}

int vx_scan_columns(vx_context* ctx, const int32_t lo[3], const uint32_t size[3], int direction, int memory, vx_scan_hit* out) {
    const char* refused = vxb::check_scan_columns(lo, size, direction);
    const vxb::Columns p = refused ? vxb::Columns{} : vxb::plan_columns(lo, size, direction);
    const size_t columns = !refused && size[0] && size[1] && size[2] ? size_t(p.size_u) * p.size_v : 0;  // (at most 2^24)
    if (columns && !out) refused = "null out";
    if (int rc = enter("scan_columns", memory, refused, memory == VX_MEM_DEVICE, {{out, 16, "out"}}, ctx)) return rc;
    VX_LOCK(ctx);
    if (columns == 0) return VX_OK;
    const OnBytes w(ctx);

    if (memory == VX_MEM_DEVICE) return enqueued(ctx, vxk::launch_scan_columns(w.variant, ctx->stream, w.scene, p, out));

    vxrt::PinnedScratch s(ctx);
    if (int rc = s.reserve(columns * sizeof(vx_scan_hit))) return rc;
    HIP_TRY(vxk::launch_scan_columns(w.variant, ctx->stream, w.scene, p, reinterpret_cast<vx_scan_hit*>(s.dev())));
    if (int rc = s.wait()) return rc;
    std::memcpy(out, s.host(), columns * sizeof(vx_scan_hit));
    return VX_OK;
}

int vx_overlap_boxes(vx_context* ctx, const vx_box_batch* boxes, uint32_t count, int memory, vx_box_hit* out) {
    static_assert(sizeof(vx_box_hit) == 32, "the ABI's record size");
    if (int rc = enter("overlap_boxes", memory, vxb::check_boxes(boxes, count, out), count && memory == VX_MEM_DEVICE, {{out, 16, "out"}}, ctx)) return rc;
    VX_LOCK(ctx);
    if (count == 0) return VX_OK;
    const OnBytes w(ctx);
    const auto launch = [&](const vx_box_batch& b, vx_box_hit* to) {
        return vxk::launch_overlap_boxes(w.variant, ctx->stream, w.scene, b.origin, b.offset, b.extents, b.origin_stride, b.offset_stride, b.extents_stride, b.only_value, count, to);
    };

    if (memory == VX_MEM_DEVICE) return enqueued(ctx, launch(*boxes, out));

    // the boxes as vx_block_scratch.hpp packs them | the records (at a multiple of 16)
    vxb::ScratchLayout lay;
    const size_t at_boxes = lay.take(vxb::packed_boxes_bytes(*boxes, count)), out_bytes = size_t(count) * sizeof(vx_box_hit), at_out = lay.take(out_bytes, 16);
    vxrt::PinnedScratch s(ctx);
    if (int rc = s.reserve(lay.end)) return rc;
    HIP_TRY(launch(vxb::pack_boxes(*boxes, count, s.host() + at_boxes, s.dev() + at_boxes), reinterpret_cast<vx_box_hit*>(s.dev() + at_out)));
    if (int rc = s.wait()) return rc;  // synchronous, like vx_block_points' host-memory call
    std::memcpy(out, s.host() + at_out, out_bytes);
    return VX_OK;
}

int vx_move_boxes(vx_context* ctx, const vx_box_batch* boxes, const void* motion, uint32_t motion_stride, uint32_t count, const vx_move_shape* shape,
                  int memory, vx_move_hit* out) {
    static_assert(sizeof(vx_move_hit) == 48 && sizeof(vx_move_shape) == 16, "the ABI's record sizes");
    const char* refused = vxb::check_move(boxes, motion, motion_stride, count, shape, out);
    if (int rc = enter("move_boxes", memory, refused, count && memory == VX_MEM_DEVICE, {{out, 16, "out"}}, ctx)) return rc;
    VX_LOCK(ctx);
    if (count == 0) return VX_OK;
    const OnBytes w(ctx);
    const auto launch = [&](const vx_box_batch& b, const void* moving, uint32_t moving_stride, vx_move_hit* to) {
        return vxk::launch_move_boxes(w.variant, ctx->stream, w.scene, b.origin, b.offset, b.extents, moving, b.origin_stride, b.offset_stride, b.extents_stride, moving_stride,
                                      b.only_value, *shape, count, to);
    };

    if (memory == VX_MEM_DEVICE) return enqueued(ctx, launch(*boxes, motion, motion_stride, out));

    // vx_overlap_boxes' layout with the motions (one; one a box) behind the extents, their bytes unchanged | the records (at a multiple of 16)
    vxb::ScratchLayout lay;
    const size_t at_boxes = lay.take(vxb::packed_boxes_bytes(*boxes, count)), at_motion = lay.take(vxb::packed3_bytes(motion, motion_stride, count));
    const size_t out_bytes = size_t(count) * sizeof(vx_move_hit), at_out = lay.take(out_bytes, 16);
    vxrt::PinnedScratch s(ctx);
    if (int rc = s.reserve(lay.end)) return rc;
    const vx_box_batch packed = vxb::pack_boxes(*boxes, count, s.host() + at_boxes, s.dev() + at_boxes);
    vxb::pack3(s.host() + at_motion, motion, motion_stride, count);
    HIP_TRY(launch(packed, s.dev() + at_motion, vxb::packed3_stride(motion_stride), reinterpret_cast<vx_move_hit*>(s.dev() + at_out)));
    if (int rc = s.wait()) return rc;  // synchronous, like vx_overlap_boxes' host-memory call
    std::memcpy(out, s.host() + at_out, out_bytes);
    return VX_OK;
}

int vx_flood_points(vx_context* ctx, const void* pos, uint32_t pos_stride, uint32_t count, const vx_flood_shape* shape, int memory, uint8_t* fields,
                    uint32_t field_stride, vx_flood_info* info) {
    static_assert(sizeof(vx_flood_info) == 16 && sizeof(vx_flood_shape) == 36, "the ABI's record sizes");
    const char* refused = vxb::check_flood(pos, pos_stride, count, shape, fields, field_stride, info);
    if (int rc = enter("flood_points", memory, refused, count && memory == VX_MEM_DEVICE, {{fields, 16, "fields"}, {info, 16, "info"}}, ctx)) return rc;
    VX_LOCK(ctx);
    if (count == 0) return VX_OK;
    const uint32_t packed = vxb::flood_round16(vxb::flood_voxels(*shape)), stride = field_stride ? field_stride : packed;
    const OnBytes w(ctx);

    if (memory == VX_MEM_DEVICE) return enqueued(ctx, vxk::launch_flood_points(w.variant, ctx->stream, w.scene, pos, pos_stride, count, *shape, fields, stride, info));

    // the positions packed at stride 12 | the records (at a multiple of 16) | the fields, each the voxel count rounded up to 16: the bytes a
    // query writes, which go to the caller's stride from there
    vxb::ScratchLayout lay;
    const size_t at_pos = lay.take(vxb::packed3_bytes(pos, pos_stride, count));
    const size_t info_bytes = info ? size_t(count) * sizeof(vx_flood_info) : 0, at_info = lay.take(info_bytes, 16);
    const size_t at_fields = lay.take(fields ? size_t(count) * packed : 0, 16);
    vxrt::PinnedScratch s(ctx);
    if (int rc = s.reserve(lay.end)) return rc;
    vxb::pack3(s.host() + at_pos, pos, pos_stride, count);
    HIP_TRY(vxk::launch_flood_points(w.variant, ctx->stream, w.scene, s.dev() + at_pos, 12, count, *shape, fields ? s.dev() + at_fields : nullptr, packed,
                                     info ? reinterpret_cast<vx_flood_info*>(s.dev() + at_info) : nullptr));
    if (int rc = s.wait()) return rc;  // synchronous, like vx_block_points' host-memory call
    if (info) std::memcpy(info, s.host() + at_info, info_bytes);
    if (fields) vxb::spread_fields(fields, stride, s.host() + at_fields, packed, count);
    return VX_OK;
}

int vx_light_boxes(vx_context* ctx, const void* lo, uint32_t lo_stride, uint32_t count, const vx_light_shape* shape, int memory, uint8_t* fields,
                   uint32_t field_stride, vx_light_info* info) {
    static_assert(sizeof(vx_light_info) == 16 && sizeof(vx_light_shape) == 32, "the ABI's record sizes");
    const char* refused = vxb::check_light(lo, lo_stride, count, shape, fields, field_stride, info);
    if (int rc = enter("light_boxes", memory, refused, count && memory == VX_MEM_DEVICE, {{fields, 16, "fields"}, {info, 16, "info"}}, ctx)) return rc;
    VX_LOCK(ctx);
    if (count == 0) return VX_OK;
    const uint32_t packed = vxb::light_round16(vxb::light_voxels(shape->size)), stride = field_stride ? field_stride : packed;
    const OnBytes w(ctx);

    if (memory == VX_MEM_DEVICE) {
        PropsRing& ring = props_ring_of(ctx->device);
        std::lock_guard<std::mutex> ring_lock(ring.mutex);
        PropsSlot* slot = nullptr;
        if (int rc = props_slot_acquire(ring, &slot)) return rc;
        fill_props(*shape, slot->host);
        slot->used = true;  // (from here on the stream may hold work that reads the slot)
        const hipError_t launched = vxk::launch_light_boxes(w.variant, ctx->stream, w.scene, lo, lo_stride, count, shape->size, shape->flags, slot->dev, fields, stride, info);
        HIP_TRY(props_slot_guard(ring, *slot, ctx->stream));
        return enqueued(ctx, launched);
    }

    // the props | the boxes packed at stride 12 | the records (at a multiple of 16) | the fields, each the voxel count rounded up to 16: the
    // bytes a query writes, which go to the caller's stride from there
    vxb::ScratchLayout lay;
    const size_t at_props = lay.take(VX_LIGHT_MAX_PROPS), at_lo = lay.take(vxb::packed3_bytes(lo, lo_stride, count), 16);
    const size_t info_bytes = info ? size_t(count) * sizeof(vx_light_info) : 0, at_info = lay.take(info_bytes, 16);
    const size_t at_fields = lay.take(fields ? size_t(count) * packed : 0, 16);
    vxrt::PinnedScratch s(ctx);
    if (int rc = s.reserve(lay.end)) return rc;
    fill_props(*shape, s.host() + at_props);
    vxb::pack3(s.host() + at_lo, lo, lo_stride, count);
    HIP_TRY(vxk::launch_light_boxes(w.variant, ctx->stream, w.scene, s.dev() + at_lo, 12, count, shape->size, shape->flags, s.dev() + at_props,
                                    fields ? s.dev() + at_fields : nullptr, packed, info ? reinterpret_cast<vx_light_info*>(s.dev() + at_info) : nullptr));
    if (int rc = s.wait()) return rc;  // synchronous, like vx_flood_points' host-memory call
    if (info) std::memcpy(info, s.host() + at_info, info_bytes);
    if (fields) vxb::spread_fields(fields, stride, s.host() + at_fields, packed, count);
    return VX_OK;
}

int vx_walk_points(vx_context* ctx, const void* pos, uint32_t pos_stride, const void* goal, uint32_t goal_stride, uint32_t count, const vx_walk_shape* shape, int memory,
                   uint8_t* fields, uint32_t field_stride, uint32_t* paths, vx_walk_info* info) {
    static_assert(sizeof(vx_walk_info) == 32 && sizeof(vx_walk_shape) == 52, "the ABI's record sizes");
    const char* refused = vxb::check_walk(pos, pos_stride, goal, goal_stride, count, shape, fields, field_stride, paths, info);
    if (int rc = enter("walk_points", memory, refused, count && memory == VX_MEM_DEVICE, {{fields, 16, "fields"}, {paths, 16, "paths"}, {info, 16, "info"}}, ctx)) return rc;
    VX_LOCK(ctx);
    if (count == 0) return VX_OK;
    const uint32_t packed = vxb::flood_round16(vxb::walk_voxels(*shape)), stride = field_stride ? field_stride : packed;
    if (!shape->path_capacity) paths = nullptr;  // (no entry to write)
    if (!fields && !info && !paths) return VX_OK;  // (paths alone, of no entries: nothing is written)
    const OnBytes w(ctx);

    if (memory == VX_MEM_DEVICE) return enqueued(ctx, vxk::launch_walk_points(w.variant, ctx->stream, w.scene, pos, pos_stride, goal, goal_stride, count, *shape, fields, stride, paths, info));

    // the positions packed at stride 12 | the goals packed at stride 12, or the one goal | the records | the paths | the fields, each the
    // voxel count rounded up to 16: the bytes a query writes, which go to the caller's stride from there (every part at a multiple of 16)
    vxb::ScratchLayout lay;
    const size_t at_pos = lay.take(vxb::packed3_bytes(pos, pos_stride, count)), at_goal = lay.take(vxb::packed3_bytes(goal, goal_stride, count), 16);
    const size_t info_bytes = info ? size_t(count) * sizeof(vx_walk_info) : 0, at_info = lay.take(info_bytes, 16);
    const size_t path_bytes = paths ? size_t(count) * shape->path_capacity * 4u : 0, at_paths = lay.take(path_bytes, 16);
    const size_t at_fields = lay.take(fields ? size_t(count) * packed : 0, 16);
    vxrt::PinnedScratch s(ctx);
    if (int rc = s.reserve(lay.end)) return rc;
    vxb::pack3(s.host() + at_pos, pos, pos_stride, count);
    vxb::pack3(s.host() + at_goal, goal, goal_stride, count);
    HIP_TRY(vxk::launch_walk_points(w.variant, ctx->stream, w.scene, s.dev() + at_pos, 12, goal ? s.dev() + at_goal : nullptr, vxb::packed3_stride(goal_stride), count, *shape,
                                    fields ? s.dev() + at_fields : nullptr, packed, paths ? reinterpret_cast<uint32_t*>(s.dev() + at_paths) : nullptr,
                                    info ? reinterpret_cast<vx_walk_info*>(s.dev() + at_info) : nullptr));
    if (int rc = s.wait()) return rc;  // synchronous, like vx_flood_points' host-memory call
    if (info) std::memcpy(info, s.host() + at_info, info_bytes);
    if (paths) std::memcpy(paths, s.host() + at_paths, path_bytes);
    if (fields) vxb::spread_fields(fields, stride, s.host() + at_fields, packed, count);
    return VX_OK;
}

int vx_label_boxes(vx_context* ctx, const void* lo, uint32_t lo_stride, uint32_t count, const vx_label_shape* shape, int memory, uint8_t* fields,
                   uint32_t field_stride, vx_label_piece* pieces, vx_label_info* info) {
    static_assert(sizeof(vx_label_info) == 32 && sizeof(vx_label_piece) == 16 && sizeof(vx_label_shape) == 32, "the ABI's record sizes");
    const char* refused = vxb::check_label(lo, lo_stride, count, shape, fields, field_stride, pieces, info);
    if (int rc = enter("label_boxes", memory, refused, count && memory == VX_MEM_DEVICE, {{fields, 16, "fields"}, {pieces, 16, "pieces"}, {info, 16, "info"}}, ctx)) return rc;
    VX_LOCK(ctx);
    if (count == 0) return VX_OK;
    const uint32_t packed = vxb::flood_round16(vxb::label_voxels(*shape)), stride = field_stride ? field_stride : packed;
    const OnBytes w(ctx);

    if (memory == VX_MEM_DEVICE) return enqueued(ctx, vxk::launch_label_boxes(w.variant, ctx->stream, w.scene, lo, lo_stride, count, *shape, fields, stride, pieces, info));

    // the boxes packed at stride 12 | the records | the piece records | the fields, each the voxel count rounded up to 16: the bytes a query
    // writes, which go to the caller's stride from there (every part behind the boxes at a multiple of 16)
    vxb::ScratchLayout lay;
    const size_t at_lo = lay.take(vxb::packed3_bytes(lo, lo_stride, count));
    const size_t info_bytes = info ? size_t(count) * sizeof(vx_label_info) : 0, at_info = lay.take(info_bytes, 16);
    const size_t piece_bytes = pieces ? size_t(count) * shape->max_pieces * sizeof(vx_label_piece) : 0, at_pieces = lay.take(piece_bytes, 16);
    const size_t at_fields = lay.take(fields ? size_t(count) * packed : 0, 16);
    vxrt::PinnedScratch s(ctx);
    if (int rc = s.reserve(lay.end)) return rc;
    vxb::pack3(s.host() + at_lo, lo, lo_stride, count);
    HIP_TRY(vxk::launch_label_boxes(w.variant, ctx->stream, w.scene, s.dev() + at_lo, 12, count, *shape, fields ? s.dev() + at_fields : nullptr, packed,
                                    pieces ? reinterpret_cast<vx_label_piece*>(s.dev() + at_pieces) : nullptr,
                                    info ? reinterpret_cast<vx_label_info*>(s.dev() + at_info) : nullptr));
    if (int rc = s.wait()) return rc;  // synchronous, like vx_light_boxes' host-memory call
    if (info) std::memcpy(info, s.host() + at_info, info_bytes);
    if (pieces) std::memcpy(pieces, s.host() + at_pieces, piece_bytes);
    if (fields) vxb::spread_fields(fields, stride, s.host() + at_fields, packed, count);
    return VX_OK;
}

int vx_distance_boxes(vx_context* ctx, const void* lo, uint32_t lo_stride, uint32_t count, const vx_distance_shape* shape, int memory, void* fields,
                      uint32_t field_stride, vx_distance_info* info) {
    static_assert(sizeof(vx_distance_info) == 16 && sizeof(vx_distance_shape) == 32, "the ABI's record sizes");
    const char* refused = vxb::check_distance(lo, lo_stride, count, shape, fields, field_stride, info);
    if (int rc = enter("distance_boxes", memory, refused, count && memory == VX_MEM_DEVICE, {{fields, 16, "fields"}, {info, 16, "info"}}, ctx)) return rc;
    VX_LOCK(ctx);
    if (count == 0) return VX_OK;
    const uint32_t packed = vxb::distance_field_bytes(*shape), stride = field_stride ? field_stride : packed;  // (bytes)
    const OnBytes w(ctx);

    if (memory == VX_MEM_DEVICE) return enqueued(ctx, vxk::launch_distance_boxes(w.variant, ctx->stream, w.scene, lo, lo_stride, count, *shape, static_cast<uint16_t*>(fields), stride, info));

    // the boxes packed at stride 12 | the records | the fields, each twice the voxel count rounded up to 16: the bytes a query writes, which
    // go to the caller's stride from there (every part behind the boxes at a multiple of 16)
    vxb::ScratchLayout lay;
    const size_t at_lo = lay.take(vxb::packed3_bytes(lo, lo_stride, count));
    const size_t info_bytes = info ? size_t(count) * sizeof(vx_distance_info) : 0, at_info = lay.take(info_bytes, 16);
    const size_t at_fields = lay.take(fields ? size_t(count) * packed : 0, 16);
    vxrt::PinnedScratch s(ctx);
    if (int rc = s.reserve(lay.end)) return rc;
    vxb::pack3(s.host() + at_lo, lo, lo_stride, count);
    HIP_TRY(vxk::launch_distance_boxes(w.variant, ctx->stream, w.scene, s.dev() + at_lo, 12, count, *shape,
                                       fields ? reinterpret_cast<uint16_t*>(s.dev() + at_fields) : nullptr, packed,
                                       info ? reinterpret_cast<vx_distance_info*>(s.dev() + at_info) : nullptr));
    if (int rc = s.wait()) return rc;  // synchronous, like vx_label_boxes' host-memory call
    if (info) std::memcpy(info, s.host() + at_info, info_bytes);
    if (fields) vxb::spread_fields(static_cast<uint8_t*>(fields), stride, s.host() + at_fields, packed, count);
    return VX_OK;
}

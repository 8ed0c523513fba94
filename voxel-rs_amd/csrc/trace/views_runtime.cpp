// libvoxelhip.so, many small views in one launch: vx_trace_views (include/voxel_hip.h) -- argument checks, the per-view camera constants (vx_view_params.hpp:
// view_params_of, evaluated here on the host as fill_params evaluates them for vx_render), the table of views the kernel reads, and the launch
// of kernels_views.hip. A further translation unit on the context, like trace_runtime.cpp, whose memory kinds, ordering and fences it shares.
#include <cstring>
#include <map>
#include <mutex>

#include "kernels_views.h"
#include "vx_context.hpp"
#include "vx_pinned_pool.hpp"

using vxd::ViewParams;
using vxrt::fail;

namespace {

constexpr uint64_t kMaxPixels = uint64_t(1) << 24;
constexpr uint32_t kMaxEdge = 8192;

size_t round16(size_t v) { return (v + 15) & ~size_t(15); }

// The table of a device-memory call, which returns before the launch has read it: a small ring of pinned host buffers with their device twins,
// each guarded by an event (like vx_commit's packed uploads, vx_context::DeltaSlot). A call fills the next slot's host buffer -- after waiting for
// the launch that last read the slot, four calls ago --, queues the copy to its twin and the launch behind it on the context's stream, and records the
// slot's event there. vx_context cannot grow (vx_pinned_pool.hpp), so the ring lives here: one per device, kept for the life of the process.
// A slot outlives the context that used it, and an event may not be waited for once the stream it was recorded on is destroyed (the runtime looks
// at that stream: a later context's call failed in hipEventSynchronize with whatever the freed stream's memory held by then). So the slot's event is
// recorded on a stream of the ring's own, which is never destroyed and waits for the launch through an event that lives for the call alone.
struct TableSlot {
    uint8_t* host = nullptr;
    uint8_t* dev = nullptr;
    size_t cap = 0;
    hipEvent_t done = nullptr;
    bool used = false;
};
struct TableRing {
    static constexpr unsigned kSlots = 4;
    std::mutex mutex;
    TableSlot slot[kSlots];
    unsigned next = 0;
    hipStream_t fence = nullptr;  // carries the slots' events; no work of its own
};

TableRing& table_ring_of(int device) {
    static std::mutex rings_mutex;
    static std::map<int, TableRing> rings;  // (node-based: a ring's address is stable)
    std::lock_guard<std::mutex> lock(rings_mutex);
    return rings[device];
}

// the ring's next slot, idle and at least `need` bytes, under the ring's mutex
int table_slot_acquire(TableRing& ring, size_t need, TableSlot** out) {
    TableSlot& s = ring.slot[ring.next++ % TableRing::kSlots];
    if (!s.done) HIP_TRY(hipEventCreateWithFlags(&s.done, hipEventDisableTiming));
    if (s.used) HIP_TRY(hipEventSynchronize(s.done));
    s.used = false;
    if (s.cap < need) {
        if (s.host) (void)hipHostFree(s.host);
        if (s.dev) (void)hipFree(s.dev);
        s.host = s.dev = nullptr;
        s.cap = 0;
        size_t cap = size_t(16) << 10;
        while (cap < need) cap *= 2;
        void *h = nullptr, *d = nullptr;
        HIP_TRY(hipHostMalloc(&h, cap, hipHostMallocDefault));
        if (const hipError_t e = hipMalloc(&d, cap); e != hipSuccess) {
            (void)hipHostFree(h);
            HIP_TRY(e);
        }
        s.host = static_cast<uint8_t*>(h);
        s.dev = static_cast<uint8_t*>(d);
        s.cap = cap;
    }
    *out = &s;
    return VX_OK;
}

// slot.done follows everything queued on `stream` so far, without belonging to it
hipError_t table_slot_guard(TableRing& ring, TableSlot& slot, hipStream_t stream) {
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

void fill_table(const vx_uniforms* views, uint32_t count, uint8_t* at) {
    ViewParams* table = reinterpret_cast<ViewParams*>(at);
    for (uint32_t k = 0; k < count; ++k) table[k] = vxd::view_params_of(views[k]);
}

}  // namespace

int vx_trace_views(vx_context* ctx, const vx_uniforms* views, uint32_t count, uint32_t width, uint32_t height, int memory, void* rgba, int format,
                   vx_hit* hits) {
    static_assert(sizeof(vx_hit) == 48, "the ABI's record size");
    // what needs no device comes first, and all of it before the context is looked at: the call itself, what is missing, the alignment
    if (memory != VX_MEM_HOST && memory != VX_MEM_DEVICE) return fail(VX_ERR_INVALID_ARGUMENT, "trace_views: memory is neither VX_MEM_HOST nor VX_MEM_DEVICE");
    if (format != VX_FORMAT_RGBA32F && format != VX_FORMAT_RGBA8) return fail(VX_ERR_INVALID_ARGUMENT, "trace_views: format is neither VX_FORMAT_RGBA32F nor VX_FORMAT_RGBA8");
    if (width == 0 || width > kMaxEdge) return fail(VX_ERR_INVALID_ARGUMENT, "trace_views: width must be 1 .. 8192");
    if (height == 0 || height > kMaxEdge) return fail(VX_ERR_INVALID_ARGUMENT, "trace_views: height must be 1 .. 8192");
    if (uint64_t(count) * width * height > kMaxPixels) return fail(VX_ERR_INVALID_ARGUMENT, "trace_views: count * width * height exceeds 16777216 (2^24) pixels");
    if (count && !views) return fail(VX_ERR_INVALID_ARGUMENT, "trace_views: null views");
    if (count && !rgba && !hits) return fail(VX_ERR_INVALID_ARGUMENT, "trace_views: null rgba and null hits (one of the two outputs is needed)");
    const size_t pixel = format == VX_FORMAT_RGBA8 ? 4 : 16;
    if (count && memory == VX_MEM_DEVICE) {  // the kernel stores whole pixels and 16-byte thirds of a record
        if (reinterpret_cast<uintptr_t>(rgba) % pixel) return fail(VX_ERR_INVALID_ARGUMENT, "trace_views: rgba in device memory must be aligned to a pixel");
        if (reinterpret_cast<uintptr_t>(hits) % 16) return fail(VX_ERR_INVALID_ARGUMENT, "trace_views: hits in device memory must be aligned to 16 bytes");
    }
    if (!ctx) return fail(VX_ERR_INVALID_ARGUMENT, "null context");
    if (int rc = vxrt::check_ready(ctx)) return rc;
    VX_LOCK(ctx);
    if (count == 0) return VX_OK;
    const int svo = ctx->big ? VX_SVO_ESVO_BIG : ctx->svo_type;  // the kernel variant, as vx_trace_rays picks it
    const size_t pixels = size_t(count) * width * height, table_bytes = size_t(count) * sizeof(ViewParams);

    if (memory == VX_MEM_DEVICE) {
        TableRing& ring = table_ring_of(ctx->device);
        std::lock_guard<std::mutex> ring_lock(ring.mutex);
        TableSlot* slot = nullptr;
        if (int rc = table_slot_acquire(ring, table_bytes, &slot)) return rc;
        fill_table(views, count, slot->host);
        HIP_TRY(hipMemcpyAsync(slot->dev, slot->host, table_bytes, hipMemcpyHostToDevice, ctx->stream));
        slot->used = true;  // (from here on the stream may hold work that reads the slot)
        const hipError_t launched = vxk::launch_trace_views(svo, ctx->stream, vxrt::scene_on_bytes(ctx), reinterpret_cast<const ViewParams*>(slot->dev), count,
                                                            width, height, rgba, format, hits);
        HIP_TRY(table_slot_guard(ring, *slot, ctx->stream));
        HIP_TRY(launched);
        return vxrt::mark_world_read(ctx);
    }

    // Host memory: the table | the pixels | the records (each at a multiple of 16), through the pinned pool; one launch, one wait
    const size_t rgba_bytes = rgba ? pixels * pixel : 0, hit_bytes = hits ? pixels * sizeof(vx_hit) : 0;
    const size_t at_rgba = round16(table_bytes), at_hits = round16(at_rgba + rgba_bytes);
    vxrt::PinnedPool& pool = vxrt::pinned_pool_of(ctx->device);
    std::lock_guard<std::mutex> pool_lock(pool.mutex);
    if (int rc = vxrt::pinned_pool_reserve(pool, at_hits + hit_bytes)) return rc;
    fill_table(views, count, pool.host);
    HIP_TRY(vxk::launch_trace_views(svo, ctx->stream, vxrt::scene_on_bytes(ctx), reinterpret_cast<const ViewParams*>(pool.dev), count, width, height,
                                    rgba ? pool.dev + at_rgba : nullptr, format, hits ? reinterpret_cast<vx_hit*>(pool.dev + at_hits) : nullptr));
    HIP_TRY(hipStreamSynchronize(ctx->stream));  // synchronous, like vx_trace_rays
    if (rgba) std::memcpy(rgba, pool.host + at_rgba, rgba_bytes);
    if (hits) std::memcpy(hits, pool.host + at_hits, hit_bytes);
    return VX_OK;
}

// Pinned scratch for the synchronous, host-memory calls of the modules beside csrc/hip (csrc/physics, csrc/raycast, csrc/trace, csrc/blocks): host records travel
// through pinned memory the device sees, which the kernel reads and writes directly -- no copy commands, one launch, one wait
// (vx_raycast in runtime.cpp: a synchronous call costs its round trips). vx_context cannot grow, so the scratch lives here: one grow-only pool
// per device, shared by that device's contexts and by the modules, whose mutex a host-memory call holds from its copy in to its copy out.
// Kept for the life of the process.
#pragma once

#include <cstddef>
#include <cstdint>
#include <map>
#include <mutex>

#include "vx_context.hpp"

namespace vxrt {

struct PinnedPool {
    std::mutex mutex;
    uint8_t* host = nullptr;
    uint8_t* dev = nullptr;
    size_t bytes = 0;
};

inline PinnedPool& pinned_pool_of(int device) {
    static std::mutex pools_mutex;
    static std::map<int, PinnedPool> pools;  // (node-based: a pool's address is stable)
    std::lock_guard<std::mutex> lock(pools_mutex);
    return pools[device];
}

// at least `need` bytes, under the pool's mutex
inline int pinned_pool_reserve(PinnedPool& p, size_t need) {
    if (p.bytes >= need) return VX_OK;
    if (p.host) (void)hipHostFree(p.host);  // (nobody's kernel reads it: every use is synchronous, under the pool's mutex)
    p.host = p.dev = nullptr;
    p.bytes = 0;
    size_t cap = size_t(64) << 10;
    while (cap < need) cap *= 2;
    void* h = nullptr;
    HIP_TRY(hipHostMalloc(&h, cap, hipHostMallocMapped));
    void* d = nullptr;
    if (const hipError_t e = hipHostGetDevicePointer(&d, h, 0); e != hipSuccess) {
        (void)hipHostFree(h);
        HIP_TRY(e);
    }
    p.host = static_cast<uint8_t*>(h);
    p.dev = static_cast<uint8_t*>(d);
    p.bytes = cap;
    return VX_OK;
}

// A host-memory call's hold on the pool of its context's device, created under the context's lock (VX_LOCK: the context first, then the
// pool) and kept from the copy in to the copy out: reserve, fill host(), launch on dev() -- the device's view of the same bytes --, wait,
// read host(). A further reserve may move the pool: host() and dev() are asked for again after it, and nothing of the old bytes is kept.
class PinnedScratch {
    const vx_context* ctx;
    PinnedPool& pool;
    std::lock_guard<std::mutex> lock;

public:
    explicit PinnedScratch(const vx_context* c) : ctx(c), pool(pinned_pool_of(c->device)), lock(pool.mutex) {}
    int reserve(size_t bytes) { return pinned_pool_reserve(pool, bytes); }
    uint8_t* host() const { return pool.host; }
    uint8_t* dev() const { return pool.dev; }
    int wait() { HIP_TRY(hipStreamSynchronize(ctx->stream)); return VX_OK; }  // everything queued on the context's stream is through
};

}  // namespace vxrt

// What a ray batch is (vx_ray_batch, include/voxel_hip.h), once for vx_raycast_batch and vx_trace_rays: its rules, the layout host arrays are
// packed to in pinned scratch, the block of arguments a kernel takes, and the gather at the head of both kernels. The standard library and
// voxel_hip.h only -- no HIP header, no HIP call -- so the host test harness compiles it as it stands (tests/cpp/batch_on_host.cpp).
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstring>
#include <string>

#include "voxel_hip.h"

namespace vxk {

// A vx_ray_batch as the kernel takes it: device-visible pointers, strides in bytes (0 = one value for every ray; the runtime has checked
// them). has_max_dst = 0: max_dst is not read and every ray gets max_dst_all. translucent picks vx_raycast_batch's kernel (cast_translucent
// is a constant of its code); vx_trace_rays does not read it.
struct RayBatchArgs {
    const void* origin;
    const void* dir;
    const void* max_dst;
    uint32_t origin_stride, dir_stride, max_dst_stride;
    float max_dst_all;
    uint32_t has_max_dst;
    uint32_t translucent;
};

}  // namespace vxk

namespace vxrt {

int fail(int code, const std::string& msg);  // (runtime.cpp: sets the calling thread's message, returns the code)

// vx_ray_batch's rules (voxel_hip.h); needs no device. `who` names the entry point in the message.
inline int check_ray_batch(const vx_ray_batch& r, const char* who) {
    const auto refuse = [who](const char* what) { return fail(VX_ERR_INVALID_ARGUMENT, std::string(who) + ": " + what); };
    if (r.flags & ~uint32_t(VX_RAYS_TRANSLUCENT)) return refuse("flags has a bit other than VX_RAYS_TRANSLUCENT");
    if (!r.origin) return refuse("null origin");
    if (!r.dir) return refuse("null dir");
    if (r.origin_stride % 4 || r.origin_stride < 12) return refuse("origin_stride must be a multiple of 4 and >= 12");
    if (r.dir_stride % 4 || (r.dir_stride && r.dir_stride < 12)) return refuse("dir_stride must be 0 or a multiple of 4 and >= 12");
    if (r.max_dst && r.max_dst_stride % 4) return refuse("max_dst_stride must be 0 or a multiple of 4");
    return VX_OK;
}

inline size_t round16(size_t v) { return (v + 15) & ~size_t(15); }

// Host arrays, packed: origins at stride 12 | directions at stride 12, or the one | distances at stride 4, the one, or none. An entry point
// appends its outputs from `end`, a multiple of 16.
struct RayPlan {
    size_t n_dir, n_dst;  // how many directions (n or 1) and distances (n, 1 or 0) are kept
    size_t at_dir, at_dst, end;
};

inline RayPlan plan_rays(const vx_ray_batch& r, size_t n) {
    RayPlan p = {};
    p.n_dir = r.dir_stride ? n : 1;
    p.n_dst = !r.max_dst ? 0 : (r.max_dst_stride ? n : 1);
    p.at_dir = 12 * n;
    p.at_dst = p.at_dir + 12 * p.n_dir;
    p.end = round16(p.at_dst + 4 * p.n_dst);
    return p;
}

// what every batch says whatever memory it lies in, and the arrays where they lie: a batch in device memory
inline vxk::RayBatchArgs rays_in_place(const vx_ray_batch& r) {
    vxk::RayBatchArgs a = {};
    a.origin = r.origin; a.dir = r.dir; a.max_dst = r.max_dst;
    a.origin_stride = r.origin_stride; a.dir_stride = r.dir_stride; a.max_dst_stride = r.max_dst_stride;
    a.max_dst_all = r.max_dst_all;
    a.has_max_dst = r.max_dst ? 1u : 0u;
    a.translucent = r.flags & VX_RAYS_TRANSLUCENT ? 1u : 0u;
    return a;
}

// `n` rays of host arrays packed to `host` as `p` lays them out (exactly the bytes of each value are read: an array may end with its last
// value); the arguments address the same bytes from `dev`, the device's view of `host`.
inline vxk::RayBatchArgs pack_rays(const vx_ray_batch& r, size_t n, const RayPlan& p, uint8_t* host, const uint8_t* dev) {
    const auto pack = [](uint8_t* to, const void* from, size_t stride, size_t width, size_t items) {
        const uint8_t* f = static_cast<const uint8_t*>(from);
        if (stride == width || items == 1) std::memcpy(to, f, width * items);
        else for (size_t i = 0; i < items; ++i) std::memcpy(to + width * i, f + stride * i, width);
    };
    pack(host, r.origin, r.origin_stride, 12, n);
    pack(host + p.at_dir, r.dir, r.dir_stride, 12, p.n_dir);
    if (p.n_dst) pack(host + p.at_dst, r.max_dst, r.max_dst_stride, 4, p.n_dst);
    vxk::RayBatchArgs a = rays_in_place(r);
    a.origin = dev; a.dir = dev + p.at_dir; a.max_dst = dev + p.at_dst;
    a.origin_stride = 12; a.dir_stride = p.n_dir == 1 ? 0 : 12; a.max_dst_stride = p.n_dst == n ? 4 : 0;
    return a;
}

}  // namespace vxrt

#if defined(__HIPCC__) || defined(VX_DEVICE_ON_HOST)
namespace vxk {

// A float[3] at base + i * stride: three dword loads in the source (a record only has to be 4-byte aligned).
__device__ __forceinline__ void load3(const uint8_t* __restrict__ base, uint32_t stride, uint32_t i, float out[3]) {
    const float* p = reinterpret_cast<const float*>(base + size_t(i) * stride);
    out[0] = p[0]; out[1] = p[1]; out[2] = p[2];
}

// Ray i of a batch, at the head of a kernel. Every argument but `i` is a kernel argument of the caller's, each pointer one of its own (not a
// member of a block), so the loads address global memory (no flat aperture check). A stride of 0 and has_max_dst are decided on the
// kernel argument: the branch is wave-uniform, no lane branches on a pointer, and the one value is read at one address in every lane.
// (__restrict__ is the kernel's to say, on its own arguments: said again here it changes how the code after the gather is scheduled.)
__device__ __forceinline__ void gather_ray(const uint8_t* origin, const uint8_t* dir, const uint8_t* max_dst, uint32_t origin_stride, uint32_t dir_stride,
                                           uint32_t max_dst_stride, float max_dst_all, uint32_t has_max_dst, uint32_t i, float ro[3], float rd[3], float& limit) {
    load3(origin, origin_stride, i, ro);
    if (dir_stride) {
        load3(dir, dir_stride, i, rd);
    } else {  // one direction for every ray
        const float* d = reinterpret_cast<const float*>(dir);
        rd[0] = d[0]; rd[1] = d[1]; rd[2] = d[2];
    }
    limit = max_dst_all;
    if (has_max_dst)
        limit = max_dst_stride ? *reinterpret_cast<const float*>(max_dst + size_t(i) * max_dst_stride) : *reinterpret_cast<const float*>(max_dst);
}

}  // namespace vxk
#endif

// TEST HARNESS ONLY: compiles vx_trace_rays' per-ray device code (voxel-rs_amd/csrc/trace/vx_trace.hpp, over vx_device.hpp) for the host with
// the shims of tests/cpp/shims, in the manner of device_on_host.cpp, so that the arithmetic can be held against the oracle without a GPU.
// Never linked into the product libraries; the product has no CPU path.
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#define __device__
#define __host__
#define __forceinline__ inline
#define __constant__ static const
#define __restrict__
struct uint4 { uint32_t x, y, z, w; };
struct float4 { float x, y, z, w; };
static inline float4 make_float4(float x, float y, float z, float w) { return float4{x, y, z, w}; }
struct uint2 { uint32_t x, y; };
static inline uint4 make_uint4(uint32_t x, uint32_t y, uint32_t z, uint32_t w) { return uint4{x, y, z, w}; }
static inline uint2 make_uint2(uint32_t x, uint32_t y) { return uint2{x, y}; }
static inline uint32_t __popc(uint32_t v) { return uint32_t(__builtin_popcount(v)); }
static inline int __clz(uint32_t v) { return v ? __builtin_clz(v) : 32; }
static inline uint32_t __float_as_uint(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }
static inline int32_t __float_as_int(float f) { int32_t u; std::memcpy(&u, &f, 4); return u; }
static inline float __uint_as_float(uint32_t u) { float f; std::memcpy(&f, &u, 4); return f; }
static inline float __int_as_float(int32_t u) { float f; std::memcpy(&f, &u, 4); return f; }
#define HIP_INCLUDE_HIP_HIP_RUNTIME_H  // keep <hip/hip_runtime.h> out
#define VX_DEVICE_ON_HOST 1
#include "vx_trace.hpp"

namespace vxd { unsigned char* vx_smem = nullptr; }
using namespace vxd;

// `n` rays as trace_rays_kernel (csrc/trace/kernels_trace.hip) traces them, one lane's stack: packed origins and directions (3 floats a ray), one
// max_dst a ray. rgba32f (4 floats a ray), rgba8 (one word a ray: pack_rgba8) and hits (vx_hit, through the three 16-byte words the kernel
// stores) are all written. The scene's arguments are devhost_ray_batch's.
extern "C" void tracehost_trace_rays(int svo_type, const uint8_t* world, uint64_t world_bytes, const vx_material* mats, uint32_t n_mats, const uint8_t* tex,
                                     uint32_t tw, uint32_t th, uint32_t layers, uint32_t levels, const uint32_t* level_offset, const vx_uniforms* uniforms,
                                     const float* origins, const float* dirs, const float* max_dst, uint32_t n, float* rgba32f, uint32_t* rgba8, vx_hit* hits) {
    SceneArgs sa = {};
    sa.world = world; sa.world_bytes = uint32_t(world_bytes); sa.materials = mats; sa.n_materials = n_mats;
    sa.tex = tex; sa.tex_bytes = 0;
    sa.width = tw; sa.height = th; sa.layers = layers; sa.levels = levels;
    for (uint32_t l = 0; l < levels && l < 16; ++l) {
        sa.level_offset[l] = level_offset[l];
        const uint32_t w = (tw >> l) ? (tw >> l) : 1, h = (th >> l) ? (th >> l) : 1;
        sa.tex_bytes = level_offset[l] + layers * w * h * 4;
    }
    const DevScene sc = make_scene(sa);
    const RenderParams p = vxt::params_of(*uniforms);
    std::vector<unsigned char> lds(Stack<1>::kBytes + 64);
    vx_smem = lds.data();
    StackSpill spill;
    Stack<1> st;
    st.init(0, &spill);
    for (uint32_t i = 0; i < n; ++i) {
        float color[4];
        vx_hit rec;
        if (svo_type == 1) vxt::trace_ray<1>(sc, p, origins + 3 * i, dirs + 3 * i, max_dst[i], st, color, rec);
        else vxt::trace_ray<2>(sc, p, origins + 3 * i, dirs + 3 * i, max_dst[i], st, color, rec);
        std::memcpy(rgba32f + 4 * i, color, 16);
        rgba8[i] = pack_rgba8(color);
        uint4 w[3];
        vxt::hit_words(rec, w);
        std::memcpy(reinterpret_cast<uint8_t*>(hits + i), w, 48);
    }
}

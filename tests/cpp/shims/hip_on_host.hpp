// TEST HARNESS ONLY: what the *_on_host.cpp harnesses put in front of the product's DEVICE headers (vx_device.hpp and what stands on it) so that g++
// compiles them for the host: plain-C++ stand-ins for the HIP qualifiers, vector types and bit built-ins, <hip/hip_runtime.h> kept out, and
// VX_DEVICE_ON_HOST for headers that hold device code beside host code. Include it before any product header, with this directory first on the
// include path: its vx_platform.hpp (plain C++) is then found instead of the product's (gfx950 built-ins).
#pragma once

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
#include "vx_args.hpp"

// The arguments of the scene of a world's own bytes as the harnesses' entries are handed it (the caller keeps them alive: a DevScene points into them)
static inline vxd::SceneArgs bytes_scene_args(const uint8_t* world, uint64_t world_bytes, const vx_material* mats, uint32_t n_mats, const uint8_t* tex, uint32_t tw, uint32_t th,
                            uint32_t layers, uint32_t levels, const uint32_t* level_offset) {
    vxd::SceneArgs sa = {};
    sa.world = world; sa.world_bytes = world_bytes; sa.materials = mats; sa.n_materials = n_mats;
    sa.tex = tex; sa.tex_bytes = 0;
    sa.width = tw; sa.height = th; sa.layers = layers; sa.levels = levels;
    for (uint32_t l = 0; l < levels && l < 16; ++l) {
        sa.level_offset[l] = level_offset[l];
        const uint32_t w = (tw >> l) ? (tw >> l) : 1, h = (th >> l) ? (th >> l) : 1;
        sa.tex_bytes = level_offset[l] + layers * w * h * 4;
    }
    return sa;
}

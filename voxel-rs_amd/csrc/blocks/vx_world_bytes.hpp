// vx_blocks.hpp's reader on a DevScene, for the kernels of kernels_blocks.hip and kernels_scan.hip: VX_SVO_ESVO and VX_SVO_CSVO through the
// buffer resource (range-checked by the hardware), VX_SVO_ESVO_BIG through Trav's 64-bit address with its explicit check. A read beyond the
// world gives 0.
#pragma once

#include <hip/hip_runtime.h>

#include "vx_blocks.hpp"
#include "vx_device.hpp"

namespace vxk {

template <int SVO>
struct WorldBytes {
    vxd::DevScene sc;
    __device__ __forceinline__ uint32_t head() const { return __float_as_uint(sc.octree_scale); }
    __device__ __forceinline__ uint32_t root_ptr() const { return sc.root_ptr; }
    __device__ __forceinline__ uint32_t word(uint32_t i) const { return vxd::Trav<SVO>::word(sc, i); }
    __device__ __forceinline__ uint32_t c32(uint32_t p) const { return vxd::csvo_u32(sc, p); }
    __device__ __forceinline__ uint32_t c8(uint32_t p) const { return vxd::csvo_u8(sc, p); }
};
template <int SVO>
constexpr int kFormat = SVO == VX_SVO_CSVO ? vxb::kCsvo : vxb::kEsvo;

}  // namespace vxk

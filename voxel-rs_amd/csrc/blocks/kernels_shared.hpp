// What the kernels of csrc/blocks (kernels_*.hip) share. A device header: it includes the HIP runtime and is no rule header -- the host
// harnesses compile vx_*.hpp and never this. Nothing here holds a barrier or zeroes LDS: what a kernel zeroes, and where its workgroup
// meets, stays written in the kernel.
//   a record's fold across a wave and across a workgroup's waves (fold_wave, fold_put, fold_take: walk, light, distance, move), the field's
//   16-byte stores from LDS (store_field: walk, light, distance), the records' stores (store_record: walk, light, distance, move, scan),
//   uniform(), load3_at, the launch by format (for_format: every launcher) and the five box launchers' two checks.
// NOT here, on measurement (profiles/box_kernels/README.md): the box workgroup's loading loop and the box's nine readfirstlanes stay
// written out in each of the five box kernels. As one function template over two callables (and a uniform_box beside it) they kept every
// LDS and register granule, but distance, label, light and flood ran 1 to 2.4 % slower in 11, 7, 15 and 29 rows of their per-call
// benchmarks, and the walk's CSVO builds took one register granule more. kernels_flood.hip, kernels_label.hip and kernels_boxes.hip also
// keep their own folds and stores: on the helpers above, rows of their benchmarks ran 0.3 to 1.1 % slower, and their device code compiles
// to the parent's instructions again. The cause was not found in the generated code in either case.
#pragma once

#include <hip/hip_runtime.h>

#include <type_traits>

#include "vx_blocks.hpp"

namespace vxk {

__device__ __forceinline__ uint32_t uniform(uint32_t v) { return uint32_t(__builtin_amdgcn_readfirstlane(int(v))); }

// A record's fold across the lanes of a wave: xor-shuffles by 32 ... 1, fold(a, other) after each; every lane ends with the wave's. T is
// moved as its 32-bit words, whatever their types: a float member travels as its bits.
template <class T, class Fold>
__device__ __forceinline__ void fold_wave(T& a, Fold&& fold) {
    static_assert(std::is_trivially_copyable<T>::value && sizeof(T) % 4u == 0, "a struct of 32-bit words");
    struct Words {
        uint32_t w[sizeof(T) / 4u];
    };
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        Words other = __builtin_bit_cast(Words, a);
#pragma unroll
        for (uint32_t k = 0; k < sizeof(T) / 4u; ++k) other.w[k] = uint32_t(__shfl_xor(int(other.w[k]), d, 64));
        fold(a, __builtin_bit_cast(T, other));
    }
}
// Across the waves through LDS: fold_put folds the wave and leaves lane 0's in slot[wave]; behind a barrier -- the kernel's, which it may
// share with something else -- fold_take combines the slots (in the one thread that wants the result, or in all).
template <class T, uint32_t WAVES, class Fold>
__device__ __forceinline__ void fold_put(T (&slot)[WAVES], uint32_t wave, uint32_t lane, T a, Fold&& fold) {
    fold_wave(a, fold);
    if (lane == 0) slot[wave] = a;
}
template <class T, uint32_t WAVES, class Fold>
__device__ __forceinline__ T fold_take(const T (&slot)[WAVES], Fold&& fold) {
    T all = slot[0];
#pragma unroll
    for (uint32_t v = 1; v < WAVES; ++v) fold(all, slot[v]);
    return all;
}

// A field leaves LDS: `chunks` 16-byte words from `from` to `to` (both 16-byte aligned), by the workgroup's `threads` threads.
__device__ __forceinline__ void store_field(uint8_t* to, const void* from, uint32_t chunks, uint32_t t, uint32_t threads) {
    uint4* const out = reinterpret_cast<uint4*>(to);
    const uint4* const in = reinterpret_cast<const uint4*>(from);
    for (uint32_t c = t; c < chunks; c += threads) out[c] = in[c];
}
// A record of 16, 32 or 48 bytes (16-byte aligned) as one, two or three 16-byte stores of ALL its words, padding included: a `_pad` the
// interface documents as "written 0" is the rule header's to zero (every vx_*.hpp constructor of such a record does), not this store's.
template <class R>
__device__ __forceinline__ void store_record(R* out, const R& r) {
    static_assert(std::is_trivially_copyable<R>::value && sizeof(R) % 16u == 0, "whole 16-byte stores");
    struct Words {
        uint4 w[sizeof(R) / 16u];
    };
    const Words words = __builtin_bit_cast(Words, r);
#pragma unroll
    for (uint32_t k = 0; k < sizeof(R) / 16u; ++k) reinterpret_cast<uint4*>(out)[k] = words.w[k];
}

__device__ __forceinline__ void load3_at(const uint8_t* base, size_t at, float out[3]) {
    const float* p = reinterpret_cast<const float*>(base + at);
    out[0] = p[0]; out[1] = p[1]; out[2] = p[2];
}

// The launch by format: launch(tag) with tag.value VX_SVO_ESVO_BIG, VX_SVO_ESVO or VX_SVO_CSVO as a constant, for a kernel's template
// argument. Any other svo is refused; else what the launch left behind.
template <class Launch>
inline hipError_t for_format(int svo, Launch&& launch) {
    if (svo == VX_SVO_ESVO_BIG) launch(std::integral_constant<int, VX_SVO_ESVO_BIG>{});
    else if (svo == VX_SVO_ESVO) launch(std::integral_constant<int, VX_SVO_ESVO>{});
    else if (svo == VX_SVO_CSVO) launch(std::integral_constant<int, VX_SVO_CSVO>{});
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

// The launchers' own checks of what a kernel indexes LDS by, whatever the caller checked: every size on 1..side; fields null, or their
// stride a multiple of 16 and at least `bytes`.
inline bool sizes_within(const uint32_t size[3], uint32_t side) {
    for (int a = 0; a < 3; ++a)
        if (size[a] == 0 || size[a] > side) return false;
    return true;
}
inline bool field_stride_ok(const void* fields, uint32_t stride, uint32_t bytes) { return !fields || (stride % 16u == 0 && stride >= bytes); }

}  // namespace vxk

// What a block entry point's host-memory call keeps in pinned scratch (csrc/vx_pinned_pool.hpp), once for all of blocks_runtime.cpp: the
// running layout of a call's parts, a float[3] or int32[3] array packed to 12 bytes an item, a vx_box_batch packed whole, and a query's field
// bytes spread to the caller's stride. The standard library and voxel_hip.h only -- no HIP header, no HIP call -- so a plain C++ program
// compiles it as it stands (tests/cpp/block_scratch_on_host.cpp).
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstring>

#include "voxel_hip.h"

namespace vxb {

// A call's parts one behind the other: `take` says where the next one starts -- at the end of the one before, rounded up to `align` (a power
// of two) -- and `end` is what the pool has to hold.
struct ScratchLayout {
    size_t end = 0;
    size_t take(size_t bytes, size_t align = 1) {
        const size_t at = (end + align - 1) & ~(align - 1);
        end = at + bytes;
        return at;
    }
};

// A float[3] or int32[3] input of `count` items at `stride` bytes. What it keeps when packed: nothing for a null array, one value for a
// stride of 0, else every item, 12 bytes each. The copy reads exactly an item's 12 bytes, never `stride`: an array may end with its last
// value. The kernel reads the packed bytes at packed3_stride.
inline size_t packed3_bytes(const void* p, uint32_t stride, size_t count) { return !p ? size_t(0) : (stride ? count * 12 : size_t(12)); }
inline uint32_t packed3_stride(uint32_t stride) { return stride ? 12u : 0u; }
inline void pack3(uint8_t* to, const void* p, uint32_t stride, size_t count) {
    const uint8_t* from = static_cast<const uint8_t*>(p);
    if (!p) return;
    if (stride == 12 || stride == 0 || count == 1) std::memcpy(to, from, packed3_bytes(p, stride, count));
    else for (size_t i = 0; i < count; ++i) std::memcpy(to + 12 * i, from + size_t(stride) * i, 12);
}

// A vx_box_batch of host arrays: the origins packed at stride 12 | the offsets (none; one; one a box) | the extents (one; one a box), nothing
// rounded between them and each vector's bytes unchanged -- the kernel does the adds, as for device memory. pack_boxes returns the batch the
// kernel takes: the same boxes in `host`, addressed from `dev`, the device's view of it.
inline size_t packed_boxes_bytes(const vx_box_batch& b, size_t count) {
    return packed3_bytes(b.origin, b.origin_stride, count) + packed3_bytes(b.offset, b.offset_stride, count) + packed3_bytes(b.extents, b.extents_stride, count);
}
inline vx_box_batch pack_boxes(const vx_box_batch& b, size_t count, uint8_t* host, const uint8_t* dev) {
    const size_t at_offset = packed3_bytes(b.origin, b.origin_stride, count), at_extents = at_offset + packed3_bytes(b.offset, b.offset_stride, count);
    pack3(host, b.origin, b.origin_stride, count);
    pack3(host + at_offset, b.offset, b.offset_stride, count);
    pack3(host + at_extents, b.extents, b.extents_stride, count);
    vx_box_batch k = b;
    k.origin = dev; k.offset = b.offset ? dev + at_offset : nullptr; k.extents = dev + at_extents;
    k.origin_stride = 12; k.offset_stride = packed3_stride(b.offset_stride); k.extents_stride = packed3_stride(b.extents_stride);
    return k;
}

// `count` fields of `packed` bytes, as a kernel wrote them one behind the other, to the caller's `stride`: only a field's own bytes are
// written, what lies between two fields stays the caller's.
inline void spread_fields(uint8_t* to, size_t stride, const uint8_t* from, size_t packed, size_t count) {
    if (stride == packed) std::memcpy(to, from, count * packed);
    else for (size_t i = 0; i < count; ++i) std::memcpy(to + i * stride, from + i * packed, packed);
}

}  // namespace vxb

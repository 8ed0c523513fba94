// vx_overlap_boxes' kernel (gfx950): vx_boxes.hpp's answer for a batch of float boxes, the world's own bytes read as kernels_blocks.hip reads
// them (vx_world_bytes.hpp: a read beyond the world gives 0). The world is read-only for the launch. No LDS, no atomic, no memory between
// bricks; no kernel waits for another workgroup.
//   a workgroup (one wave) owns one box, blockIdx.x its number.
//   1  every lane reads the box's nine floats through the strides at the same address (scalar loads in the code) and works out the cover; the
//      cover, its validity and its brick range go through readfirstlane, so that everything above a brick -- the loop over the bricks,
//      enter_brick_at's descent -- runs on scalar registers and wave-uniform addresses, as in kernels_list.hip where the brick comes from
//      blockIdx: in the disassembly the descent is one buffer load at a uniform address and a readfirstlane a word, with scalar branches
//      and no waterfall loop. The lanes keep their own copy of the cover in VGPRs for their tests: it keeps the SGPRs below the limit.
//   2  no box, or a cover with no voxel: lane 0 writes the record, the wave leaves with no load from the world.
//   3  the bricks of the cover, x fastest: a brick of air, or one leaf above the brick that only_value refuses, is skipped by a scalar branch;
//      one leaf above the brick that counts (a LOD voxel of side 8 or more) is folded in with no load; else lane l takes column
//      (l & 7, l >> 3) with vxb::brick_column (lanes whose column lies outside the cover load nothing).
//   4  per lane: the count, min and max of x, y, z, the smallest key with its value (vxb::BoxAcc); folded ONCE across the wave after the last
//      brick by 6 x 9 xor-shuffles.
//   5  lane 0 writes the record as two 16-byte stores.
// Registers (hipcc -Rpass-analysis=kernel-resource-usage, ESVO / CSVO / ESVO beyond 4 GiB): 76 / 87 / 74 VGPRs, 67 / 83 / 66 SGPRs.
// No spill, no scratch, no LDS in any of the three.
// The fold and the record's store below are deliberately the ones from before kernels_shared.hpp (uniform(), load3_at and the launcher come
// from the header): on fold_wave and store_record one row of profiles/boxes_bench.py (ESVO, 256 boxes of 64^3) ran 1 % slower in two
// visits (profiles/box_kernels/README.md), and the cause was not found in the generated code.
#include <hip/hip_runtime.h>

#include "kernels_blocks.h"
#include "kernels_shared.hpp"
#include "vx_device.hpp"
#include "vx_world_bytes.hpp"

using namespace vxd;
using vxk::kFormat;
using vxk::WorldBytes;
using vxk::load3_at;
using vxk::uniform;

namespace {

__device__ __forceinline__ void store_record(vx_box_hit* out, const vx_box_hit& h) {
    uint4* const o = reinterpret_cast<uint4*>(out);
    o[0] = make_uint4(h.blocks, h.value, uint32_t(h.lo[0]), uint32_t(h.lo[1]));
    o[1] = make_uint4(uint32_t(h.lo[2]), uint32_t(h.hi[0]), uint32_t(h.hi[1]), uint32_t(h.hi[2]));
}

// (each pointer a kernel argument of its own, as in vx_ray_batch.hpp's gather: the loads address global memory; has_offset and the strides
// are decided on kernel arguments: wave-uniform branches)
template <int SVO>
__global__ __launch_bounds__(64) void overlap_boxes_kernel(SceneArgs sa, const uint8_t* __restrict__ origin, const uint8_t* __restrict__ offset,
                                                           const uint8_t* __restrict__ extents, uint32_t origin_stride, uint32_t offset_stride,
                                                           uint32_t extents_stride, uint32_t has_offset, uint32_t only_value,
                                                           vx_box_hit* __restrict__ out) {
    const WorldBytes<SVO> w = {make_scene(sa)};
    const uint32_t n = blockIdx.x, lane = threadIdx.x;
    float o[3], f[3] = {0.0f, 0.0f, 0.0f}, e[3];
    load3_at(origin, size_t(n) * origin_stride, o);
    if (has_offset) load3_at(offset, size_t(n) * offset_stride, f);
    load3_at(extents, size_t(n) * extents_stride, e);
    // cv: the cover as the lanes hold it (VGPRs, for their own tests); c: the same through readfirstlane (SGPRs, for everything above a brick)
    const vxb::Cover cv = vxb::box_cover(o, f, e, has_offset != 0, vxb::depth_of(w.head()));
    vxb::Cover c;
    c.valid = uniform(cv.valid);
    c.some = uniform(cv.some);
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        c.first[a] = int32_t(uniform(uint32_t(cv.first[a])));
        c.last[a] = int32_t(uniform(uint32_t(cv.last[a])));
    }
    if (!c.valid || !c.some) {  // (wave-uniform) no load from the world
        if (lane == 0) store_record(out + n, c.valid ? vxb::box_record(vxb::box_acc_none()) : vxb::box_invalid());
        return;
    }
    const vxb::BoxBricks r = vxb::cover_bricks(c);  // (of uniform values: scalar)
    const uint32_t i = lane & 7u, j = lane >> 3;
    vxb::BoxAcc acc = vxb::box_acc_none();
    const uint32_t end_x = r.corner[0] + r.count[0] * vxb::kBrick, end_y = r.corner[1] + r.count[1] * vxb::kBrick, end_z = r.corner[2] + r.count[2] * vxb::kBrick;
#pragma nounroll
    for (uint32_t cx = r.corner[0], cy = r.corner[1], cz = r.corner[2]; cz != end_z;) {  // the bricks of the cover, x fastest
        const vxb::Brick b = vxb::enter_brick_at<kFormat<SVO>>(w, cx, cy, cz);                // (wave-uniform)
        if (!vxb::box_brick_skipped(b, only_value)) vxb::box_brick_lane<kFormat<SVO>>(w, cv, only_value, b, i, j, acc);  // (a scalar branch)
        cx += vxb::kBrick;
        if (cx == end_x) {
            cx = r.corner[0];
            cy += vxb::kBrick;
            if (cy == end_y) cy = r.corner[1], cz += vxb::kBrick;
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        vxb::BoxAcc other;
        other.count = uint32_t(__shfl_xor(int(acc.count), d, 64));
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            other.mn[a] = __shfl_xor(acc.mn[a], d, 64);
            other.mx[a] = __shfl_xor(acc.mx[a], d, 64);
        }
        other.key = uint32_t(__shfl_xor(int(acc.key), d, 64));
        other.value = uint32_t(__shfl_xor(int(acc.value), d, 64));
        vxb::box_fold(acc, other);
    }
    if (lane == 0) store_record(out + n, vxb::box_record(acc));
}

}  // namespace

namespace vxk {

hipError_t launch_overlap_boxes(int svo, hipStream_t stream, const SceneArgs& sc, const void* origin, const void* offset, const void* extents,
                                uint32_t origin_stride, uint32_t offset_stride, uint32_t extents_stride, uint32_t only_value, uint32_t count,
                                vx_box_hit* out) {
    static_assert(sizeof(vx_box_hit) == 32, "two 16-byte stores");
    if (count == 0 || count > vxb::kMaxCount) return hipErrorInvalidValue;
    const dim3 grid(count, 1, 1), block(64);  // (a grid's x may be as large as 2^31 - 1)
    const uint8_t *po = static_cast<const uint8_t*>(origin), *pf = static_cast<const uint8_t*>(offset), *pe = static_cast<const uint8_t*>(extents);
    const uint32_t has_offset = offset ? 1u : 0u;
    return for_format(svo, [&](auto f) {
        hipLaunchKernelGGL((overlap_boxes_kernel<decltype(f)::value>), grid, block, 0, stream, sc, po, pf, pe, origin_stride, offset_stride, extents_stride, has_offset,
                           only_value, out);
    });
}

}  // namespace vxk

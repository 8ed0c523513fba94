// vx_block_points' and vx_read_region's kernels (gfx950): vx_blocks.hpp's descent of a point through the world's own bytes, read through the
// buffer resources the picker and the ray batches read them through (vx_device.hpp: a read beyond the world gives 0). The world is read-only
// for the whole launch. Neither kernel uses LDS or an atomic.
//   points  64 lanes a workgroup, one point a lane, gathered through the stride as kernels_raycast.hip gathers origins (vx_ray_batch.hpp's
//           load3); the whole descent per lane; one 8-byte store a lane.
//   region  a workgroup (one wave) owns one brick of 8 x 8 x 8 voxels aligned to the world grid. Everything above the brick hangs on
//           blockIdx and kernel arguments alone: the wave descends it once, through wave-uniform addresses (every lane asks for the same
//           word: one cache line a load). Lane l then takes the column (x, y) = (l & 7, l >> 3) of the brick and runs the last three
//           levels for its eight z level by level (vxb::brick_column: 2 + 4 + 8 steps, a level's steps independent of one another). A
//           brick whose own descent ended above it (empty space, a LOD voxel of 8 and more, outside the world) is filled with no further
//           load: a wave-uniform branch in brick_column, a scalar branch around the lanes' loads in the code. Eight consecutive lanes
//           hold eight consecutive x: a store instruction writes eight whole 32-byte runs. Lanes outside the box store nothing.
// Registers (hipcc -Rpass-analysis=kernel-resource-usage, ESVO / CSVO / ESVO beyond 4 GiB): points 16 / 18 / 18 VGPRs, region 40 / 56 / 40;
// no spill, no scratch, no LDS in any of the six.
#include <hip/hip_runtime.h>

#include "kernels_blocks.h"
#include "kernels_shared.hpp"
#include "vx_device.hpp"
#include "vx_ray_batch.hpp"
#include "vx_world_bytes.hpp"

using namespace vxd;

namespace {

using vxk::kFormat;
using vxk::WorldBytes;  // (vx_world_bytes.hpp: vx_blocks.hpp's reader on a DevScene)

template <int SVO>
__global__ __launch_bounds__(64) void block_points_kernel(SceneArgs sa, const uint8_t* __restrict__ pos, uint32_t pos_stride, uint32_t n,
                                                          vx_block_cell* __restrict__ out) {
    const WorldBytes<SVO> w = {make_scene(sa)};
    const uint32_t i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    float p[3];
    vxk::load3(pos, pos_stride, i, p);
    const vx_block_cell c = vxb::cell_at_point<kFormat<SVO>>(w, p);
    *reinterpret_cast<uint2*>(out + i) = make_uint2(c.value, c.cell_log2);
}

template <int SVO>
__global__ __launch_bounds__(64) void read_region_kernel(SceneArgs sa, vxb::Region r, uint32_t* __restrict__ out) {
    const WorldBytes<SVO> w = {make_scene(sa)};
    const vxb::Brick b = vxb::enter_brick<kFormat<SVO>>(w, r, blockIdx.x);  // (wave-uniform)
    const uint32_t i = threadIdx.x & 7u, j = threadIdx.x >> 3;
    uint32_t value[vxb::kBrick];
    vxb::brick_column<kFormat<SVO>>(w, b, i, j, value);
#pragma unroll
    for (uint32_t k = 0; k < vxb::kBrick; ++k) {
        uint32_t index;
        if (vxb::box_index(r, b, i, j, k, index)) out[index] = value[k];
    }
}

}  // namespace

namespace vxk {

hipError_t launch_block_points(int svo, hipStream_t stream, const SceneArgs& sc, const void* pos, uint32_t pos_stride, uint32_t count, vx_block_cell* out) {
    static_assert(sizeof(vx_block_cell) == 8, "one 8-byte store");
    const dim3 grid((count + 63u) / 64u), block(64);
    const uint8_t* p = static_cast<const uint8_t*>(pos);
    return for_format(svo, [&](auto f) { hipLaunchKernelGGL((block_points_kernel<decltype(f)::value>), grid, block, 0, stream, sc, p, pos_stride, count, out); });
}

hipError_t launch_read_region(int svo, hipStream_t stream, const SceneArgs& sc, const vxb::Region& r, uint32_t* out) {
    const uint64_t bricks = vxb::region_bricks(r);
    if (bricks == 0 || bricks > 0x7fffffffull) return hipErrorInvalidValue;  // (a region of 2^24 voxels has fewer than 2^24 bricks)
    const dim3 grid(static_cast<uint32_t>(bricks), 1, 1), block(64);
    return for_format(svo, [&](auto f) { hipLaunchKernelGGL((read_region_kernel<decltype(f)::value>), grid, block, 0, stream, sc, r, out); });
}

}  // namespace vxk

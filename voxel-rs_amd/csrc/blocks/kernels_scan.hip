// vx_scan_points' and vx_scan_columns' kernels (gfx950): vx_scan.hpp's walk along an axis through the world's own bytes, read as
// kernels_blocks.hip reads them (vx_world_bytes.hpp: a read beyond the world gives 0). The world is read-only for the whole launch. Neither
// kernel uses LDS or an atomic; the columns kernel's one cross-lane operation is the vote that ends a wave's walk.
//   points   64 lanes a workgroup, one position a lane, gathered through the stride as block_points_kernel gathers it; the lane walks its
//            own column, every trip a descent from the root, an empty cell stepped over at a time; one 16-byte store a lane. Lanes of a
//            wave diverge: neighbouring points need not be neighbours in the world.
//   columns  a workgroup (one wave) owns a tile of 8 x 8 columns aligned to the world grid, lane l the column (l & 7, l >> 3). The walk's
//            coordinate, the descent to the brick that holds it and the step beyond an empty cell hang on blockIdx and kernel arguments
//            alone: wave-uniform addresses (every lane asks for the same word), scalar branches. Only the last three levels, for a lane's
//            eight voxels along the axis, are per lane -- and skipped by the whole wave where the brick's descent ended above it. The wave
//            leaves the loop when no lane is open any more. Eight consecutive lanes hold eight consecutive u: a store instruction writes
//            eight whole 128-byte runs. Lanes outside the box store nothing.
// Registers (hipcc -Rpass-analysis=kernel-resource-usage, ESVO / CSVO / ESVO beyond 4 GiB): points 29 / 34 / 30 VGPRs, columns 79 / 95 / 82;
// no spill, no scratch, no LDS in any of the six.
#include <hip/hip_runtime.h>

#include "kernels_blocks.h"
#include "kernels_shared.hpp"
#include "vx_device.hpp"
#include "vx_ray_batch.hpp"
#include "vx_world_bytes.hpp"

using namespace vxd;
using namespace vxk;

namespace {

template <int SVO>
__global__ __launch_bounds__(64) void scan_points_kernel(SceneArgs sa, const uint8_t* __restrict__ pos, uint32_t pos_stride, uint32_t n,
                                                         uint32_t direction, uint32_t reach, vx_scan_hit* __restrict__ out) {
    const WorldBytes<SVO> w = {make_scene(sa)};
    const uint32_t i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    float p[3];
    vxk::load3(pos, pos_stride, i, p);
    uint32_t trips = 0;  // (the harness's figure: dead here)
    store_record(out + i, vxb::scan_point<kFormat<SVO>>(w, p, direction, reach, trips));
}

template <int SVO>
__global__ __launch_bounds__(64) void scan_columns_kernel(SceneArgs sa, vxb::Columns p, vx_scan_hit* __restrict__ out) {
    const WorldBytes<SVO> w = {make_scene(sa)};
    const vxb::ColumnTile t = vxb::enter_tile(w, p, blockIdx.x);  // (wave-uniform)
    const uint32_t i = threadIdx.x & 7u, j = threadIdx.x >> 3;
    vx_scan_hit hit = vxb::scan_none();
    if (t.small) {
        uint32_t trips = 0;
        hit = vxb::tile_lane_small<kFormat<SVO>>(w, p, t, i, j, trips);
    } else if (t.walk) {
        uint32_t c = p.positive ? t.first : t.last;  // (wave-uniform, like the brick and the step)
        bool open = true;
        for (;;) {
            const vxb::Brick b = vxb::tile_brick<kFormat<SVO>>(w, p, t, c);
            if (open) open = !vxb::tile_lane<kFormat<SVO>>(w, p, t, b, c, i, j, hit);
            if (!__any(open) || !vxb::tile_advance(p, t, b, c)) break;
        }
    }
    uint32_t index;
    if (vxb::column_index(p, t, i, j, index)) store_record(out + index, hit);
}

}  // namespace

namespace vxk {

hipError_t launch_scan_points(int svo, hipStream_t stream, const SceneArgs& sc, const void* pos, uint32_t pos_stride, uint32_t count, int direction,
                              uint32_t reach, vx_scan_hit* out) {
    static_assert(sizeof(vx_scan_hit) == 16, "one 16-byte store");
    const dim3 grid((count + 63u) / 64u), block(64);
    const uint8_t* p = static_cast<const uint8_t*>(pos);
    const uint32_t dir = static_cast<uint32_t>(direction);
    return for_format(svo, [&](auto f) { hipLaunchKernelGGL((scan_points_kernel<decltype(f)::value>), grid, block, 0, stream, sc, p, pos_stride, count, dir, reach, out); });
}

hipError_t launch_scan_columns(int svo, hipStream_t stream, const SceneArgs& sc, const vxb::Columns& p, vx_scan_hit* out) {
    const uint64_t tiles = vxb::column_tiles(p);
    if (tiles == 0 || tiles > 0x7fffffffull) return hipErrorInvalidValue;  // (a footprint of 2^24 columns has fewer than 2^23 tiles)
    const dim3 grid(static_cast<uint32_t>(tiles), 1, 1), block(64);
    return for_format(svo, [&](auto f) { hipLaunchKernelGGL((scan_columns_kernel<decltype(f)::value>), grid, block, 0, stream, sc, p, out); });
}

}  // namespace vxk

// vx_distance_boxes' kernel (gfx950): vx_distance.hpp's exact squared distance to the nearest target cell for a batch of boxes, the world's
// own bytes read as kernels_blocks.hip reads them (vx_world_bytes.hpp: a read beyond the world gives 0). The world is read-only for the
// launch. No global atomic, no LDS atomic; no workgroup waits for another. Every loop bound is a kernel argument or a constant -- the sizes
// (<= 32) and the brick counts (<= 5 an axis), which the launcher checks again whatever the caller checked -- and no loop or branch around a
// barrier depends on what the world holds: a query's time is bounded, and every thread reaches each of the three barriers.
//   a workgroup of 256 threads (4 waves) owns one box, blockIdx.x its number.
//   1  every thread reads lo at the same address (scalar loads in the code); the box and its bricks through readfirstlane: everything above
//      a brick runs on scalar registers and wave-uniform addresses.
//   2  loading, as kernels_flood.hip loads: wave v takes the brick rows v, v + 4, ... of the cover, enters each brick once (enter_brick_at)
//      and has lane l read the column along x at (y, z) = (l & 7, l >> 3) (vxb::flood_brick_lane; with a match_value a second time under
//      that value, see vx_distance.hpp); after the last brick along x the lane stores its row's target word (vxb::distance_row) into LDS:
//      one lane holds a row, a plain store. (Why each box kernel writes this loop out: kernels_shared.hpp.)
//   3  pass y: thread t owns the columns (x, z) = (t & 31, (t >> 5) + 8 k), k = 0..3, along y. It reads the row words of its z -- the threads
//      of one z read the same words --, takes its x's distance from each (vxb::distance_row_x), keeps the line of 32 in registers, runs the
//      pass entry by entry (vxb::distance_pass_at) and writes 16-bit values into the LDS array, which is laid out as the field is: entry
//      (z * size.y + y) * size.x + x.
//   4  pass z: thread t owns the columns (x, y) = (t & 31, (t >> 5) + 8 k) along z: its entries into registers, the pass, the final values
//      back in place -- the column is its own --, and the record's fold (vxb::distance_fold_cell) from the values in registers; then
//      across the workgroup (fold_put, fold_take with vxb::distance_fold: three LDS words a wave).
//   5  the field leaves LDS as 16-byte stores (store_field), the entries behind the last cell written VX_DISTANCE_NONE in LDS before;
//      thread 0 stores the 16-byte record in one store (store_record).
// One build a format: records need `farthest`, so a records-only call runs both passes and needs the same 64 KiB between them; only the
// stores of step 5 are left out (fields == NULL is a kernel argument).
// Registers (hipcc -Rpass-analysis=kernel-resource-usage, ESVO / CSVO / ESVO beyond 4 GiB): 245 / 245 / 245 VGPRs, 91 / 106 / 95 SGPRs. No
// spill, no scratch in any of the three. LDS: 69,680 bytes (64 KiB of entries, 4 KiB of rows, 48 bytes of fold words): two workgroups a CU
// under the 160 KiB, which 245 registers a thread allow as well (two waves a SIMD by the compiler's count).
#include <hip/hip_runtime.h>

#include "kernels_blocks.h"
#include "kernels_shared.hpp"
#include "vx_device.hpp"
#include "vx_world_bytes.hpp"

using namespace vxd;
using namespace vxk;

namespace {

// A uniform value the compiler may not carry across this point: the 32 comparisons of a line's length with a constant are made where a
// trip of the loop over the owned columns needs them, not ahead of the loop, where they would fill the scalar registers.
__device__ __forceinline__ uint32_t fresh(uint32_t v) {
    asm volatile("" : "+s"(v));
    return v;
}

constexpr uint32_t kWaves = vxb::kFloodThreads / 64u;

struct DistanceLds {
    alignas(16) uint16_t dist[vxb::kDistanceCells];  // 64 KiB: the rounded field fits (2 * 32,768 bytes is a multiple of 16)
    uint32_t rows[vxb::kFloodRows];
    vxb::DistanceAcc fold[kWaves];
};

template <int SVO>
__global__ __launch_bounds__(256) void distance_boxes_kernel(SceneArgs sa, const uint8_t* __restrict__ lo, uint32_t lo_stride, vx_distance_shape s,
                                                             uint8_t* __restrict__ fields, uint32_t field_stride, vx_distance_info* __restrict__ info) {
    __shared__ DistanceLds lds;
    const WorldBytes<SVO> w = {make_scene(sa)};
    const uint32_t n = blockIdx.x, t = threadIdx.x, lane = t & 63u, wave = uniform(t >> 6);
    const uint32_t voxels = vxb::distance_voxels(s), chunks = vxb::distance_field_bytes(s) / 16u;

    // 1  the box
    int32_t at[3];
    {
        const int32_t* q = reinterpret_cast<const int32_t*>(lo + size_t(n) * lo_stride);
        at[0] = q[0]; at[1] = q[1]; at[2] = q[2];
    }
    vxb::FloodBox box = vxb::distance_box(at, s);
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        box.lo[a] = uniform(box.lo[a]);
        box.first[a] = uniform(box.first[a]);
        box.count[a] = uniform(box.count[a]);
    }

    // 2  loading: the target rows (every row of the box is some lane's; the others are never used)
    {
        const vx_flood_shape load0 = vxb::distance_load_shape(s, false), load1 = vxb::distance_load_shape(s, true);
        const bool twice = vxb::distance_loads_twice(s);  // (a kernel argument: uniform)
        const uint32_t i = lane & 7u, j = lane >> 3, brick_rows = box.count[1] * box.count[2];
#pragma nounroll
        for (uint32_t m = wave; m < brick_rows; m += kWaves) {  // (wave-uniform)
            const uint32_t cy = box.first[1] + (m % box.count[1]) * vxb::kBrick, cz = box.first[2] + (m / box.count[1]) * vxb::kBrick;
            uint32_t first = 0u, second = 0u, unused = 0u;
#pragma nounroll
            for (uint32_t bx = 0; bx < box.count[0]; ++bx) {
                const vxb::Brick b = vxb::enter_brick_at<kFormat<SVO>>(w, box.first[0] + bx * vxb::kBrick, cy, cz);
                vxb::flood_brick_lane<kFormat<SVO>>(w, load0, box, b, i, j, first, unused);
                if (twice) vxb::flood_brick_lane<kFormat<SVO>>(w, load1, box, b, i, j, second, unused);
            }
            const uint32_t ry = cy + i - box.lo[1], rz = cz + j - box.lo[2];
            if (ry < s.size[1] && rz < s.size[2]) lds.rows[vxb::flood_row_of(ry, rz)] = vxb::distance_row(s, first, second);
        }
    }
    __syncthreads();

    const uint32_t rx = t & (vxb::kFloodSide - 1u), r0 = t >> 5;
    uint32_t in[vxb::kFloodSide];

    // 3  pass y. A line's 32 inputs stay in registers; each output is stored as soon as it is there (sched_barrier: the compiler may not
    // run the 32 outputs' sums side by side, which took more than 256 registers). Rows and entries behind the line's end are read at its
    // last index instead: a copy of the last entry, farther away than the entry itself, is never the minimum, and the index stays in the box.
#pragma nounroll
    for (uint32_t k = 0; k < vxb::kFloodOwned; ++k) {
        const uint32_t rz = r0 + 8u * k;
        s.size[1] = fresh(s.size[1]);
        if (rx < s.size[0] && rz < s.size[2]) {
#pragma unroll
            for (uint32_t ry = 0; ry < vxb::kFloodSide; ++ry) in[ry] = vxb::distance_row_x(lds.rows[vxb::flood_row_of(min(ry, s.size[1] - 1u), rz)], rx);
#pragma unroll
            for (uint32_t ry = 0; ry < vxb::kFloodSide; ++ry) {
                if (ry < s.size[1]) lds.dist[vxb::distance_entry(s, rx, ry, rz)] = uint16_t(vxb::distance_pass_at(in, ry));
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    }
    if (t < 8u && voxels + t < chunks * 8u) lds.dist[voxels + t] = uint16_t(vxb::kDistanceNone);  // (behind the last cell: no pass touches them)
    __syncthreads();

    // 4  pass z, in place -- every entry of the column is in registers before the first is overwritten --, and the fold
    vxb::DistanceAcc acc = vxb::distance_acc();
#pragma nounroll
    for (uint32_t k = 0; k < vxb::kFloodOwned; ++k) {
        const uint32_t ry = r0 + 8u * k;
        s.size[2] = fresh(s.size[2]);
        if (rx < s.size[0] && ry < s.size[1]) {
#pragma unroll
            for (uint32_t rz = 0; rz < vxb::kFloodSide; ++rz) in[rz] = lds.dist[vxb::distance_entry(s, rx, ry, min(rz, s.size[2] - 1u))];
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (uint32_t rz = 0; rz < vxb::kFloodSide; ++rz) {
                if (rz < s.size[2]) {
                    const uint32_t value = vxb::distance_pass_at(in, rz);
                    lds.dist[vxb::distance_entry(s, rx, ry, rz)] = uint16_t(value);
                    vxb::distance_fold_cell(acc, s, rx, ry, rz, value);
                }
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    }
    fold_put(lds.fold, wave, lane, acc, vxb::distance_fold);
    __syncthreads();

    // 5  the record, the field
    if (info && t == 0) store_record(info + n, vxb::distance_record(fold_take(lds.fold, vxb::distance_fold), s));  // (info: a kernel argument)
    if (fields) store_field(fields + size_t(n) * field_stride, lds.dist, chunks, t, vxb::kFloodThreads);
}

}  // namespace

namespace vxk {

hipError_t launch_distance_boxes(int svo, hipStream_t stream, const SceneArgs& sc, const void* lo, uint32_t lo_stride, uint32_t count, const vx_distance_shape& shape,
                                 uint16_t* fields, uint32_t field_stride, vx_distance_info* info) {
    static_assert(sizeof(vx_distance_info) == 16, "one 16-byte store");
    if (count == 0 || count > vxb::kDistanceMaxCount || (!fields && !info) || !lo) return hipErrorInvalidValue;
    // the kernel's own bounds, whatever the caller checked: rows and entries of LDS are indexed by these, and its loops end by them
    if (!sizes_within(shape.size, vxb::kFloodSide)) return hipErrorInvalidValue;
    if ((shape.flags & ~uint32_t(VX_DISTANCE_TO_AIR)) || (shape.match_value && shape.pass_value)) return hipErrorInvalidValue;
    if (!field_stride_ok(fields, field_stride, 2u * vxb::distance_voxels(shape))) return hipErrorInvalidValue;
    const dim3 grid(count, 1, 1), block(vxb::kFloodThreads);
    const uint8_t* p = static_cast<const uint8_t*>(lo);
    uint8_t* const f = reinterpret_cast<uint8_t*>(fields);
    return for_format(svo, [&](auto fmt) {
        hipLaunchKernelGGL((distance_boxes_kernel<decltype(fmt)::value>), grid, block, 0, stream, sc, p, lo_stride, shape, f, field_stride, info);
    });
}

}  // namespace vxk

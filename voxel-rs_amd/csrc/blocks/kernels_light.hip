// vx_light_boxes' kernel (gfx950): vx_light.hpp's sky and block light for a batch of boxes, the world's own bytes read as kernels_blocks.hip
// reads them (vx_world_bytes.hpp: a read beyond the world gives 0). The world is read-only for the launch. No global atomic, no LDS atomic
// but the one word __syncthreads_or reduces into; no workgroup waits for another; every loop bound is a kernel argument or a constant (the
// exposure's scan goes up by at least one voxel a trip: the world's height bounds it).
//   a workgroup of 256 threads (4 waves) owns one query, blockIdx.x its number.
//   1  the table of props, 4 KiB with zeros behind props_count, into LDS as dwords; the box at one address (scalar loads), it and its
//      bricks through readfirstlane.
//   2  loading, as kernels_flood.hip loads: wave v takes the brick rows v, v + 4, ... of the cover (at most 7 x 7), enters each brick along x
//      once (enter_brick_at) and has lane l read the column along x at (y, z) = (l & 7, l >> 3) (vxb::light_brick_lane); after the last brick
//      the lane stores its five rows -- passable, four emission planes -- into LDS: one lane holds a row, plain stores. (Why each box
//      kernel writes this loop out: kernels_shared.hpp.)
//   3  exposure above the box (not under VX_LIGHT_NO_SKY): wave v takes z = v, v + 4, ...; lane x runs the column's chain of scan_line
//      (vxb::column_open); the 64 answers are the word of that z by one ballot.
//   4  thread t owns rows t + 256 k, k = 0..8: (y, z) = (r % 48, r / 48). It takes its passable row and its emission planes into REGISTERS;
//      from here on the same LDS holds the two 64-bit frontiers, which the neighbours read.
//   5  exposure inside the box goes THROUGH LDS: thread z < size.z walks its slab from the top y downwards, ANDing the open word with the
//      passable rows where the loader left them and writing the exposed row over each -- the sky's first frontier in place. 48 threads, 48
//      dependent LDS round trips at most; an ownership by slabs would have cost the spread its consecutive addresses.
//   6  the sky channel: 14 steps at most of vxb::light_step from the current frontier into the other, one __syncthreads_or a step which every
//      thread reaches; a step that finds nothing ends it. Then the block channel the same way in the same frontiers, its level planes
//      starting as the emission planes (sources_L: the planes say L); it ends when no frontier and no unreached source is left.
//   7  the levels of both channels stay in registers as 2 x 4 bit planes a row (144 VGPRs): no read-modify-write of bytes in global memory,
//      which byte stores from 64 different rows a wave would have made of it. At the end the owners expand their rows to bytes in LDS, in
//      vx_read_region's layout, at most 92,160 bytes a pass (two passes from 45^3 on), and the workgroup stores them as 16-byte words
//      (store_field).
//   8  the record: folded across the workgroup (fold_put, fold_take: 16 LDS words), one 16-byte store (store_record).
//   FIELD == false (fields == NULL): step 7's expansion and stores are left out; the planes are still what the record is read from.
// Resources (hipcc -Rpass-analysis=kernel-resource-usage), the same with and without FIELD -- the planes and the loader set them, not the
// expansion --, ESVO / CSVO / ESVO beyond 4 GiB: 256 VGPRs and 5 AGPRs in each of the six; 79 / 105 / 82 SGPRs; no VGPR spill, no SGPR spill,
// no scratch. The 5 AGPRs are the register allocator's own overflow of the 256 architectural registers (copies, not memory): the 144
// registers of planes, 36 of passable and reached rows and the descent's live set do not fit beside one another in 256. LDS: 96,960 bytes
// (92,160 of the arena, 4 KiB of props, the open words and the fold). So one workgroup a CU and one wave a SIMD, by LDS and by registers
// alike: a call of up to 256 boxes runs every box at once, a larger one in rounds of 256. Measured: profiles/light/results.json.
#include <hip/hip_runtime.h>

#include "kernels_blocks.h"
#include "kernels_shared.hpp"
#include "vx_device.hpp"
#include "vx_world_bytes.hpp"

using namespace vxd;
using namespace vxk;

namespace {

constexpr uint32_t kWaves = vxb::kLightThreads / 64u;
constexpr uint32_t kRowBytes = vxb::kLightRows * 8u;  // one 64-bit row each: 18,432
constexpr uint32_t kArena = 5u * kRowBytes;           // the loaded rows (passable, four planes) | the two frontiers | the field's staging
static_assert(kArena % 16u == 0, "a pass of the field ends on a 16-byte word");

struct LightLds {
    alignas(16) uint8_t arena[kArena];
    uint64_t open[vxb::kLightSide];
    vxb::LightAcc fold[kWaves];
    alignas(16) uint8_t props[VX_LIGHT_MAX_PROPS];
};

__device__ __forceinline__ void light_fold(vxb::LightAcc& a, const vxb::LightAcc& b) {
    a.lit += b.lit, a.sources += b.sources, a.open_columns += b.open_columns, a.faces |= b.faces;
}

// One channel's steps (vx_light.hpp: the spread) on the thread's rows; frontier 0 holds the first frontier, `reached` its rows.
template <bool SOURCES>
__device__ __forceinline__ void run_channel(uint64_t* frontier0, uint64_t* frontier1, const uint32_t size[3], uint32_t t, const uint64_t (&passable)[vxb::kLightOwned],
                                            uint64_t (&reached)[vxb::kLightOwned], vxb::LightLevels (&v)[vxb::kLightOwned]) {
#pragma nounroll
    for (uint32_t step = 0; step < vxb::kLightSteps; ++step) {
        const uint32_t level = vxb::kLightSteps - step;
        const uint64_t* const cur = (step & 1u) ? frontier1 : frontier0;
        uint64_t* const next = (step & 1u) ? frontier0 : frontier1;
        uint64_t any = 0u;
        // (the thread's number through an empty asm each step: where its rows lie in the box is worked out again, a few instructions a row,
        // and not kept across the loop as 45 lane masks, which are more scalar registers than there are)
        uint32_t tt = t;
        asm volatile("" : "+v"(tt));
#pragma unroll
        for (uint32_t k = 0; k < vxb::kLightOwned; ++k) {
            const uint32_t r = tt + k * vxb::kLightThreads, ry = r % vxb::kLightSide, rz = r / vxb::kLightSide;
            uint64_t found = 0u;
            if (ry < size[1] && rz < size[2]) {
                const uint64_t around = vxb::light_spread(cur[r], ry > 0 ? cur[r - 1u] : 0u, ry + 1u < size[1] ? cur[r + 1u] : 0u, rz > 0 ? cur[r - vxb::kLightSide] : 0u,
                                                          rz + 1u < size[2] ? cur[r + vxb::kLightSide] : 0u);
                found = vxb::light_step(around, passable[k], SOURCES ? vxb::light_equal(v[k], level) : 0u, reached[k]);
            }
            next[r] = found;
            reached[k] |= found;
            vxb::light_set(v[k], found, level);
            any |= found | (SOURCES ? vxb::light_any(v[k]) & ~reached[k] : 0u);  // (a source of a lower level is still to come)
        }
        if (!__syncthreads_or(int(any != 0u))) break;  // (the same answer in every thread: all leave, or none)
    }
}

template <int SVO, bool FIELD>
__global__ __launch_bounds__(256) void light_boxes_kernel(SceneArgs sa, const uint8_t* __restrict__ lo, uint32_t lo_stride, uint32_t sx, uint32_t sy, uint32_t sz,
                                                          uint32_t flags, const uint32_t* __restrict__ props, uint8_t* __restrict__ fields, uint32_t field_stride,
                                                          vx_light_info* __restrict__ info) {
    __shared__ LightLds lds;
    const WorldBytes<SVO> w = {make_scene(sa)};
    const uint32_t n = blockIdx.x, t = threadIdx.x, lane = t & 63u, wave = uniform(t >> 6);
    const uint32_t size[3] = {sx, sy, sz};
    const bool sky_wanted = !(flags & VX_LIGHT_NO_SKY), block_wanted = !(flags & VX_LIGHT_NO_BLOCKS);

    // 1  the props and the box
#pragma unroll
    for (uint32_t k = 0; k < VX_LIGHT_MAX_PROPS / 4u / vxb::kLightThreads; ++k)
        reinterpret_cast<uint32_t*>(lds.props)[t + k * vxb::kLightThreads] = props[t + k * vxb::kLightThreads];
    int32_t at[3];
    {
        const int32_t* q = reinterpret_cast<const int32_t*>(lo + size_t(n) * lo_stride);
        at[0] = q[0]; at[1] = q[1]; at[2] = q[2];
    }
    vxb::LightBox box = vxb::light_box(at, size);
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        box.lo[a] = uniform(box.lo[a]);
        box.first[a] = uniform(box.first[a]);
        box.count[a] = uniform(box.count[a]);
    }
    box.top = int64_t(int32_t(box.lo[1])) + int64_t(sy);
    __syncthreads();

    // 2  loading
    uint64_t* const loaded = reinterpret_cast<uint64_t*>(lds.arena);  // [5][kLightRows]: passable, the planes
    const uint32_t i = lane & 7u, j = lane >> 3, brick_rows = box.count[1] * box.count[2];
#pragma nounroll
    for (uint32_t m = wave; m < brick_rows; m += vxb::kLightThreads / 64u) {  // (wave-uniform)
        const uint32_t cy = box.first[1] + (m % box.count[1]) * vxb::kBrick, cz = box.first[2] + (m / box.count[1]) * vxb::kBrick;
        vxb::LightRows rows = {0u, {0u, 0u, 0u, 0u}};
#pragma nounroll
        for (uint32_t bx = 0; bx < box.count[0]; ++bx) {
            const vxb::Brick b = vxb::enter_brick_at<kFormat<SVO>>(w, box.first[0] + bx * vxb::kBrick, cy, cz);
            vxb::light_brick_lane<kFormat<SVO>>(w, lds.props, VX_LIGHT_MAX_PROPS, box, b, i, j, rows);
        }
        const uint32_t ry = cy + i - box.lo[1], rz = cz + j - box.lo[2];
        if (ry < sy && rz < sz) {
            const uint32_t r = vxb::light_row_of(ry, rz);
            loaded[r] = rows.passable;
#pragma unroll
            for (uint32_t e = 0; e < 4; ++e) loaded[(1u + e) * vxb::kLightRows + r] = rows.emit[e];
        }
    }

    // 3  exposure above the box
    if (sky_wanted) {
#pragma nounroll
        for (uint32_t rz = wave; rz < sz; rz += kWaves) {  // (wave-uniform)
            uint32_t trips = 0u;
            const bool open = lane < sx && vxb::column_open<kFormat<SVO>>(w, lds.props, VX_LIGHT_MAX_PROPS, box.lo[0] + lane, box.lo[2] + rz, box.top, trips);
            const uint64_t word = __ballot(open);
            if (lane == 0) lds.open[rz] = word;
        }
    }
    __syncthreads();

    // 4  the owned rows
    uint64_t passable[vxb::kLightOwned], reached[vxb::kLightOwned];
    vxb::LightLevels sky[vxb::kLightOwned], block[vxb::kLightOwned];
    vxb::LightAcc acc = {0u, 0u, 0u, 0u};
#pragma unroll
    for (uint32_t k = 0; k < vxb::kLightOwned; ++k) {
        const uint32_t r = t + k * vxb::kLightThreads;
        const bool in = r % vxb::kLightSide < sy && r / vxb::kLightSide < sz;
        passable[k] = in ? loaded[r] : 0u;
#pragma unroll
        for (uint32_t e = 0; e < 4; ++e) {
            block[k].plane[e] = (in && block_wanted) ? loaded[(1u + e) * vxb::kLightRows + r] : 0u;
            sky[k].plane[e] = 0u;
        }
        reached[k] = 0u;
        acc.sources += vxb::popc64(vxb::light_any(block[k]));
    }
    __syncthreads();  // (the planes' part of LDS becomes the second frontier)
    uint64_t* const frontier0 = loaded;
    uint64_t* const frontier1 = loaded + vxb::kLightRows;

    if (sky_wanted) {
        // 5  exposure inside the box: the slab walk, in place
        if (t < sz) {
            uint64_t e = lds.open[t];
#pragma nounroll
            for (uint32_t ry = sy; ry-- > 0u;) {
                e &= frontier0[vxb::light_row_of(ry, t)];
                frontier0[vxb::light_row_of(ry, t)] = e;
            }
        }
        __syncthreads();
        // 6  the sky channel
#pragma unroll
        for (uint32_t k = 0; k < vxb::kLightOwned; ++k) {
            const uint32_t r = t + k * vxb::kLightThreads, ry = r % vxb::kLightSide;
            const bool in = ry < sy && r / vxb::kLightSide < sz;
            reached[k] = in ? frontier0[r] : 0u;
            if (!in) frontier0[r] = 0u;
            vxb::light_set(sky[k], reached[k], vxb::kLightTop);
            if (in && ry + 1u == sy) acc.open_columns += vxb::popc64(reached[k]);
        }
        __syncthreads();
        run_channel<false>(frontier0, frontier1, size, t, passable, reached, sky);
    }
    if (block_wanted) {
#pragma unroll
        for (uint32_t k = 0; k < vxb::kLightOwned; ++k) {
            reached[k] = vxb::light_equal(block[k], vxb::kLightTop);
            frontier0[t + k * vxb::kLightThreads] = reached[k];
        }
        __syncthreads();
        run_channel<true>(frontier0, frontier1, size, t, passable, reached, block);
    }

    // 8  the record
    if (info) {  // (a kernel argument: uniform)
#pragma unroll
        for (uint32_t k = 0; k < vxb::kLightOwned; ++k) {
            const uint32_t r = t + k * vxb::kLightThreads;
            vxb::light_fold_row(acc, size, r % vxb::kLightSide, r / vxb::kLightSide, sky[k], block[k]);
        }
        fold_put(lds.fold, wave, lane, acc, light_fold);
    }
    __syncthreads();  // (the fold's words; the last step's reads of the frontiers)
    if (info && t == 0) store_record(info + n, vxb::light_record(fold_take(lds.fold, light_fold)));

    // 7  the field: the owners' rows as bytes into LDS, a pass of kArena bytes at a time, out as 16-byte words
    if (FIELD) {
        const uint32_t voxels = vxb::light_voxels(size), padded = vxb::light_round16(voxels);
        uint8_t* const out = fields + size_t(n) * field_stride;
#pragma nounroll
        for (uint32_t base = 0; base < padded; base += kArena) {  // (uniform)
#pragma unroll
            for (uint32_t k = 0; k < vxb::kLightOwned; ++k) {
                const uint32_t r = t + k * vxb::kLightThreads, ry = r % vxb::kLightSide, rz = r / vxb::kLightSide;
                const uint32_t row = vxb::light_field_row(size, ry, rz);
                if (ry < sy && rz < sz && row + sx > base && row < base + kArena) {
                    vxb::LightLevels s = sky[k], b = block[k];
#pragma nounroll
                    for (uint32_t rx = 0; rx < sx; ++rx) {
                        const uint32_t idx = row + rx - base;  // (below the pass: a large number)
                        if (idx < kArena) lds.arena[idx] = vxb::light_byte(s, b, 0u);
#pragma unroll
                        for (uint32_t e = 0; e < 4; ++e) s.plane[e] >>= 1, b.plane[e] >>= 1;
                    }
                }
            }
            if (t < 16u && voxels + t < padded && voxels + t - base < kArena) lds.arena[voxels + t - base] = 0u;
            __syncthreads();
            const uint32_t chunks = ((padded - base < kArena ? padded - base : kArena)) / 16u;
            store_field(out + base, lds.arena, chunks, t, vxb::kLightThreads);
            __syncthreads();
        }
    }
}

}  // namespace

namespace vxk {

hipError_t launch_light_boxes(int svo, hipStream_t stream, const SceneArgs& sc, const void* lo, uint32_t lo_stride, uint32_t count, const uint32_t size[3],
                              uint32_t flags, const void* props, uint8_t* fields, uint32_t field_stride, vx_light_info* info) {
    static_assert(sizeof(vx_light_info) == 16, "one 16-byte store");
    if (count == 0 || count > vxb::kMaxCount || (!fields && !info) || !lo || !props) return hipErrorInvalidValue;
    // the kernel's own bounds, whatever the caller checked: rows and bytes of LDS are indexed by these
    if (!sizes_within(size, vxb::kLightSide)) return hipErrorInvalidValue;
    if ((flags & ~uint32_t(VX_LIGHT_NO_SKY | VX_LIGHT_NO_BLOCKS)) || flags == uint32_t(VX_LIGHT_NO_SKY | VX_LIGHT_NO_BLOCKS)) return hipErrorInvalidValue;
    if (lo_stride % 4u || lo_stride < 12u) return hipErrorInvalidValue;
    if (!field_stride_ok(fields, field_stride, vxb::light_voxels(size))) return hipErrorInvalidValue;
    const dim3 grid(count, 1, 1), block(vxb::kLightThreads);
    const uint8_t* p = static_cast<const uint8_t*>(lo);
    const uint32_t* table = static_cast<const uint32_t*>(props);
    return for_format(svo, [&](auto f) {
        constexpr int S = decltype(f)::value;
        if (fields) hipLaunchKernelGGL((light_boxes_kernel<S, true>), grid, block, 0, stream, sc, p, lo_stride, size[0], size[1], size[2], flags, table, fields, field_stride, info);
        else hipLaunchKernelGGL((light_boxes_kernel<S, false>), grid, block, 0, stream, sc, p, lo_stride, size[0], size[1], size[2], flags, table, fields, field_stride, info);
    });
}

}  // namespace vxk

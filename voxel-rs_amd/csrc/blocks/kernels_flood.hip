// vx_flood_points' kernel (gfx950): vx_flood.hpp's breadth-first flood for a batch of positions, the world's own bytes read as
// kernels_blocks.hip reads them (vx_world_bytes.hpp: a read beyond the world gives 0). The world is read-only for the launch. No global
// atomic, no LDS atomic but the one word __syncthreads_or reduces into; no workgroup waits for another; every loop bound is a kernel
// argument (max_steps <= 250 bounds the kernel's life).
//   a workgroup of 256 threads (4 waves) owns one query, blockIdx.x its number.
//   1  every thread reads the position at the same address (scalar loads in the code). No position (a NaN or infinite component): decided
//      here, before any barrier and for the whole workgroup alike -- the field goes out as VX_FLOOD_NO_POSITION, thread 0 writes the record.
//   2  the box and its bricks through readfirstlane: everything above a brick runs on scalar registers and wave-uniform addresses.
//   3  loading: the passable rows in LDS start as 0; wave v takes the brick rows v, v + 4, ... of the cover (all bricks along x of one
//      (brick y, brick z)), enters each brick once (enter_brick_at) and has lane l read the column along x at (y, z) = (l & 7, l >> 3)
//      (vxb::flood_brick_lane); after the last brick along x the lane stores its row: one lane holds a row, a plain store.
//   4  thread t owns rows t + 256 k, k = 0..3: (y, z) = (t & 31, (t >> 5) + 8 k). Their passable and reached bits live in REGISTERS from here
//      on (only the owner ever needs them); LDS keeps the two frontiers, which the neighbours read. With a field: the owner initialises its
//      rows' bytes from the passable bits, in vx_read_region's layout.
//   5  a step: vxb::flood_step for each owned row from the current frontier, the result into the other one; newly reached bits get the step
//      written into the byte field; one __syncthreads_or a step -- which every thread reaches -- says whether any thread found a cell.
//   6  the record: reached bits and faces folded by xor-shuffles in a wave, across the waves through 8 LDS words; the field as 16-byte stores.
//   FIELD == false (fields == NULL): the byte field is not declared, and the kernel uses 12 KiB of LDS.
// Registers (hipcc -Rpass-analysis=kernel-resource-usage, ESVO / CSVO / ESVO beyond 4 GiB): with a field 66 / 87 / 68 VGPRs, 89 / 104 / 91
// SGPRs; records only 59 / 87 / 68 and 82 / 97 / 84. No spill, no scratch in any of the six. LDS: 45,360 bytes with a field (three
// workgroups a CU under the 160 KiB), 12,608 bytes for records only; both include what __syncthreads_or keeps for itself.
// The device code below is deliberately the one from before kernels_shared.hpp (own folds, stores and loading loop; only uniform() and the
// launcher come from the header): on the header's folds, rows_around and stores 2 of the 96 rows of profiles/flood_bench.py
// ran 0.3 and 0.9 % slower (profiles/box_kernels/README.md), and the cause was not found in the generated code.
#include <hip/hip_runtime.h>

#include "kernels_blocks.h"
#include "kernels_shared.hpp"
#include "vx_device.hpp"
#include "vx_world_bytes.hpp"

using namespace vxd;
using vxk::kFormat;
using vxk::WorldBytes;
using vxk::uniform;

namespace {

constexpr uint32_t kFieldBytes = vxb::kFloodRows * vxb::kFloodSide;  // 32 KiB: a multiple of 16, so the rounded voxel count fits

template <bool FIELD>
struct FloodLds {
    uint32_t passable[vxb::kFloodRows];
    uint32_t frontier[2][vxb::kFloodRows];
    uint32_t fold[8];
    uint32_t seed_value;
    alignas(16) uint8_t field[FIELD ? kFieldBytes : 16];
};

template <int SVO, bool FIELD>
__global__ __launch_bounds__(256) void flood_points_kernel(SceneArgs sa, const uint8_t* __restrict__ pos, uint32_t pos_stride, vx_flood_shape s,
                                                           uint8_t* __restrict__ fields, uint32_t field_stride, vx_flood_info* __restrict__ info) {
    __shared__ FloodLds<FIELD> lds;
    const WorldBytes<SVO> w = {make_scene(sa)};
    const uint32_t n = blockIdx.x, t = threadIdx.x, lane = t & 63u, wave = uniform(t >> 6);
    const uint32_t voxels = vxb::flood_voxels(s), chunks = vxb::flood_round16(voxels) / 16u;
    float p[3];
    {
        const float* q = reinterpret_cast<const float*>(pos + size_t(n) * pos_stride);
        p[0] = q[0]; p[1] = q[1]; p[2] = q[2];
    }
    uint4* const out = FIELD ? reinterpret_cast<uint4*>(fields + size_t(n) * field_stride) : nullptr;
    if (!vxb::flood_has_position(p)) {  // (the same for every thread of the workgroup; no barrier has been met)
        if (FIELD)
            for (uint32_t c = t; c < chunks; c += vxb::kFloodThreads)
                out[c] = make_uint4(vxb::flood_no_position_word(4u * c, voxels), vxb::flood_no_position_word(4u * c + 1u, voxels),
                                    vxb::flood_no_position_word(4u * c + 2u, voxels), vxb::flood_no_position_word(4u * c + 3u, voxels));
        if (info && t == 0) *reinterpret_cast<uint4*>(info + n) = make_uint4(VX_FLOOD_INVALID, 0u, 0u, 0u);
        return;
    }
    vxb::FloodBox box = vxb::flood_box(p, s);
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        box.lo[a] = uniform(box.lo[a]);
        box.first[a] = uniform(box.first[a]);
        box.count[a] = uniform(box.count[a]);
    }

    // 3  loading
#pragma unroll
    for (uint32_t k = 0; k < vxb::kFloodOwned; ++k) lds.passable[t + k * vxb::kFloodThreads] = 0u;
    __syncthreads();
    const uint32_t i = lane & 7u, j = lane >> 3, brick_rows = box.count[1] * box.count[2];
#pragma nounroll
    for (uint32_t m = wave; m < brick_rows; m += vxb::kFloodThreads / 64u) {  // (wave-uniform)
        const uint32_t cy = box.first[1] + (m % box.count[1]) * vxb::kBrick, cz = box.first[2] + (m / box.count[1]) * vxb::kBrick;
        uint32_t row = 0u, seed_value = 0u;
#pragma nounroll
        for (uint32_t bx = 0; bx < box.count[0]; ++bx) {
            const vxb::Brick b = vxb::enter_brick_at<kFormat<SVO>>(w, box.first[0] + bx * vxb::kBrick, cy, cz);
            vxb::flood_brick_lane<kFormat<SVO>>(w, s, box, b, i, j, row, seed_value);
        }
        const uint32_t ry = cy + i - box.lo[1], rz = cz + j - box.lo[2];
        if (ry < s.size[1] && rz < s.size[2]) {
            lds.passable[vxb::flood_row_of(ry, rz)] = row;
            if (ry == s.seed_at[1] && rz == s.seed_at[2]) lds.seed_value = seed_value;  // (the one lane that met the seed's cell)
        }
    }
    __syncthreads();

    // 4  the owned rows
    const uint32_t ry = t & (vxb::kFloodSide - 1u), rz0 = t >> 5;
    const uint32_t seed_row = vxb::flood_seed_row(s), seed_bit = 1u << s.seed_at[0];
    uint32_t passable[vxb::kFloodOwned], reached[vxb::kFloodOwned];
#pragma unroll
    for (uint32_t k = 0; k < vxb::kFloodOwned; ++k) {
        const uint32_t r = t + k * vxb::kFloodThreads, rz = rz0 + 8u * k;
        passable[k] = lds.passable[r];
        if (r == seed_row && (s.flags & VX_FLOOD_SEED_ALWAYS)) passable[k] |= seed_bit;
        reached[k] = r == seed_row ? passable[k] & seed_bit : 0u;
        lds.frontier[0][r] = reached[k];
        if (FIELD && ry < s.size[1] && rz < s.size[2]) {
            const uint32_t at = vxb::flood_field_row(s, ry, rz);
            for (uint32_t rx = 0; rx < s.size[0]; ++rx) lds.field[at + rx] = ((passable[k] >> rx) & 1u) ? uint8_t(VX_FLOOD_UNREACHED) : uint8_t(VX_FLOOD_BLOCKED);
            if (reached[k]) lds.field[at + s.seed_at[0]] = 0;
        }
    }
    if (FIELD && t < 16u && voxels + t < chunks * 16u) lds.field[voxels + t] = uint8_t(VX_FLOOD_BLOCKED);
    __syncthreads();

    // 5  the steps
    uint32_t farthest = 0u;
#pragma nounroll
    for (uint32_t step = 1; step <= s.max_steps; ++step) {
        const uint32_t* const cur = lds.frontier[(step - 1u) & 1u];
        uint32_t* const next = lds.frontier[step & 1u];
        uint32_t any = 0u;
#pragma unroll
        for (uint32_t k = 0; k < vxb::kFloodOwned; ++k) {
            const uint32_t r = t + k * vxb::kFloodThreads, rz = rz0 + 8u * k;
            uint32_t found = 0u;
            if (ry < s.size[1] && rz < s.size[2])
                found = vxb::flood_step(cur[r], ry > 0 ? cur[r - 1u] : 0u, ry + 1u < s.size[1] ? cur[r + 1u] : 0u, rz > 0 ? cur[r - vxb::kFloodSide] : 0u,
                                        rz + 1u < s.size[2] ? cur[r + vxb::kFloodSide] : 0u, passable[k], reached[k]);
            next[r] = found;
            reached[k] |= found;
            any |= found;
            if (FIELD && found) {
                const uint32_t at = vxb::flood_field_row(s, ry, rz);
                for (uint32_t m = found; m; m &= m - 1u) lds.field[at + uint32_t(__builtin_ctz(m))] = uint8_t(step);
            }
        }
        if (!__syncthreads_or(int(any))) break;  // (the same answer in every thread: all leave, or none)
        farthest = step;
    }

    // 6  the record and the field
    if (info) {  // (a kernel argument: uniform)
        vxb::FloodAcc acc = {0u, 0u};
#pragma unroll
        for (uint32_t k = 0; k < vxb::kFloodOwned; ++k) vxb::flood_fold_row(acc, s, ry, rz0 + 8u * k, reached[k]);
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            acc.reached += uint32_t(__shfl_xor(int(acc.reached), d, 64));
            acc.faces |= uint32_t(__shfl_xor(int(acc.faces), d, 64));
        }
        if (lane == 0) lds.fold[wave] = acc.reached, lds.fold[4u + wave] = acc.faces;
    }
    __syncthreads();  // (the fold's words; the last step's bytes of the field)
    if (info && t == 0) {
        vxb::FloodAcc all = {lds.fold[0] + lds.fold[1] + lds.fold[2] + lds.fold[3], lds.fold[4] | lds.fold[5] | lds.fold[6] | lds.fold[7]};
        const vx_flood_info r = vxb::flood_record(all, farthest, lds.seed_value);
        *reinterpret_cast<uint4*>(info + n) = make_uint4(r.reached, r.farthest, r.faces, r.seed_value);
    }
    if (FIELD) {
        const uint4* const from = reinterpret_cast<const uint4*>(lds.field);
        for (uint32_t c = t; c < chunks; c += vxb::kFloodThreads) out[c] = from[c];
    }
}

}  // namespace

namespace vxk {

hipError_t launch_flood_points(int svo, hipStream_t stream, const SceneArgs& sc, const void* pos, uint32_t pos_stride, uint32_t count, const vx_flood_shape& shape,
                               uint8_t* fields, uint32_t field_stride, vx_flood_info* info) {
    static_assert(sizeof(vx_flood_info) == 16, "one 16-byte store");
    if (count == 0 || count > vxb::kMaxCount || (!fields && !info)) return hipErrorInvalidValue;
    // the kernel's own bounds, whatever the caller checked: rows and bytes of LDS are indexed by these
    if (!sizes_within(shape.size, vxb::kFloodSide)) return hipErrorInvalidValue;
    if (shape.seed_at[0] >= shape.size[0] || shape.seed_at[1] >= shape.size[1] || shape.seed_at[2] >= shape.size[2]) return hipErrorInvalidValue;
    if (shape.max_steps > VX_FLOOD_MAX_STEPS) return hipErrorInvalidValue;
    if (!field_stride_ok(fields, field_stride, vxb::flood_voxels(shape))) return hipErrorInvalidValue;
    const dim3 grid(count, 1, 1), block(vxb::kFloodThreads);
    const uint8_t* p = static_cast<const uint8_t*>(pos);
    return for_format(svo, [&](auto f) {
        constexpr int S = decltype(f)::value;
        if (fields) hipLaunchKernelGGL((flood_points_kernel<S, true>), grid, block, 0, stream, sc, p, pos_stride, shape, fields, field_stride, info);
        else hipLaunchKernelGGL((flood_points_kernel<S, false>), grid, block, 0, stream, sc, p, pos_stride, shape, fields, field_stride, info);
    });
}

}  // namespace vxk

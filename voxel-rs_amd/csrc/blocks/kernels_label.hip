// vx_label_boxes' kernel (gfx950): vx_label.hpp's floods of the solid cells for a batch of boxes, the world's own bytes read as
// kernels_blocks.hip reads them (vx_world_bytes.hpp: a read beyond the world gives 0). The world is read-only for the launch. No global
// atomic, no LDS atomic but the one word __syncthreads_or reduces into; no workgroup waits for another. Every decision a barrier depends on
// is the same in every thread of the workgroup: "the flood ended" is __syncthreads_or's answer, "the budget is spent" is arithmetic on that
// answer and on kernel arguments, "no seed is left" is the minimum of four LDS words that every thread reads behind a barrier. The only loop
// bounds are max_steps (<= 4,096), max_pieces (<= 250) and the brick counts (<= 5 an axis): all kernel arguments, which the launcher checks
// again whatever the caller checked; a query takes at most max_steps + max_pieces + 1 steps.
//   a workgroup of 256 threads (4 waves) owns one box, blockIdx.x its number.
//   1  every thread reads lo at the same address (scalar loads in the code); the box and its bricks through readfirstlane: everything above
//      a brick runs on scalar registers and wave-uniform addresses.
//   2  loading, as kernels_flood.hip loads: wave v takes the brick rows v, v + 4, ... of the cover, enters each brick once (enter_brick_at)
//      and has lane l read the column along x at (y, z) = (l & 7, l >> 3) (vxb::flood_brick_lane); after the last brick along x the lane
//      stores its row into the frontier that is not used yet: one lane holds a row, a plain store.
//   3  thread t owns rows t + 256 k, k = 0..3: (y, z) = (t & 31, (t >> 5) + 8 k). Their solid, settled and piece bits live in REGISTERS from
//      here on (only the owner ever needs them); LDS keeps the two frontiers, which the neighbours read. With a field: the owner initialises
//      its rows' bytes, VX_LABEL_MORE for a solid cell, VX_LABEL_AIR for the others.
//   4  the held flood from the solid cells on the anchor faces: vxb::label_flood over a step that is vxb::label_step for each owned row from
//      the current frontier into the other one and ONE __syncthreads_or, which every thread reaches. Its cells' bytes become VX_LABEL_HELD.
//   5  the pieces: each thread's first unsettled key (vxb::label_seed_key) folded to the workgroup's minimum by xor-shuffles in a wave and
//      four LDS words; the owner of the seed's row puts the bit into the frontier written last, which is empty; the flood; when it is
//      complete the owners write the label into their rows' bytes from the piece bits -- behind the flood, not a step at a time: a cut flood
//      has nothing to take back -- and the piece's fold goes across the waves through LDS, thread 0 stores the 16-byte record.
//   6  what is still VX_LABEL_MORE stays; the unused piece records are zeroed by the workgroup, the record leaves as two 16-byte stores, the
//      field as 16-byte stores from LDS.
//   FIELD == false (fields == NULL): the byte field is not declared, and the kernel uses 8 KiB of LDS and a few words.
// Registers (hipcc -Rpass-analysis=kernel-resource-usage, ESVO / CSVO / ESVO beyond 4 GiB): with a field 82 / 85 / 82 VGPRs, 79 / 90 / 79
// SGPRs; records only 72 / 85 / 72 and 76 / 90 / 77. No spill, no scratch in any of the six. LDS: 41,392 bytes with a field (three
// workgroups a CU under the 160 KiB, as kernels_flood.hip), 8,640 bytes for records only; both include what __syncthreads_or keeps for
// itself.
// The device code below is deliberately the one from before kernels_shared.hpp (own folds, stores and loading loop; only uniform() and the
// launcher come from the header): on the header's folds, rows_around and stores 10 of the 36 rows of profiles/label_bench.py
// ran 0.4 to 1.1 % slower (profiles/box_kernels/README.md), and the cause was not found in the generated code.
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
constexpr uint32_t kWaves = vxb::kFloodThreads / 64u;

template <bool FIELD>
struct LabelLds {
    uint32_t frontier[2][vxb::kFloodRows];
    uint32_t key[kWaves];
    vxb::LabelAcc fold[kWaves];
    uint32_t sums[kWaves][3];
    alignas(16) uint8_t field[FIELD ? kFieldBytes : 16];
};

// a fold's words across the lanes of a wave: every lane ends with the wave's
__device__ __forceinline__ void fold_wave(vxb::LabelAcc& a) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        vxb::LabelAcc b;
        b.cells = uint32_t(__shfl_xor(int(a.cells), d, 64));
        b.xbits = uint32_t(__shfl_xor(int(a.xbits), d, 64));
        b.ylo = uint32_t(__shfl_xor(int(a.ylo), d, 64));
        b.yhi = uint32_t(__shfl_xor(int(a.yhi), d, 64));
        b.zlo = uint32_t(__shfl_xor(int(a.zlo), d, 64));
        b.zhi = uint32_t(__shfl_xor(int(a.zhi), d, 64));
        b.faces = uint32_t(__shfl_xor(int(a.faces), d, 64));
        vxb::label_fold(a, b);
    }
}

template <int SVO, bool FIELD>
__global__ __launch_bounds__(256) void label_boxes_kernel(SceneArgs sa, const uint8_t* __restrict__ lo, uint32_t lo_stride, vx_label_shape s,
                                                          uint8_t* __restrict__ fields, uint32_t field_stride, vx_label_piece* __restrict__ pieces,
                                                          vx_label_info* __restrict__ info) {
    __shared__ LabelLds<FIELD> lds;
    const WorldBytes<SVO> w = {make_scene(sa)};
    const uint32_t n = blockIdx.x, t = threadIdx.x, lane = t & 63u, wave = uniform(t >> 6);
    const uint32_t voxels = vxb::label_voxels(s), chunks = vxb::flood_round16(voxels) / 16u;
    const vx_flood_shape load = vxb::label_load_shape(s);

    // 1  the box
    int32_t at[3];
    {
        const int32_t* q = reinterpret_cast<const int32_t*>(lo + size_t(n) * lo_stride);
        at[0] = q[0]; at[1] = q[1]; at[2] = q[2];
    }
    vxb::FloodBox box = vxb::label_box(at, s);
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        box.lo[a] = uniform(box.lo[a]);
        box.first[a] = uniform(box.first[a]);
        box.count[a] = uniform(box.count[a]);
    }

    // 2  loading: the passable rows into frontier[1] (every row of the box is some lane's; the others are never read)
    {
        const uint32_t i = lane & 7u, j = lane >> 3, brick_rows = box.count[1] * box.count[2];
#pragma nounroll
        for (uint32_t m = wave; m < brick_rows; m += kWaves) {  // (wave-uniform)
            const uint32_t cy = box.first[1] + (m % box.count[1]) * vxb::kBrick, cz = box.first[2] + (m / box.count[1]) * vxb::kBrick;
            uint32_t row = 0u, unused = 0u;
#pragma nounroll
            for (uint32_t bx = 0; bx < box.count[0]; ++bx) {
                const vxb::Brick b = vxb::enter_brick_at<kFormat<SVO>>(w, box.first[0] + bx * vxb::kBrick, cy, cz);
                vxb::flood_brick_lane<kFormat<SVO>>(w, load, box, b, i, j, row, unused);
            }
            const uint32_t ry = cy + i - box.lo[1], rz = cz + j - box.lo[2];
            if (ry < s.size[1] && rz < s.size[2]) lds.frontier[1][vxb::flood_row_of(ry, rz)] = row;
        }
    }
    __syncthreads();

    // 3  the owned rows; the held flood's seeds into frontier[0]
    const uint32_t ry = t & (vxb::kFloodSide - 1u), rz0 = t >> 5;
    uint32_t solid[vxb::kFloodOwned], settled[vxb::kFloodOwned], piece[vxb::kFloodOwned];
#pragma unroll
    for (uint32_t k = 0; k < vxb::kFloodOwned; ++k) {
        const uint32_t r = t + k * vxb::kFloodThreads, rz = rz0 + 8u * k;
        const bool in_box = ry < s.size[1] && rz < s.size[2];
        solid[k] = in_box ? vxb::label_solid_row(lds.frontier[1][r], s.size[0]) : 0u;
        settled[k] = 0u;
        piece[k] = in_box ? solid[k] & vxb::label_anchor_row(s, ry, rz) : 0u;
        lds.frontier[0][r] = piece[k];
        if (FIELD && in_box) {
            const uint32_t at_row = vxb::flood_field_row(load, ry, rz);
            for (uint32_t rx = 0; rx < s.size[0]; ++rx) lds.field[at_row + rx] = ((solid[k] >> rx) & 1u) ? uint8_t(VX_LABEL_MORE) : uint8_t(VX_LABEL_AIR);
        }
    }
    if (FIELD && t < 16u && voxels + t < chunks * 16u) lds.field[voxels + t] = uint8_t(VX_LABEL_AIR);
    __syncthreads();

    // the bytes of the owned rows' cells `piece`
    const auto write = [&](uint32_t byte) {
        if (!FIELD) return;
#pragma unroll
        for (uint32_t k = 0; k < vxb::kFloodOwned; ++k) {
            if (!piece[k]) continue;
            const uint32_t at_row = vxb::flood_field_row(load, ry, rz0 + 8u * k);
            for (uint32_t m = piece[k]; m; m &= m - 1u) lds.field[at_row + uint32_t(__builtin_ctz(m))] = uint8_t(byte);
        }
    };
    // a step of the running flood: frontier[phase] -> frontier[phase ^ 1]; the same answer in every thread
    uint32_t phase = 0u;
    const auto step = [&](bool keep) {
        const uint32_t* const cur = lds.frontier[phase];
        uint32_t* const next = lds.frontier[phase ^ 1u];
        uint32_t any = 0u;
#pragma unroll
        for (uint32_t k = 0; k < vxb::kFloodOwned; ++k) {
            const uint32_t r = t + k * vxb::kFloodThreads, rz = rz0 + 8u * k;
            uint32_t found = 0u;
            if (ry < s.size[1] && rz < s.size[2])
                found = vxb::label_step(cur[r], ry > 0 ? cur[r - 1u] : 0u, ry + 1u < s.size[1] ? cur[r + 1u] : 0u, rz > 0 ? cur[r - vxb::kFloodSide] : 0u,
                                        rz + 1u < s.size[2] ? cur[r + vxb::kFloodSide] : 0u, solid[k], settled[k], piece[k]);
            next[r] = found;
            if (keep) piece[k] |= found;
            any |= found;
        }
        phase ^= 1u;
        return __syncthreads_or(int(any)) != 0;  // (every thread reaches it: all go on, or none)
    };

    // 4  held
    vxb::LabelBudget budget = {0u, s.max_steps, 0u};
    bool going = vxb::label_flood(budget, step);
    write(VX_LABEL_HELD);
    uint32_t held = 0u;
#pragma unroll
    for (uint32_t k = 0; k < vxb::kFloodOwned; ++k) {
        held += vxb::popc(piece[k]);
        settled[k] = piece[k];
        piece[k] = 0u;
    }

    // 5  the pieces (going, count and the keys: the same in every thread)
    uint32_t count = 0u, loose = 0u;
#pragma nounroll
    while (going && count < s.max_pieces) {
        uint32_t key = vxb::kLabelNoSeed;
#pragma unroll
        for (uint32_t k = 0; k < vxb::kFloodOwned; ++k) key = min(key, vxb::label_seed_key(t + k * vxb::kFloodThreads, solid[k], settled[k]));
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) key = min(key, uint32_t(__shfl_xor(int(key), d, 64)));
        if (lane == 0) lds.key[wave] = key;
        __syncthreads();
        key = min(min(lds.key[0], lds.key[1]), min(lds.key[2], lds.key[3]));
        if (key == vxb::kLabelNoSeed) break;
#pragma unroll
        for (uint32_t k = 0; k < vxb::kFloodOwned; ++k)
            if (t + k * vxb::kFloodThreads == vxb::label_key_row(key)) {
                piece[k] = vxb::label_key_bit(key);
                lds.frontier[phase][t + k * vxb::kFloodThreads] = piece[k];  // (the frontier written last: empty)
            }
        __syncthreads();
        going = vxb::label_flood(budget, step);
        if (going) {
            write(count + 1u);
            vxb::LabelAcc acc = vxb::label_acc();
#pragma unroll
            for (uint32_t k = 0; k < vxb::kFloodOwned; ++k) {
                vxb::label_fold_row(acc, s, ry, rz0 + 8u * k, piece[k]);
                settled[k] |= piece[k];
            }
            fold_wave(acc);
            if (lane == 0) lds.fold[wave] = acc;
        }
#pragma unroll
        for (uint32_t k = 0; k < vxb::kFloodOwned; ++k) piece[k] = 0u;
        if (!going) break;
        __syncthreads();  // (the fold's words; the next piece's steps lie between this read and the next write of them)
        if (t == 0) {
            vxb::LabelAcc all = lds.fold[0];
            for (uint32_t v = 1; v < kWaves; ++v) vxb::label_fold(all, lds.fold[v]);
            loose += all.cells;
            if (pieces) {
                const vx_label_piece p = vxb::label_piece(all, key);
                *reinterpret_cast<uint4*>(pieces + size_t(n) * s.max_pieces + count) = make_uint4(p.cells, p.lo, p.hi, p.where);
            }
        }
        ++count;
    }

    // 6  the unused piece records, the record, the field
    if (pieces)
        for (uint32_t k = count + t; k < s.max_pieces; k += vxb::kFloodThreads) *reinterpret_cast<uint4*>(pieces + size_t(n) * s.max_pieces + k) = make_uint4(0u, 0u, 0u, 0u);
    __syncthreads();  // (the last label's bytes of the field)
    if (info) {  // (a kernel argument: uniform)
        uint32_t cells = 0u, faces = 0u;
#pragma unroll
        for (uint32_t k = 0; k < vxb::kFloodOwned; ++k) cells += vxb::popc(solid[k]), faces |= vxb::label_faces(s, ry, rz0 + 8u * k, solid[k]);
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            cells += uint32_t(__shfl_xor(int(cells), d, 64));
            held += uint32_t(__shfl_xor(int(held), d, 64));
            faces |= uint32_t(__shfl_xor(int(faces), d, 64));
        }
        if (lane == 0) lds.sums[wave][0] = cells, lds.sums[wave][1] = held, lds.sums[wave][2] = faces;
        __syncthreads();
        if (t == 0) {
            cells = held = faces = 0u;
            for (uint32_t v = 0; v < kWaves; ++v) cells += lds.sums[v][0], held += lds.sums[v][1], faces |= lds.sums[v][2];
            const vx_label_info r = vxb::label_record(cells, held, count, loose, faces, budget);
            uint4* const to = reinterpret_cast<uint4*>(info + n);
            to[0] = make_uint4(r.solid, r.held, r.pieces, r.loose);
            to[1] = make_uint4(r.more, r.steps, r.faces, r.flags);
        }
    }
    if (FIELD) {
        uint4* const out = reinterpret_cast<uint4*>(fields + size_t(n) * field_stride);
        const uint4* const from = reinterpret_cast<const uint4*>(lds.field);
        for (uint32_t c = t; c < chunks; c += vxb::kFloodThreads) out[c] = from[c];
    }
}

}  // namespace

namespace vxk {

hipError_t launch_label_boxes(int svo, hipStream_t stream, const SceneArgs& sc, const void* lo, uint32_t lo_stride, uint32_t count, const vx_label_shape& shape,
                              uint8_t* fields, uint32_t field_stride, vx_label_piece* pieces, vx_label_info* info) {
    static_assert(sizeof(vx_label_piece) == 16 && sizeof(vx_label_info) == 32, "16-byte stores");
    if (count == 0 || count > vxb::kLabelMaxCount || (!fields && !pieces && !info) || !lo) return hipErrorInvalidValue;
    // the kernel's own bounds, whatever the caller checked: rows and bytes of LDS are indexed by these, and its loops end by them
    if (!sizes_within(shape.size, vxb::kFloodSide)) return hipErrorInvalidValue;
    if (shape.max_steps > VX_LABEL_MAX_STEPS || shape.max_pieces > VX_LABEL_MAX_PIECES || (shape.anchor_faces & ~uint32_t(VX_LABEL_ALL_FACES)) || shape.flags)
        return hipErrorInvalidValue;
    if (pieces && shape.max_pieces == 0) return hipErrorInvalidValue;
    if (!field_stride_ok(fields, field_stride, vxb::label_voxels(shape))) return hipErrorInvalidValue;
    const dim3 grid(count, 1, 1), block(vxb::kFloodThreads);
    const uint8_t* p = static_cast<const uint8_t*>(lo);
    return for_format(svo, [&](auto f) {
        constexpr int S = decltype(f)::value;
        if (fields) hipLaunchKernelGGL((label_boxes_kernel<S, true>), grid, block, 0, stream, sc, p, lo_stride, shape, fields, field_stride, pieces, info);
        else hipLaunchKernelGGL((label_boxes_kernel<S, false>), grid, block, 0, stream, sc, p, lo_stride, shape, fields, field_stride, pieces, info);
    });
}

}  // namespace vxk

// vx_walk_points' kernel (gfx950): vx_walk.hpp's walking graph searched breadth first for a batch of positions, and the path to a goal traced
// back, over the world's own bytes read as kernels_flood.hip reads them (vx_world_bytes.hpp: a read beyond the world gives 0). The world is
// read-only for the launch. No global atomic, no LDS atomic but the one word __syncthreads_or reduces into; no workgroup waits for another;
// every loop bound is a kernel argument or a constant (max_steps <= 250 bounds the steps and the back-trace's trips).
//   a workgroup of 256 threads (4 waves) owns one query, blockIdx.x its number.
//   1  every thread reads the position at the same address. No position: decided here, before any barrier and for the whole
//      workgroup alike -- the field goes out as VX_WALK_NO_POSITION, the path as VX_WALK_NONE, thread 0 writes the record.
//   2  the box of the extended layers (vxb::walk_load_shape) and its bricks through readfirstlane.
//   3  loading: kernels_flood.hip's, over size.y + height layers: wave v takes the brick rows v, v + 4, ... of the cover, lane l the column
//      along x at (y, z) = (l & 7, l >> 3); one lane holds a row, a plain store. (Why each box kernel writes this loop out: kernels_shared.hpp.)
//   4  settling: every thread reads the goal (and the position again) at the same addresses; thread 0 walks the seed's column down, thread
//      64 the goal's (vxb::walk_settle: at most 36 LDS reads); two words of LDS.
//   5  thread t owns rows t + 256 k, k = 0..3: (layer, z) = (t & 31, (t >> 5) + 8 k). Its rows' standable and reached bits, the up mask and
//      the three "clear above me for a drop of d" masks live in REGISTERS (vxb::walk_row, from the passable rows of its column); LDS keeps the
//      passable rows (the back-trace reads them), two frontiers and, per parity, the cells of the frontier that may step up -- written by
//      the owner, so a neighbour reads one word per edge kind. With a field: the owner initialises its rows' bytes.
//   6  a step: vxb::walk_step for each owned row -- level, from below, from above by d = 1..drop --, the result and its up part into the
//      other parity; newly reached bits get the step written into the byte field; the owner of the goal's row notes the step that finds it;
//      one __syncthreads_or a step, which every thread reaches. Under VX_WALK_STOP_AT_GOAL all threads compare that word with the step just
//      done (a thread already in the next step can only write a LARGER step into it: the comparison cannot tear the workgroup apart).
//   7  the record: folded across the workgroup (fold_put, fold_take: 8 LDS words); two 16-byte stores by thread 0 (store_record).
//   8  the path: wave 0 walks back from the goal, lane c the candidate c of vxb::walk_candidate (at most 4 x (2 + drop) = 20 lanes), a ballot
//      picks the first, a readlane hands it on; at most path_steps <= max_steps trips; entries into LDS, and after a barrier out as 16-byte
//      stores. The field leaves as 16-byte stores (store_field). The step's reads of the frontier stay vxb::walk_beside's (vx_walk.hpp, which
//      the host harness shares): its rows beside a row are other layers of the column.
//   FIELD == false (no fields and no path): the byte field is not declared.
// Registers (hipcc -Rpass-analysis=kernel-resource-usage, ESVO / CSVO / ESVO beyond 4 GiB): with a field 66 / 88 / 68 VGPRs, 99 / 106 / 101
// SGPRs; records only 67 / 88 / 70 and 91 / 106 / 93. No scratch in any of the six and no VGPR spill. The target of no spill at all is missed
// by one build: CSVO with a field keeps 2 SGPRs in lanes of a VGPR (v_writelane, no memory) -- its descent to a brick, two to three dependent
// loads a level, holds more scalar state beside the 13 words of the shape and five pointers than 102 SGPRs take. LDS: 53,536 bytes with a
// field (three workgroups a CU under the 160 KiB; the flood's 45,360 and 8 KiB for the second frontiers), 20,816 bytes for records only;
// both include what __syncthreads_or keeps for itself.
#include <hip/hip_runtime.h>

#include "kernels_blocks.h"
#include "kernels_shared.hpp"
#include "vx_device.hpp"
#include "vx_world_bytes.hpp"

using namespace vxd;
using namespace vxk;

namespace {

constexpr uint32_t kWaves = vxb::kFloodThreads / 64u;

template <bool FIELD>
struct WalkLds {
    uint32_t passable[vxb::kFloodRows];
    uint32_t frontier[2][vxb::kFloodRows];
    uint32_t up[2][vxb::kFloodRows];
    vxb::FloodAcc fold[kWaves];
    uint32_t seed_value, start_e, goal_e, goal_step;
    alignas(16) uint32_t path[FIELD ? vxb::kWalkMaxPath : 4];
    alignas(16) uint8_t field[FIELD ? vxb::kWalkFieldBytes : 16];
};

__device__ __forceinline__ void walk_fold(vxb::FloodAcc& a, const vxb::FloodAcc& b) { a.reached += b.reached, a.faces |= b.faces; }

// where a query's outputs go
struct WalkOutputs {
    uint32_t voxels, chunks, path_chunks;
    uint8_t* out;
    uint4* path_out;
};

template <int SVO, bool FIELD>
__global__ __launch_bounds__(256) void walk_points_kernel(SceneArgs sa, const uint8_t* __restrict__ pos, uint32_t pos_stride, const uint8_t* __restrict__ goals,
                                                          uint32_t goal_stride, vx_walk_shape s, uint8_t* __restrict__ fields, uint32_t field_stride,
                                                          uint32_t* __restrict__ paths, vx_walk_info* __restrict__ info) {
    __shared__ WalkLds<FIELD> lds;
    const WorldBytes<SVO> w = {make_scene(sa)};
    const uint32_t n = blockIdx.x, t = threadIdx.x, lane = t & 63u, wave = uniform(t >> 6);
    float p[3];
    load3_at(pos, size_t(n) * pos_stride, p);
    // (where the outputs go is worked out where they are written, here and at the end: nothing of it is kept across the loading)
    const auto outputs = [&] {
        const uint32_t voxels = vxb::walk_voxels(s);
        return WalkOutputs{voxels, vxb::flood_round16(voxels) / 16u, s.path_capacity / 4u, FIELD && fields ? fields + size_t(n) * field_stride : nullptr,
                           FIELD && paths ? reinterpret_cast<uint4*>(paths + size_t(n) * s.path_capacity) : nullptr};
    };
    if (!vxb::flood_has_position(p)) {  // (the same for every thread of the workgroup; no barrier has been met)
        const WalkOutputs o = outputs();
        if (o.out)
            for (uint32_t c = t; c < o.chunks; c += vxb::kFloodThreads)
                reinterpret_cast<uint4*>(o.out)[c] = make_uint4(vxb::flood_no_position_word(4u * c, o.voxels), vxb::flood_no_position_word(4u * c + 1u, o.voxels),
                                                                vxb::flood_no_position_word(4u * c + 2u, o.voxels), vxb::flood_no_position_word(4u * c + 3u, o.voxels));
        if (o.path_out && t < o.path_chunks) o.path_out[t] = make_uint4(VX_WALK_NONE, VX_WALK_NONE, VX_WALK_NONE, VX_WALK_NONE);
        if (info && t == 0) store_record(info + n, vxb::walk_no_position());
        return;
    }
    const vx_flood_shape ls = vxb::walk_load_shape(s);
    vxb::FloodBox box = vxb::flood_box(p, ls);
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        box.lo[a] = uniform(box.lo[a]);
        box.first[a] = uniform(box.first[a]);
        box.count[a] = uniform(box.count[a]);
    }

    // 3  loading
#pragma unroll
    for (uint32_t k = 0; k < vxb::kFloodOwned; ++k) {
        const uint32_t r = t + k * vxb::kFloodThreads;
        lds.passable[r] = 0u;
        lds.frontier[0][r] = lds.frontier[1][r] = lds.up[0][r] = lds.up[1][r] = 0u;
    }
    if (FIELD && t < vxb::kWalkMaxPath) lds.path[t] = VX_WALK_NONE;
    __syncthreads();
    const uint32_t i = lane & 7u, j = lane >> 3, brick_rows = box.count[1] * box.count[2];
#pragma nounroll
    for (uint32_t m = wave; m < brick_rows; m += kWaves) {  // (wave-uniform)
        const uint32_t cy = box.first[1] + (m % box.count[1]) * vxb::kBrick, cz = box.first[2] + (m / box.count[1]) * vxb::kBrick;
        uint32_t row = 0u, seed_value = 0u;
#pragma nounroll
        for (uint32_t bx = 0; bx < box.count[0]; ++bx) {
            const vxb::Brick b = vxb::enter_brick_at<kFormat<SVO>>(w, box.first[0] + bx * vxb::kBrick, cy, cz);
            vxb::flood_brick_lane<kFormat<SVO>>(w, ls, box, b, i, j, row, seed_value);
        }
        const uint32_t e = cy + i - box.lo[1], rz = cz + j - box.lo[2];
        if (e < ls.size[1] && rz < ls.size[2]) {
            lds.passable[vxb::flood_row_of(e, rz)] = row;
            if (e == ls.seed_at[1] && rz == ls.seed_at[2]) lds.seed_value = seed_value;  // (the one lane that met the seed's cell)
        }
    }
    __syncthreads();

    // 4  settling (the goal is read here, and the position again: nothing of them is kept across the loading)
    vxb::WalkCell goal = {0u, 0u, 0u, false};
    if (goals) {  // (a kernel argument: uniform)
        float at[3], g[3];
        load3_at(pos, size_t(n) * pos_stride, at);
        load3_at(goals, size_t(n) * goal_stride, g);
        if (vxb::flood_has_position(g)) goal = vxb::walk_goal_cell(at, g, s);
    }
    goal.rx = uniform(goal.rx), goal.ry = uniform(goal.ry), goal.rz = uniform(goal.rz);
    const bool goal_in = uniform(goal.in ? 1u : 0u) != 0u;
    if (t == 0) lds.start_e = vxb::walk_settle(lds.passable + s.seed_at[2] * vxb::kFloodSide, 1u << s.seed_at[0], s.seed_at[1] + 1u, s);
    if (t == 64u) lds.goal_e = goal_in ? vxb::walk_settle(lds.passable + goal.rz * vxb::kFloodSide, 1u << goal.rx, goal.ry + 1u, s) : VX_WALK_NONE;
    __syncthreads();
    const uint32_t start_e = lds.start_e, goal_e = lds.goal_e;  // (the same in every thread)
    const uint32_t seed_bit = 1u << s.seed_at[0];
    const uint32_t start_row = start_e != VX_WALK_NONE ? vxb::flood_row_of(start_e, s.seed_at[2]) : VX_WALK_NONE;
    const uint32_t goal_row = goal_e != VX_WALK_NONE ? vxb::flood_row_of(goal_e, goal.rz) : VX_WALK_NONE;
    const uint32_t goal_bit = goal_e != VX_WALK_NONE ? 1u << goal.rx : 0u;
    const bool goal_is_start = goal_row != VX_WALK_NONE && goal_row == start_row && goal_bit == seed_bit;

    // 5  the owned rows
    const uint32_t e = t & (vxb::kFloodSide - 1u), rz0 = t >> 5;
    vxb::WalkRow rows[vxb::kFloodOwned];
    uint32_t reached[vxb::kFloodOwned];
#pragma unroll
    for (uint32_t k = 0; k < vxb::kFloodOwned; ++k) {
        const uint32_t r = t + k * vxb::kFloodThreads, rz = rz0 + 8u * k;
        rows[k] = vxb::walk_row(lds.passable + rz * vxb::kFloodSide, e, s);
        reached[k] = r == start_row ? seed_bit : 0u;
        if (r == start_row) lds.frontier[0][r] = seed_bit, lds.up[0][r] = seed_bit & rows[k].up_ok;
        if (FIELD && e >= 1u && e <= s.size[1] && rz < s.size[2]) {
            const uint32_t at = vxb::walk_field_row(s, e - 1u, rz);
            for (uint32_t rx = 0; rx < s.size[0]; ++rx) lds.field[at + rx] = ((rows[k].stand >> rx) & 1u) ? uint8_t(VX_WALK_UNREACHED) : uint8_t(VX_WALK_NO_STAND);
            if (reached[k]) lds.field[at + s.seed_at[0]] = 0;
        }
    }
    if (FIELD && t < 16u) {
        const uint32_t voxels = vxb::walk_voxels(s);
        if (voxels + t < vxb::flood_round16(voxels)) lds.field[voxels + t] = uint8_t(VX_WALK_NO_STAND);
    }
    if (t == 0) lds.goal_step = goal_is_start ? 0u : VX_WALK_NONE;
    __syncthreads();

    // 6  the steps
    const bool stop = (s.flags & VX_WALK_STOP_AT_GOAL) != 0u;
    const uint32_t max_steps = stop && goal_is_start ? 0u : s.max_steps;
    uint32_t farthest = 0u;
#pragma nounroll
    for (uint32_t step = 1; step <= max_steps; ++step) {
        const uint32_t *const cur = lds.frontier[(step - 1u) & 1u], *const cur_up = lds.up[(step - 1u) & 1u];
        uint32_t *const next = lds.frontier[step & 1u], *const next_up = lds.up[step & 1u];
        uint32_t any = 0u;
#pragma unroll
        for (uint32_t k = 0; k < vxb::kFloodOwned; ++k) {
            const uint32_t r = t + k * vxb::kFloodThreads, rz = rz0 + 8u * k;
            const uint32_t found = vxb::walk_step(cur, cur_up, r, e, rz, s, rows[k], reached[k]);
            next[r] = found;
            next_up[r] = found & rows[k].up_ok;
            reached[k] |= found;
            any |= found;
            if (found) {
                if (r == goal_row && (found & goal_bit)) lds.goal_step = step;
                if (FIELD) {
                    const uint32_t at = vxb::walk_field_row(s, e - 1u, rz);
                    for (uint32_t m = found; m; m &= m - 1u) lds.field[at + uint32_t(__builtin_ctz(m))] = uint8_t(step);
                }
            }
        }
        if (!__syncthreads_or(int(any))) break;  // (the same answer in every thread: all leave, or none)
        farthest = step;
        if (stop && lds.goal_step == step) break;  // (written before the barrier, if at all; later writes hold later steps)
    }

    // 7  the record
    if (info) {  // (a kernel argument: uniform)
        vxb::FloodAcc acc = {0u, 0u};
#pragma unroll
        for (uint32_t k = 0; k < vxb::kFloodOwned; ++k) vxb::walk_fold_row(acc, s, e, rz0 + 8u * k, reached[k]);
        fold_put(lds.fold, wave, lane, acc, walk_fold);
    }
    __syncthreads();  // (the fold's words; the last step's bytes of the field; the goal's step)
    const uint32_t path_steps = lds.goal_step;
    if (info && t == 0) store_record(info + n, vxb::walk_record(fold_take(lds.fold, walk_fold), farthest, lds.seed_value, start_e, goal_e, path_steps));
    if (FIELD) {
        const WalkOutputs o = outputs();
        // 8  the path
        if (o.path_out) {  // (a kernel argument: uniform)
            if (wave == 0 && path_steps != VX_WALK_NONE) {
                uint32_t x = goal.rx, at_e = goal_e, z = goal.rz, k = path_steps;
#pragma nounroll
                for (uint32_t trip = 0; trip < s.max_steps && k >= 1u; ++trip, --k) {
                    if (lane == 0 && k - 1u < s.path_capacity) lds.path[k - 1u] = vxb::walk_pack(x, at_e - 1u, z);
                    const uint32_t from = lane < 4u * (2u + s.drop) ? vxb::walk_candidate(lds.passable, lds.field, s, x, at_e, z, k, lane) : VX_WALK_NONE;
                    const uint64_t votes = __ballot(from != VX_WALK_NONE);
                    if (!votes) break;  // (cannot happen: a cell of step k was found from one of step k - 1)
                    const uint32_t took = uint32_t(__builtin_amdgcn_readlane(int(from), int(__builtin_ctzll(votes))));
                    x = took & 0xffu, at_e = (took >> 8) & 0xffu, z = took >> 16;
                }
            }
            __syncthreads();  // (reached by every thread: path_out is uniform)
            if (t < o.path_chunks) o.path_out[t] = reinterpret_cast<const uint4*>(lds.path)[t];
        }
        if (o.out) store_field(o.out, lds.field, o.chunks, t, vxb::kFloodThreads);
    }
}

}  // namespace

namespace vxk {

hipError_t launch_walk_points(int svo, hipStream_t stream, const SceneArgs& sc, const void* pos, uint32_t pos_stride, const void* goal, uint32_t goal_stride, uint32_t count,
                              const vx_walk_shape& shape, uint8_t* fields, uint32_t field_stride, uint32_t* paths, vx_walk_info* info) {
    static_assert(sizeof(vx_walk_info) == 32, "two 16-byte stores");
    if (!goal || shape.path_capacity == 0) paths = nullptr;  // no path is written
    if (count == 0 || count > vxb::kMaxCount || (!fields && !info && !paths)) return hipErrorInvalidValue;
    // the kernel's own bounds, whatever the caller checked: rows and bytes of LDS are indexed by these
    if (!sizes_within(shape.size, vxb::kFloodSide)) return hipErrorInvalidValue;
    if (shape.seed_at[0] >= shape.size[0] || shape.seed_at[1] >= shape.size[1] || shape.seed_at[2] >= shape.size[2]) return hipErrorInvalidValue;
    if (shape.height == 0 || shape.height > vxb::kWalkMaxHeight || shape.size[1] + shape.height > vxb::kFloodSide) return hipErrorInvalidValue;
    if (shape.max_steps > VX_WALK_MAX_STEPS || shape.climb > 1u || shape.drop > vxb::kWalkMaxDrop) return hipErrorInvalidValue;
    if (shape.path_capacity > vxb::kWalkMaxPath || shape.path_capacity % 4u) return hipErrorInvalidValue;
    if (!field_stride_ok(fields, field_stride, vxb::walk_voxels(shape))) return hipErrorInvalidValue;
    const dim3 grid(count, 1, 1), block(vxb::kFloodThreads);
    const uint8_t *p = static_cast<const uint8_t*>(pos), *g = static_cast<const uint8_t*>(goal);
    return for_format(svo, [&](auto f) {
        constexpr int S = decltype(f)::value;
        if (fields || paths) hipLaunchKernelGGL((walk_points_kernel<S, true>), grid, block, 0, stream, sc, p, pos_stride, g, goal_stride, shape, fields, field_stride, paths, info);
        else hipLaunchKernelGGL((walk_points_kernel<S, false>), grid, block, 0, stream, sc, p, pos_stride, g, goal_stride, shape, fields, field_stride, paths, info);
    });
}

}  // namespace vxk

// Step distances through air around a batch of positions (vx_flood_points; include/voxel_hip.h): the breadth-first search a caller of the
// reference would run on the host over get_block (gameplay.rs:161-201), asked of the world's OWN bytes through vx_blocks.hpp's descent. The
// work is shared out by QUERY: a workgroup of 256 threads owns one position and its box of up to 32 x 32 x 32 cells.
//   the box: seed = floor(p) per component saturated to int32 (vx_scan.hpp's rule), lo = seed - seed_at modulo 2^32, as vxb::Region keeps a
//   box: a wrapped coordinate is below 2^23 exactly when the true one lies inside a world. A NaN or infinite component is no position.
//   rows: the cells (0..size.x, ry, rz) of the box are bit rx of row rz * 32 + ry, 1,024 rows whatever the size; rows and bits beyond the size
//   stay 0. The field keeps vx_read_region's layout: the byte of cell (rx, ry, rz) is at (rz * size.y + ry) * size.x + rx.
//   loading: a wave takes all bricks along x of one (brick y, brick z) of the box's cover (at most 5 x 5 such brick rows of at most 5 bricks);
//   lane l reads the column along x at (y, z) = (l & 7, l >> 3) of each (brick_column_along, axis 0) and ORs its passable bits into its row.
//   One lane of one wave holds each row: plain stores, no atomics. The lane that meets the seed's cell keeps its value.
//   a step: next = (f << 1 | f >> 1 | f[y - 1] | f[y + 1] | f[z - 1] | f[z + 1]) & passable & ~reached, a row at a time; rows on a face of
//   the box take no neighbour from beyond it; `passable` holds no bit beyond size.x. Thread t owns rows t, t + 256, t + 512, t + 768.
//   the record: the reached bits counted, the faces of the box they touch, the last step that found a new cell, the seed's value.
// flood_points runs whole calls on one thread, brick by brick, row by row and step by step as the kernel runs them (the host test harness).
// The reader W is vx_blocks.hpp's. The standard library and voxel_hip.h only -- no HIP header, no HIP call.
#pragma once

#include <cstddef>

#include "vx_scan.hpp"

namespace vxb {

constexpr uint32_t kFloodSide = 32, kFloodRows = kFloodSide * kFloodSide;  // a box is at most 32 cells an axis: a row is a dword
constexpr uint32_t kFloodThreads = 256, kFloodOwned = kFloodRows / kFloodThreads;  // rows a thread owns
constexpr uint32_t kFloodLanes = kBrick * kBrick;

VXB_FN bool flood_has_position(const float p[3]) { return is_finite(p[0]) && is_finite(p[1]) && is_finite(p[2]); }

VXB_FN bool flood_passable(uint32_t value, uint32_t pass_value) { return value == 0 || (pass_value != 0 && value == pass_value); }

VXB_FN uint32_t flood_voxels(const vx_flood_shape& s) { return s.size[0] * s.size[1] * s.size[2]; }
VXB_FN uint32_t flood_round16(uint32_t v) { return (v + 15u) & ~15u; }

// The box of a query and the bricks of its cover, modulo 2^32 (p has a position).
struct FloodBox {
    uint32_t lo[3];
    uint32_t first[3], count[3];  // the first brick's corner (a multiple of 8), how many bricks along each axis (1..5)
};
VXB_FN FloodBox flood_box(const float p[3], const vx_flood_shape& s) {
    FloodBox b;
    for (int a = 0; a < 3; ++a) {
        b.lo[a] = uint32_t(floor_saturated(p[a])) - s.seed_at[a];
        b.first[a] = b.lo[a] & ~(kBrick - 1u);
        b.count[a] = ((b.lo[a] & (kBrick - 1u)) + s.size[a] + kBrick - 1u) >> kBrickLog2;
    }
    return b;
}

VXB_FN uint32_t flood_row_of(uint32_t ry, uint32_t rz) { return rz * kFloodSide + ry; }
VXB_FN uint32_t flood_seed_row(const vx_flood_shape& s) { return flood_row_of(s.seed_at[1], s.seed_at[2]); }
// where in the field the bytes of row (ry, rz) begin
VXB_FN uint32_t flood_field_row(const vx_flood_shape& s, uint32_t ry, uint32_t rz) { return (rz * s.size[1] + ry) * s.size[0]; }

// What a lane does for one brick of its brick row: column (y, z) = (i, j) of the brick along x, the cells of it that lie in the box and are
// passable, into `row`. A lane whose column lies outside the box loads nothing; a brick of air, outside the world or answered above the
// brick is filled in with no load (brick_column_along). The lane that meets the seed's cell keeps its value.
template <int FMT, class W>
VXB_FN void flood_brick_lane(const W& w, const vx_flood_shape& s, const FloodBox& box, const Brick& b, uint32_t i, uint32_t j, uint32_t& row, uint32_t& seed_value) {
    const uint32_t ry = b.corner[1] + i - box.lo[1], rz = b.corner[2] + j - box.lo[2];
    if (ry >= s.size[1] || rz >= s.size[2]) return;
    uint32_t value[kBrick];
    brick_column_along<FMT, false>(w, b, 0u, i, j, value, nullptr);
    const bool seed_row = ry == s.seed_at[1] && rz == s.seed_at[2];
    for (uint32_t k = 0; k < kBrick; ++k) {
        const uint32_t rx = b.corner[0] + k - box.lo[0];
        const bool in = rx < s.size[0];
        row |= (in && flood_passable(value[k], s.pass_value)) ? 1u << (rx & 31u) : 0u;
        seed_value = (seed_row && rx == s.seed_at[0]) ? value[k] : seed_value;
    }
}

// One step of a row: f its frontier, ym, yp, zm, zp those of the rows at y - 1, y + 1, z - 1, z + 1 (0 where the row lies on that face of the
// box). The cells reached by this step.
VXB_FN uint32_t flood_step(uint32_t f, uint32_t ym, uint32_t yp, uint32_t zm, uint32_t zp, uint32_t passable, uint32_t reached) {
    return ((f << 1) | (f >> 1) | ym | yp | zm | zp) & passable & ~reached;
}

// What the reached rows say of a flood: folded row by row, then across the threads (sums and ORs: any order gives the same)
struct FloodAcc {
    uint32_t reached, faces;
};
VXB_FN void flood_fold_row(FloodAcc& a, const vx_flood_shape& s, uint32_t ry, uint32_t rz, uint32_t reached) {
    if (!reached) return;
    a.reached += popc(reached);
    a.faces |= (reached & 1u) | (((reached >> (s.size[0] - 1u)) & 1u) << 1) | (ry == 0 ? 4u : 0u) | (ry + 1u == s.size[1] ? 8u : 0u) | (rz == 0 ? 16u : 0u) |
               (rz + 1u == s.size[2] ? 32u : 0u);
}
VXB_FN vx_flood_info flood_record(const FloodAcc& a, uint32_t farthest, uint32_t seed_value) {
    vx_flood_info r = {a.reached, farthest, a.faces, seed_value};
    return r;
}
VXB_FN vx_flood_info flood_no_position() {
    vx_flood_info r = {VX_FLOOD_INVALID, 0u, 0u, 0u};
    return r;
}
// dword d of the field of a position that is no position: VX_FLOOD_NO_POSITION below the voxel count, VX_FLOOD_BLOCKED from there on
VXB_FN uint32_t flood_no_position_word(uint32_t d, uint32_t voxels) {
    uint32_t word = 0;
    for (uint32_t k = 0; k < 4; ++k) word |= (4u * d + k < voxels ? uint32_t(VX_FLOOD_NO_POSITION) : uint32_t(VX_FLOOD_BLOCKED)) << (8u * k);
    return word;
}

// A whole query on one thread, as the kernel's workgroup runs it. field: round16(voxels) bytes, or null; info: a record, or null.
template <int FMT, class W>
inline void flood_query(const W& w, const float p[3], const vx_flood_shape& s, uint8_t* field, vx_flood_info* info) {
    const uint32_t voxels = flood_voxels(s), padded = flood_round16(voxels);
    if (!flood_has_position(p)) {
        if (field)
            for (uint32_t d = 0; d < padded / 4; ++d) {
                const uint32_t word = flood_no_position_word(d, voxels);
                __builtin_memcpy(field + 4 * d, &word, 4);
            }
        if (info) *info = flood_no_position();
        return;
    }
    const FloodBox box = flood_box(p, s);
    static thread_local uint32_t passable[kFloodRows], reached[kFloodRows], frontier[2][kFloodRows];
    for (uint32_t r = 0; r < kFloodRows; ++r) passable[r] = reached[r] = frontier[0][r] = frontier[1][r] = 0;
    uint32_t seed_value = 0;
    // loading: the brick rows of the cover, one after the other (the kernel: four waves take them in turn)
    for (uint32_t n = 0; n < box.count[1] * box.count[2]; ++n) {
        const uint32_t cy = box.first[1] + (n % box.count[1]) * kBrick, cz = box.first[2] + (n / box.count[1]) * kBrick;
        uint32_t row[kFloodLanes];
        for (uint32_t lane = 0; lane < kFloodLanes; ++lane) row[lane] = 0;
        for (uint32_t bx = 0; bx < box.count[0]; ++bx) {
            const Brick b = enter_brick_at<FMT>(w, box.first[0] + bx * kBrick, cy, cz);
            for (uint32_t lane = 0; lane < kFloodLanes; ++lane) flood_brick_lane<FMT>(w, s, box, b, lane & 7u, lane >> 3, row[lane], seed_value);
        }
        for (uint32_t lane = 0; lane < kFloodLanes; ++lane) {
            const uint32_t ry = cy + (lane & 7u) - box.lo[1], rz = cz + (lane >> 3) - box.lo[2];
            if (ry < s.size[1] && rz < s.size[2]) passable[flood_row_of(ry, rz)] = row[lane];
        }
    }
    const uint32_t seed_row = flood_seed_row(s), seed_bit = 1u << s.seed_at[0];
    if (s.flags & VX_FLOOD_SEED_ALWAYS) passable[seed_row] |= seed_bit;
    if (field) {
        for (uint32_t rz = 0; rz < s.size[2]; ++rz)
            for (uint32_t ry = 0; ry < s.size[1]; ++ry)
                for (uint32_t rx = 0; rx < s.size[0]; ++rx)
                    field[flood_field_row(s, ry, rz) + rx] = ((passable[flood_row_of(ry, rz)] >> rx) & 1u) ? uint8_t(VX_FLOOD_UNREACHED) : uint8_t(VX_FLOOD_BLOCKED);
        for (uint32_t at = voxels; at < padded; ++at) field[at] = uint8_t(VX_FLOOD_BLOCKED);
    }
    reached[seed_row] = frontier[0][seed_row] = passable[seed_row] & seed_bit;
    if (field && reached[seed_row]) field[flood_field_row(s, s.seed_at[1], s.seed_at[2]) + s.seed_at[0]] = 0;
    uint32_t farthest = 0;
    for (uint32_t step = 1; step <= s.max_steps; ++step) {
        const uint32_t* cur = frontier[(step - 1u) & 1u];
        uint32_t* next = frontier[step & 1u];
        uint32_t any = 0;
        for (uint32_t t = 0; t < kFloodThreads; ++t)
            for (uint32_t k = 0; k < kFloodOwned; ++k) {
                const uint32_t r = t + k * kFloodThreads, ry = r & (kFloodSide - 1u), rz = r / kFloodSide;
                uint32_t found = 0;
                if (ry < s.size[1] && rz < s.size[2])
                    found = flood_step(cur[r], ry > 0 ? cur[r - 1] : 0u, ry + 1u < s.size[1] ? cur[r + 1] : 0u, rz > 0 ? cur[r - kFloodSide] : 0u,
                                       rz + 1u < s.size[2] ? cur[r + kFloodSide] : 0u, passable[r], reached[r]);
                next[r] = found;
                reached[r] |= found;
                any |= found;
                if (field)
                    for (uint32_t m = found; m; m &= m - 1u) field[flood_field_row(s, ry, rz) + uint32_t(__builtin_ctz(m))] = uint8_t(step);
            }
        if (!any) break;
        farthest = step;
    }
    if (info) {
        FloodAcc acc = {0u, 0u};
        for (uint32_t r = 0; r < kFloodRows; ++r) flood_fold_row(acc, s, r & (kFloodSide - 1u), r / kFloodSide, reached[r]);
        *info = flood_record(acc, farthest, seed_value);
    }
}

// the whole of vx_flood_points on one thread (the host test harness). field_stride: as the call takes it (0: the voxel count rounded up to 16)
template <int FMT, class W>
inline void flood_points(const W& w, const uint8_t* pos, uint32_t pos_stride, uint32_t count, const vx_flood_shape& s, uint8_t* fields, uint32_t field_stride,
                         vx_flood_info* info) {
    const uint32_t stride = field_stride ? field_stride : flood_round16(flood_voxels(s));
    for (uint32_t n = 0; n < count; ++n) {
        float p[3];
        __builtin_memcpy(p, pos + size_t(n) * pos_stride, 12);
        flood_query<FMT>(w, p, s, fields ? fields + size_t(n) * stride : nullptr, info ? info + n : nullptr);
    }
}

// the rules of the call that need no device: what is wrong, naming the field, or null. (Alignment of device memory: blocks_runtime.cpp.)
inline const char* check_flood(const void* pos, uint32_t pos_stride, uint32_t count, const vx_flood_shape* s, const void* fields, uint32_t field_stride,
                               const void* info) {
    if (count == 0) return nullptr;  // nothing is read or written: nothing to refuse
    if (count > kMaxCount) return "count exceeds 16777216 (2^24)";
    if (!s) return "null shape";
    if (!fields && !info) return "fields and info are both null";
    if (const char* what = check_points(pos, pos_stride, count, fields ? fields : info)) return what;  // (its `out`: the output there is)
    if (const char* what = size_rule(s->size, kFloodSide, "size: every component must be 1..32", s->seed_at)) return what;
    if (s->max_steps > VX_FLOOD_MAX_STEPS) return "max_steps exceeds VX_FLOOD_MAX_STEPS (250)";
    if (s->flags & ~uint32_t(VX_FLOOD_SEED_ALWAYS)) return "flags holds a bit other than VX_FLOOD_SEED_ALWAYS";
    const uint32_t voxels = flood_voxels(*s);
    if (fields) return field_stride_rule(count, field_stride, voxels, flood_round16(voxels), "field_stride must be 0, or a multiple of 16 and at least size.x * size.y * size.z");
    return nullptr;
}

}  // namespace vxb

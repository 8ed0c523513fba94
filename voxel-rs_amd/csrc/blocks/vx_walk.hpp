// Walking distances and paths for ground agents around a batch of positions (vx_walk_points; include/voxel_hip.h): the search a caller of
// the reference would run on the host over get_block (gameplay.rs:161-201), asked of the world's OWN bytes. vx_flood.hpp's box, brick
// loading and rows of 32 bits, under a different graph: its nodes are judged over several layers, its edges are directed (up one, down
// several), and it ends in a serial back-trace. A workgroup of 256 threads owns one query.
//   layers: the box's cells (0..size.x, ry, rz) are bit rx of row rz * 32 + e with e = ry + 1: layer 0 lies below the box, layers size.y + 1
//   .. size.y + height - 1 above it -- size.y + height <= 32 layers, loaded as vx_flood.hpp loads a box of that height whose seed cell lies
//   one layer higher (walk_load_shape). Rows and bits beyond stay 0.
//   standable: stand[e] = P[e] & .. & P[e + height - 1] & ~P[e - 1] for e in 1..size.y (P the passable rows of the column (rz)): walk_row,
//   which also gives the row's up_ok = P[e + height] ("a cell here may step up", e < size.y) and clear[d - 1] = P[e + height] & .. & P[e +
//   height + d - 1] ("clear above me for a drop of d", e + d <= size.y).
//   a step (walk_step): beside(X, r) = X[r] << 1 | X[r] >> 1 | X[r - 32] | X[r + 32] (no row beyond a z face). With F the frontier and U =
//   F & up_ok the cells of it that may step up: found[e] = (beside(F, e) | beside(U, e - 1) | beside(F, e + d) & clear[d - 1] for d <=
//   drop) & stand & ~reached. One word a neighbour and edge kind.
//   settling (walk_settle), the goal's cell (walk_goal_cell), the back-trace's candidates in their order (walk_candidate), the record's
//   fold (walk_fold_row, walk_record) and the rules (check_walk).
// walk_points runs whole calls on one thread, row by row, step by step and candidate by candidate as the kernel runs them (the host test
// harness). The reader W is vx_blocks.hpp's. The standard library and voxel_hip.h only -- no HIP header, no HIP call.
#pragma once

#include <cstddef>

#include "vx_flood.hpp"

namespace vxb {

constexpr uint32_t kWalkMaxPath = 252;        // entries of a path: 63 16-byte stores
constexpr uint32_t kWalkMaxBytes = 1u << 24;  // of all paths of a call (the fields: vx_rules.hpp)
constexpr uint32_t kWalkMaxHeight = 4, kWalkMaxDrop = 3;
constexpr uint32_t kWalkFieldBytes = kFloodSide * (kFloodSide - 1u) * kFloodSide;  // size.y <= 31: a multiple of 16

VXB_FN uint32_t walk_voxels(const vx_walk_shape& s) { return s.size[0] * s.size[1] * s.size[2]; }
VXB_FN uint32_t walk_layers(const vx_walk_shape& s) { return s.size[1] + s.height; }
VXB_FN uint32_t walk_field_row(const vx_walk_shape& s, uint32_t ry, uint32_t rz) { return (rz * s.size[1] + ry) * s.size[0]; }
VXB_FN uint32_t walk_pack(uint32_t rx, uint32_t ry, uint32_t rz) { return rx | ry << 8 | rz << 16; }

// The box whose passable rows a query needs, as vx_flood.hpp loads one: the layers below and above the walk's box with it.
VXB_FN vx_flood_shape walk_load_shape(const vx_walk_shape& s) {
    vx_flood_shape f = {{s.size[0], walk_layers(s), s.size[2]}, {s.seed_at[0], s.seed_at[1] + 1u, s.seed_at[2]}, 0u, s.pass_value, 0u};
    return f;
}

// What the owner of row (e, rz) keeps of it. column: the 32 passable rows of rz, layer e at column[e].
struct WalkRow {
    uint32_t stand, up_ok, clear[kWalkMaxDrop];
};
VXB_FN WalkRow walk_row(const uint32_t* column, uint32_t e, const vx_walk_shape& s) {
    WalkRow r = {0u, 0u, {0u, 0u, 0u}};
    if (e == 0 || e > s.size[1]) return r;
    uint32_t head = column[e];
    for (uint32_t j = 1; j < kWalkMaxHeight; ++j)
        if (j < s.height) head &= column[e + j];
    r.stand = head & ~column[e - 1u];
    if (s.climb && e < s.size[1]) r.up_ok = column[e + s.height];
    uint32_t clear = 0xffffffffu;
    for (uint32_t d = 1; d <= kWalkMaxDrop; ++d)
        if (d <= s.drop && e + d <= s.size[1]) {
            clear &= column[e + s.height + d - 1u];
            r.clear[d - 1u] = clear;
        }
    return r;
}

// the cells beside those of row r of `f` (row r itself is another layer of the asking row's column, or the asking row's own)
VXB_FN uint32_t walk_beside(const uint32_t* f, uint32_t r, uint32_t rz, uint32_t size_z) {
    const uint32_t own = f[r];
    return (own << 1) | (own >> 1) | (rz > 0 ? f[r - kFloodSide] : 0u) | (rz + 1u < size_z ? f[r + kFloodSide] : 0u);
}

// One step of row r = rz * 32 + e: f the frontier, up the cells of it that may step up. The cells reached by this step.
VXB_FN uint32_t walk_step(const uint32_t* f, const uint32_t* up, uint32_t r, uint32_t e, uint32_t rz, const vx_walk_shape& s, const WalkRow& row, uint32_t reached) {
    if (!(row.stand & ~reached)) return 0u;  // (so e is in 1..size.y below)
    uint32_t from = walk_beside(f, r, rz, s.size[2]);
    if (s.climb) from |= walk_beside(up, r - 1u, rz, s.size[2]);
    for (uint32_t d = 1; d <= kWalkMaxDrop; ++d)
        if (d <= s.drop && e + d <= s.size[1]) from |= walk_beside(f, r + d, rz, s.size[2]) & row.clear[d - 1u];
    return from & row.stand & ~reached;
}

// The layer on which an agent put into cell (bit, e), e in 1..size.y, comes to stand, or VX_WALK_NONE: no headroom there, or it falls
// out of the box's bottom.
VXB_FN uint32_t walk_settle(const uint32_t* column, uint32_t bit, uint32_t e, const vx_walk_shape& s) {
    for (uint32_t j = 0; j < kWalkMaxHeight; ++j)
        if (j < s.height && !(column[e + j] & bit)) return VX_WALK_NONE;
    for (uint32_t trip = 0; trip < kFloodSide && e >= 1u && (column[e - 1u] & bit); ++trip) --e;
    return e >= 1u ? e : VX_WALK_NONE;
}

// The goal's cell inside the box of position p, by true integers (a wrapped difference would put far goals into the box).
struct WalkCell {
    uint32_t rx, ry, rz;
    bool in;
};
VXB_FN WalkCell walk_goal_cell(const float p[3], const float g[3], const vx_walk_shape& s) {
    uint32_t rel[3];
    bool in = true;
    for (int a = 0; a < 3; ++a) {
        const int64_t d = int64_t(floor_saturated(g[a])) - (int64_t(floor_saturated(p[a])) - int64_t(s.seed_at[a]));
        in = in && d >= 0 && d < int64_t(s.size[a]);
        rel[a] = uint32_t(d);
    }
    WalkCell c = {rel[0], rel[1], rel[2], in};
    return c;
}

// Candidate c of the back-trace from cell (x, layer e, z) of step k: side c / (2 + drop) in the order -x, +x, -z, +z; per side level, from
// below (the up edge), from above by d = 1..drop. The candidate as rx | layer << 8 | rz << 16 when it lies in the box, has step k - 1 and
// an edge to the cell; else VX_WALK_NONE. passable: all rows; field: the byte field.
VXB_FN uint32_t walk_candidate(const uint32_t* passable, const uint8_t* field, const vx_walk_shape& s, uint32_t x, uint32_t e, uint32_t z, uint32_t k, uint32_t c) {
    const uint32_t kinds = 2u + s.drop, side = c / kinds, kind = c % kinds;
    uint32_t px = x, pz = z, pe = e;
    if (side == 0) { if (x == 0) return VX_WALK_NONE; px = x - 1u; }
    else if (side == 1) { if (x + 1u >= s.size[0]) return VX_WALK_NONE; px = x + 1u; }
    else if (side == 2) { if (z == 0) return VX_WALK_NONE; pz = z - 1u; }
    else if (side == 3) { if (z + 1u >= s.size[2]) return VX_WALK_NONE; pz = z + 1u; }
    else return VX_WALK_NONE;
    if (kind == 1u) {
        if (!s.climb || e < 2u) return VX_WALK_NONE;
        pe = e - 1u;
        if (!((passable[pz * kFloodSide + pe + s.height] >> px) & 1u)) return VX_WALK_NONE;
    } else if (kind >= 2u) {
        const uint32_t d = kind - 1u;
        pe = e + d;
        if (pe > s.size[1]) return VX_WALK_NONE;
        for (uint32_t j = 0; j < kWalkMaxDrop; ++j)
            if (j < d && !((passable[z * kFloodSide + e + s.height + j] >> x) & 1u)) return VX_WALK_NONE;
    }
    if (field[walk_field_row(s, pe - 1u, pz) + px] != uint8_t(k - 1u)) return VX_WALK_NONE;
    return walk_pack(px, pe, pz);
}

// What the reached rows say of a walk, as vx_flood.hpp folds a flood's (e: the row's layer, 1..size.y where reached != 0)
VXB_FN void walk_fold_row(FloodAcc& a, const vx_walk_shape& s, uint32_t e, uint32_t rz, uint32_t reached) {
    if (!reached) return;
    a.reached += popc(reached);
    a.faces |= (reached & 1u) | (((reached >> (s.size[0] - 1u)) & 1u) << 1) | (e == 1u ? 4u : 0u) | (e == s.size[1] ? 8u : 0u) | (rz == 0 ? 16u : 0u) |
               (rz + 1u == s.size[2] ? 32u : 0u);
}
VXB_FN uint32_t walk_ry(uint32_t e) { return e == VX_WALK_NONE ? VX_WALK_NONE : e - 1u; }
VXB_FN vx_walk_info walk_record(const FloodAcc& a, uint32_t farthest, uint32_t seed_value, uint32_t start_e, uint32_t goal_e, uint32_t path_steps) {
    vx_walk_info r = {a.reached, farthest, a.faces, seed_value, walk_ry(start_e), walk_ry(goal_e), path_steps, 0u};
    return r;
}
VXB_FN vx_walk_info walk_no_position() {
    vx_walk_info r = {VX_FLOOD_INVALID, 0u, 0u, 0u, VX_WALK_NONE, VX_WALK_NONE, VX_WALK_NONE, 0u};
    return r;
}

// A whole query on one thread, as the kernel's workgroup runs it. g: the goal, or null; field: round16(voxels) bytes, or null; path:
// path_capacity entries, or null; info: a record, or null.
template <int FMT, class W>
inline void walk_query(const W& w, const float p[3], const float* g, const vx_walk_shape& s, uint8_t* field, uint32_t* path, vx_walk_info* info) {
    static_assert(VX_WALK_NO_POSITION == VX_FLOOD_NO_POSITION && VX_WALK_NO_STAND == VX_FLOOD_BLOCKED, "flood_no_position_word serves both");
    const uint32_t voxels = walk_voxels(s), padded = flood_round16(voxels);
    if (path)
        for (uint32_t i = 0; i < s.path_capacity; ++i) path[i] = VX_WALK_NONE;
    if (!flood_has_position(p)) {
        if (field)
            for (uint32_t d = 0; d < padded / 4; ++d) {
                const uint32_t word = flood_no_position_word(d, voxels);
                __builtin_memcpy(field + 4 * d, &word, 4);
            }
        if (info) *info = walk_no_position();
        return;
    }
    const vx_flood_shape ls = walk_load_shape(s);
    const FloodBox box = flood_box(p, ls);
    static thread_local uint32_t passable[kFloodRows], reached[kFloodRows], frontier[2][kFloodRows], up[2][kFloodRows];
    static thread_local WalkRow rows[kFloodRows];
    static thread_local uint8_t bytes[kWalkFieldBytes];
    for (uint32_t r = 0; r < kFloodRows; ++r) passable[r] = reached[r] = frontier[0][r] = frontier[1][r] = up[0][r] = up[1][r] = 0;
    uint32_t seed_value = 0;
    // loading: vx_flood.hpp's, over the extended layers
    for (uint32_t n = 0; n < box.count[1] * box.count[2]; ++n) {
        const uint32_t cy = box.first[1] + (n % box.count[1]) * kBrick, cz = box.first[2] + (n / box.count[1]) * kBrick;
        uint32_t row[kFloodLanes];
        for (uint32_t lane = 0; lane < kFloodLanes; ++lane) row[lane] = 0;
        for (uint32_t bx = 0; bx < box.count[0]; ++bx) {
            const Brick b = enter_brick_at<FMT>(w, box.first[0] + bx * kBrick, cy, cz);
            for (uint32_t lane = 0; lane < kFloodLanes; ++lane) flood_brick_lane<FMT>(w, ls, box, b, lane & 7u, lane >> 3, row[lane], seed_value);
        }
        for (uint32_t lane = 0; lane < kFloodLanes; ++lane) {
            const uint32_t e = cy + (lane & 7u) - box.lo[1], rz = cz + (lane >> 3) - box.lo[2];
            if (e < ls.size[1] && rz < ls.size[2]) passable[flood_row_of(e, rz)] = row[lane];
        }
    }
    // settling (the kernel: one thread each)
    const uint32_t start_e = walk_settle(passable + s.seed_at[2] * kFloodSide, 1u << s.seed_at[0], s.seed_at[1] + 1u, s);
    uint32_t goal_e = VX_WALK_NONE;
    WalkCell goal = {0u, 0u, 0u, false};
    if (g && flood_has_position(g)) {
        goal = walk_goal_cell(p, g, s);
        if (goal.in) goal_e = walk_settle(passable + goal.rz * kFloodSide, 1u << goal.rx, goal.ry + 1u, s);
    }
    // the owned rows
    const bool bytes_needed = field || path;
    for (uint32_t r = 0; r < kFloodRows; ++r) {
        const uint32_t e = r & (kFloodSide - 1u), rz = r / kFloodSide;
        rows[r] = rz < s.size[2] ? walk_row(passable + rz * kFloodSide, e, s) : WalkRow{0u, 0u, {0u, 0u, 0u}};
        if (bytes_needed && e >= 1u && e <= s.size[1] && rz < s.size[2])
            for (uint32_t rx = 0; rx < s.size[0]; ++rx)
                bytes[walk_field_row(s, e - 1u, rz) + rx] = ((rows[r].stand >> rx) & 1u) ? uint8_t(VX_WALK_UNREACHED) : uint8_t(VX_WALK_NO_STAND);
    }
    const uint32_t seed_bit = 1u << s.seed_at[0];
    if (start_e != VX_WALK_NONE) {
        const uint32_t r = flood_row_of(start_e, s.seed_at[2]);
        reached[r] = frontier[0][r] = seed_bit;
        up[0][r] = seed_bit & rows[r].up_ok;
        if (bytes_needed) bytes[walk_field_row(s, start_e - 1u, s.seed_at[2]) + s.seed_at[0]] = 0;
    }
    const uint32_t goal_row = goal_e != VX_WALK_NONE ? flood_row_of(goal_e, goal.rz) : VX_WALK_NONE, goal_bit = goal_e != VX_WALK_NONE ? 1u << goal.rx : 0u;
    uint32_t goal_step = VX_WALK_NONE;
    if (goal_e != VX_WALK_NONE && goal_e == start_e && goal.rx == s.seed_at[0] && goal.rz == s.seed_at[2]) goal_step = 0u;
    const bool stop = (s.flags & VX_WALK_STOP_AT_GOAL) != 0;
    const uint32_t max_steps = stop && goal_step == 0u ? 0u : s.max_steps;
    uint32_t farthest = 0;
    for (uint32_t step = 1; step <= max_steps; ++step) {
        const uint32_t *cur = frontier[(step - 1u) & 1u], *cur_up = up[(step - 1u) & 1u];
        uint32_t *next = frontier[step & 1u], *next_up = up[step & 1u];
        uint32_t any = 0;
        for (uint32_t t = 0; t < kFloodThreads; ++t)
            for (uint32_t k = 0; k < kFloodOwned; ++k) {
                const uint32_t r = t + k * kFloodThreads, e = r & (kFloodSide - 1u), rz = r / kFloodSide;
                const uint32_t found = walk_step(cur, cur_up, r, e, rz, s, rows[r], reached[r]);
                next[r] = found;
                next_up[r] = found & rows[r].up_ok;
                reached[r] |= found;
                any |= found;
                if (r == goal_row && (found & goal_bit)) goal_step = step;
                if (bytes_needed)
                    for (uint32_t m = found; m; m &= m - 1u) bytes[walk_field_row(s, e - 1u, rz) + uint32_t(__builtin_ctz(m))] = uint8_t(step);
            }
        if (!any) break;
        farthest = step;
        if (stop && goal_step == step) break;
    }
    if (info) {
        FloodAcc acc = {0u, 0u};
        for (uint32_t r = 0; r < kFloodRows; ++r) walk_fold_row(acc, s, r & (kFloodSide - 1u), r / kFloodSide, reached[r]);
        *info = walk_record(acc, farthest, seed_value, start_e, goal_e, goal_step);
    }
    // the back-trace (the kernel: wave 0, a lane a candidate, a ballot picks the first)
    if (path && goal_step != VX_WALK_NONE) {
        uint32_t x = goal.rx, e = goal_e, z = goal.rz;
        for (uint32_t k = goal_step; k >= 1u; --k) {
            if (k - 1u < s.path_capacity) path[k - 1u] = walk_pack(x, e - 1u, z);
            uint32_t from = VX_WALK_NONE;
            for (uint32_t c = 0; c < 4u * (2u + s.drop) && from == VX_WALK_NONE; ++c) from = walk_candidate(passable, bytes, s, x, e, z, k, c);
            if (from == VX_WALK_NONE) break;  // (cannot happen: a cell of step k was found from one of step k - 1)
            x = from & 0xffu, e = (from >> 8) & 0xffu, z = from >> 16;
        }
    }
    if (field) {
        for (uint32_t at = 0; at < voxels; ++at) field[at] = bytes[at];
        for (uint32_t at = voxels; at < padded; ++at) field[at] = uint8_t(VX_WALK_NO_STAND);
    }
}

// the whole of vx_walk_points on one thread (the host test harness). field_stride: as the call takes it (0: the voxel count rounded up to 16)
template <int FMT, class W>
inline void walk_points(const W& w, const uint8_t* pos, uint32_t pos_stride, const uint8_t* goal, uint32_t goal_stride, uint32_t count, const vx_walk_shape& s,
                        uint8_t* fields, uint32_t field_stride, uint32_t* paths, vx_walk_info* info) {
    const uint32_t stride = field_stride ? field_stride : flood_round16(walk_voxels(s));
    const bool with_paths = goal && paths && s.path_capacity;
    for (uint32_t n = 0; n < count; ++n) {
        float p[3], g[3];
        __builtin_memcpy(p, pos + size_t(n) * pos_stride, 12);
        if (goal) __builtin_memcpy(g, goal + size_t(n) * goal_stride, 12);
        walk_query<FMT>(w, p, goal ? g : nullptr, s, fields ? fields + size_t(n) * stride : nullptr, with_paths ? paths + size_t(n) * s.path_capacity : nullptr,
                        info ? info + n : nullptr);
    }
}

// the rules of the call that need no device: what is wrong, naming the field, or null. (Alignment of device memory: blocks_runtime.cpp.)
inline const char* check_walk(const void* pos, uint32_t pos_stride, const void* goal, uint32_t goal_stride, uint32_t count, const vx_walk_shape* s, const void* fields,
                              uint32_t field_stride, const void* paths, const void* info) {
    if (count == 0) return nullptr;  // nothing is read or written: nothing to refuse
    if (count > kMaxCount) return "count exceeds 16777216 (2^24)";
    if (!s) return "null shape";
    if (!fields && !info && !paths) return "fields, info and paths are all null";
    if (paths && !goal) return "paths without goal";
    if (const char* what = check_points(pos, pos_stride, count, fields ? fields : info ? info : paths)) return what;  // (its `out`: the output there is)
    if (goal) {
        if (!stride_ok(goal_stride, true)) return "goal_stride must be 0, or a multiple of 4 and >= 12";
        if (!aligned_to_4(goal)) return "goal must be aligned to 4 bytes";
    }
    if (const char* what = size_rule(s->size, kFloodSide, "size: every component must be 1..32", s->seed_at)) return what;
    if (s->height == 0 || s->height > kWalkMaxHeight) return "height must be 1..4";
    if (s->size[1] + s->height > kFloodSide) return "size[1] + height exceeds 32";
    if (s->max_steps > VX_WALK_MAX_STEPS) return "max_steps exceeds VX_WALK_MAX_STEPS (250)";
    if (s->climb > 1u) return "climb must be 0 or 1";
    if (s->drop > kWalkMaxDrop) return "drop must be 0..3";
    if (s->path_capacity > kWalkMaxPath || s->path_capacity % 4u) return "path_capacity must be a multiple of 4 and at most 252";
    if (s->flags & ~uint32_t(VX_WALK_STOP_AT_GOAL)) return "flags holds a bit other than VX_WALK_STOP_AT_GOAL";
    const uint32_t voxels = walk_voxels(*s);
    const char* const at_least = "field_stride must be 0, or a multiple of 16 and at least size.x * size.y * size.z";
    if (fields)
        if (const char* what = field_stride_rule(count, field_stride, voxels, flood_round16(voxels), at_least)) return what;
    if (paths && uint64_t(count) * s->path_capacity * 4u > kWalkMaxBytes) return "count * path_capacity * 4 exceeds 16777216 (2^24) bytes";
    return nullptr;
}

}  // namespace vxb

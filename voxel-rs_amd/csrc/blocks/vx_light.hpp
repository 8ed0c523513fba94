// Sky and block light levels for a batch of boxes (vx_light_boxes; include/voxel_hip.h): the two breadth-first searches a caller of the
// reference would run on the host over get_block (gameplay.rs:161-201), asked of the world's OWN bytes through vx_blocks.hpp's descent and
// vx_scan.hpp's walk. The work is shared out by QUERY: a workgroup of 256 threads owns one box of up to 48 x 48 x 48 cells.
//   the rules: a cell is passable when its value is 0 or props[value] has VX_LIGHT_TRANSPARENT; it emits props[value] & 15 (air: nothing;
//   ids at or above props_count: opaque and dark). Sky: a passable cell with only passable cells above it up to the world's top is exposed and
//   has 15; every other passable cell has max(0, max over its six neighbours in the box - 1); impassable cells have 0. Block: a cell has at
//   least its emission; a passable one the larger of that and (max over its neighbours in the box - 1).
//   rows: the cells (0..size.x, ry, rz) of the box are bit rx of the 64-bit row rz * 48 + ry, 2,304 rows whatever the size; rows and bits
//   beyond the size stay 0. The field keeps vx_read_region's layout: the byte of cell (rx, ry, rz) is at (rz * size.y + ry) * size.x + rx.
//   loading: as vx_flood.hpp loads: a wave takes all bricks along x of one (brick y, brick z) of the box's cover (at most 7 x 7 such brick
//   rows of at most 7 bricks); lane l reads the column along x at (y, z) = (l & 7, l >> 3) of each and ORs the passable bit and the four bits
//   of the emission of each cell into five rows (LightRows).
//   exposure: above the box one chain of scan_line a column (x, z), upwards from lo.y + size.y to the world's top, again from the voxel
//   behind each transparent block it finds (column_open); a column beside the world, or a box whose top is at or above the world's, is open
//   with no scan. Inside the box the open bits of a z are ANDed with the passable rows from the top y downwards (the slab walk).
//   the spread: level-ordered, for L = 14 down to 1:
//       frontier_L = (spread(frontier_L+1) & passable & ~reached) | (sources_L & ~reached),
//   spread = f << 1 | f >> 1 | f[y - 1] | f[y + 1] | f[z - 1] | f[z + 1] (vx_flood.hpp's step on 64 bits; rows on a face of the box take
//   no neighbour from beyond it), frontier_15 = the exposed cells (sky) or the cells that emit 15 (block), sources_L = the cells that emit L
//   (block; none for the sky). A cell first met in frontier_L has level L. That is max over the sources s of (level_s - the length of the
//   shortest path from s through passable cells of the box), floored at 0 -- which is the unique solution of the per-cell rule above (a cell
//   takes the largest neighbour less one or its own source level; the levels fall by one a step, so the first frontier to meet a cell
//   carries the largest). An impassable source enters through sources_L alone and spreads, but nothing spreads into it.
//   The levels are kept as four bit planes a channel (LightLevels); the block channel's planes start as the emission planes, so that
//   sources_L is "the planes say L" of the cells not yet reached.
//   the record: the cells whose byte is not 0, the cells that emit, the columns whose top cell is exposed, the faces of the box on which a
//   cell has a level of 2 or more. A channel that a flag leaves out counts nothing: VX_LIGHT_NO_SKY gives open_columns 0 (no column is
//   scanned), VX_LIGHT_NO_BLOCKS gives sources 0.
// light_query runs a whole query on one thread in the order the kernel's workgroup runs it (the host test harness). The reader W is
// vx_blocks.hpp's. The standard library and voxel_hip.h only -- no HIP header, no HIP call.
#pragma once

#include <cstddef>

#include "vx_scan.hpp"

namespace vxb {

constexpr uint32_t kLightSide = VX_LIGHT_MAX_SIDE, kLightRows = kLightSide * kLightSide;  // a box is at most 48 cells an axis: a row is 64 bits
constexpr uint32_t kLightThreads = 256, kLightOwned = kLightRows / kLightThreads;           // rows a thread owns: 9
constexpr uint32_t kLightTop = 15, kLightSteps = 14;                                        // the levels 14 .. 1 are found by spreading
static_assert(kLightOwned * kLightThreads == kLightRows, "every row has an owner");

// props[value] of a block id (air, and ids the table does not hold: 0 -- but air passes)
VXB_FN uint32_t light_props(const uint8_t* props, uint32_t props_count, uint32_t value) { return (value != 0 && value < props_count) ? props[value] : 0u; }
VXB_FN bool light_passable(const uint8_t* props, uint32_t props_count, uint32_t value) {
    return value == 0 || (light_props(props, props_count, value) & VX_LIGHT_TRANSPARENT) != 0;
}
VXB_FN uint32_t light_emission(const uint8_t* props, uint32_t props_count, uint32_t value) { return light_props(props, props_count, value) & 15u; }

VXB_FN uint32_t light_voxels(const uint32_t size[3]) { return size[0] * size[1] * size[2]; }
VXB_FN uint32_t light_round16(uint32_t v) { return (v + 15u) & ~15u; }
VXB_FN uint32_t popc64(uint64_t v) { return uint32_t(__builtin_popcountll(v)); }

// The box of a query and the bricks of its cover, modulo 2^32 as vxb::Region keeps a box.
struct LightBox {
    uint32_t lo[3], size[3];
    uint32_t first[3], count[3];  // the first brick's corner (a multiple of 8), how many bricks along each axis (1..7)
    int64_t top;                  // lo.y + size.y as it is: where the exposure's scan begins
};
VXB_FN LightBox light_box(const int32_t lo[3], const uint32_t size[3]) {
    LightBox b;
    for (int a = 0; a < 3; ++a) {
        b.lo[a] = uint32_t(lo[a]);
        b.size[a] = size[a];
        b.first[a] = b.lo[a] & ~(kBrick - 1u);
        b.count[a] = ((b.lo[a] & (kBrick - 1u)) + size[a] + kBrick - 1u) >> kBrickLog2;
    }
    b.top = int64_t(lo[1]) + int64_t(size[1]);
    return b;
}

VXB_FN uint32_t light_row_of(uint32_t ry, uint32_t rz) { return rz * kLightSide + ry; }
// where in the field the bytes of row (ry, rz) begin
VXB_FN uint32_t light_field_row(const uint32_t size[3], uint32_t ry, uint32_t rz) { return (rz * size[1] + ry) * size[0]; }

// What a row is loaded as: its passable bits and the four bit planes of its cells' emission.
struct LightRows {
    uint64_t passable, emit[4];
};

// What a lane does for one brick of its brick row: column (y, z) = (i, j) of the brick along x, the cells of it that lie in the box, into
// `rows`. A lane whose column lies outside the box loads nothing.
template <int FMT, class W>
VXB_FN void light_brick_lane(const W& w, const uint8_t* props, uint32_t props_count, const LightBox& box, const Brick& b, uint32_t i, uint32_t j, LightRows& rows) {
    const uint32_t ry = b.corner[1] + i - box.lo[1], rz = b.corner[2] + j - box.lo[2];
    if (ry >= box.size[1] || rz >= box.size[2]) return;
    uint32_t value[kBrick];
    brick_column_along<FMT, false>(w, b, 0u, i, j, value, nullptr);
    for (uint32_t k = 0; k < kBrick; ++k) {
        const uint32_t rx = b.corner[0] + k - box.lo[0];
        const uint64_t bit = rx < box.size[0] ? uint64_t(1) << (rx & 63u) : 0u;
        const uint32_t p = light_props(props, props_count, value[k]);
        rows.passable |= (value[k] == 0 || (p & VX_LIGHT_TRANSPARENT)) ? bit : 0u;
        for (uint32_t e = 0; e < 4; ++e) rows.emit[e] |= ((p >> e) & 1u) ? bit : 0u;
    }
}

// Is the column (x, z) of the world open above the box: every cell from `top` up to the world's top passable? A column beside the world and
// a top at or above the world's are open with no scan; below the world is air. One scan_line after the other, each from the voxel behind
// the transparent block (a LOD voxel: behind all of it) the last one found: every trip goes up by at least one voxel.
template <int FMT, class W>
VXB_FN bool column_open(const W& w, const uint8_t* props, uint32_t props_count, uint32_t x, uint32_t z, int64_t top, uint32_t& trips) {
    const uint32_t depth = depth_of(w.head()), edge = 1u << depth;
    if ((x >> depth) || (z >> depth) || top >= int64_t(edge)) return true;
    uint32_t c = top < 0 ? 0u : uint32_t(top);
    for (;;) {
        const vx_scan_hit hit = scan_line<FMT>(w, 1u, true, x, z, c, edge - 1u, trips);
        if (hit.coord == VX_SCAN_NONE) return true;
        if (!light_passable(props, props_count, hit.value)) return false;
        const uint32_t last = uint32_t(hit.coord) | low_bits(int(hit.cell_log2));
        if (last >= edge - 1u) return true;
        c = last + 1u;
    }
}

// the shift-and-OR of a row and its four neighbour rows (0 where the row lies on that face of the box)
VXB_FN uint64_t light_spread(uint64_t f, uint64_t ym, uint64_t yp, uint64_t zm, uint64_t zp) { return (f << 1) | (f >> 1) | ym | yp | zm | zp; }

// The levels of a row's cells as four bit planes; set: the cells of `found` get level L, whatever they had.
struct LightLevels {
    uint64_t plane[4];
};
VXB_FN void light_set(LightLevels& v, uint64_t found, uint32_t level) {
    for (uint32_t e = 0; e < 4; ++e) v.plane[e] = ((level >> e) & 1u) ? (v.plane[e] | found) : (v.plane[e] & ~found);
}
// the cells whose planes say `level` (1..15)
VXB_FN uint64_t light_equal(const LightLevels& v, uint32_t level) {
    uint64_t m = ~uint64_t(0);
    for (uint32_t e = 0; e < 4; ++e) m &= ((level >> e) & 1u) ? v.plane[e] : ~v.plane[e];
    return m;
}
VXB_FN uint64_t light_any(const LightLevels& v) { return v.plane[0] | v.plane[1] | v.plane[2] | v.plane[3]; }
VXB_FN uint64_t light_bright(const LightLevels& v) { return v.plane[1] | v.plane[2] | v.plane[3]; }  // a level of 2 or more
VXB_FN uint32_t light_level_at(const LightLevels& v, uint32_t rx) {
    uint32_t level = 0;
    for (uint32_t e = 0; e < 4; ++e) level |= uint32_t((v.plane[e] >> rx) & 1u) << e;
    return level;
}
VXB_FN uint8_t light_byte(const LightLevels& sky, const LightLevels& block, uint32_t rx) { return uint8_t(light_level_at(sky, rx) << 4 | light_level_at(block, rx)); }

// One step of a row at level L: the cells the spread reaches, and (block channel) the cells that emit L; none that was reached before.
VXB_FN uint64_t light_step(uint64_t spread, uint64_t passable, uint64_t sources, uint64_t reached) { return ((spread & passable) | sources) & ~reached; }

// What the rows say of a box: folded row by row, then across the threads (sums and ORs: any order gives the same)
struct LightAcc {
    uint32_t lit, sources, open_columns, faces;
};
VXB_FN uint32_t light_faces(const uint32_t size[3], uint32_t ry, uint32_t rz, uint64_t bright) {
    if (!bright) return 0u;
    return uint32_t(bright & 1u) | (uint32_t((bright >> (size[0] - 1u)) & 1u) << 1) | (ry == 0 ? 4u : 0u) | (ry + 1u == size[1] ? 8u : 0u) | (rz == 0 ? 16u : 0u) |
           (rz + 1u == size[2] ? 32u : 0u);
}
VXB_FN void light_fold_row(LightAcc& a, const uint32_t size[3], uint32_t ry, uint32_t rz, const LightLevels& sky, const LightLevels& block) {
    a.lit += popc64(light_any(sky) | light_any(block));
    a.faces |= light_faces(size, ry, rz, light_bright(sky) | light_bright(block));
}
VXB_FN vx_light_info light_record(const LightAcc& a) {
    vx_light_info r = {a.lit, a.sources, a.open_columns, a.faces};
    return r;
}

// A whole query on one thread, as the kernel's workgroup runs it. props: props_count bytes; field: round16(voxels) bytes, or null; info: a
// record, or null.
template <int FMT, class W>
inline void light_query(const W& w, const int32_t lo[3], const vx_light_shape& s, uint8_t* field, vx_light_info* info) {
    const LightBox box = light_box(lo, s.size);
    const uint8_t* const props = s.props;
    const uint32_t props_count = s.props_count;
    const bool sky_wanted = !(s.flags & VX_LIGHT_NO_SKY), block_wanted = !(s.flags & VX_LIGHT_NO_BLOCKS);
    static thread_local LightRows loaded[kLightRows];
    static thread_local LightLevels sky[kLightRows], block[kLightRows];
    static thread_local uint64_t reached[kLightRows], frontier[2][kLightRows], open[kLightSide];
    for (uint32_t r = 0; r < kLightRows; ++r) {
        loaded[r] = LightRows{0u, {0u, 0u, 0u, 0u}};
        sky[r] = block[r] = LightLevels{{0u, 0u, 0u, 0u}};
        reached[r] = frontier[0][r] = frontier[1][r] = 0u;
    }
    // loading: the brick rows of the cover, one after the other (the kernel: four waves take them in turn)
    for (uint32_t n = 0; n < box.count[1] * box.count[2]; ++n) {
        const uint32_t cy = box.first[1] + (n % box.count[1]) * kBrick, cz = box.first[2] + (n / box.count[1]) * kBrick;
        LightRows rows[kBrick * kBrick];
        for (uint32_t lane = 0; lane < kBrick * kBrick; ++lane) rows[lane] = LightRows{0u, {0u, 0u, 0u, 0u}};
        for (uint32_t bx = 0; bx < box.count[0]; ++bx) {
            const Brick b = enter_brick_at<FMT>(w, box.first[0] + bx * kBrick, cy, cz);
            for (uint32_t lane = 0; lane < kBrick * kBrick; ++lane) light_brick_lane<FMT>(w, props, props_count, box, b, lane & 7u, lane >> 3, rows[lane]);
        }
        for (uint32_t lane = 0; lane < kBrick * kBrick; ++lane) {
            const uint32_t ry = cy + (lane & 7u) - box.lo[1], rz = cz + (lane >> 3) - box.lo[2];
            if (ry < box.size[1] && rz < box.size[2]) loaded[light_row_of(ry, rz)] = rows[lane];
        }
    }
    LightAcc acc = {0u, 0u, 0u, 0u};
    const auto in_box = [&](uint32_t r) { return r % kLightSide < box.size[1] && r / kLightSide < box.size[2]; };
    // one channel's spread from frontier[0] and reached[], the levels into v; sources: the block channel's
    const auto spread = [&](LightLevels* v, bool sources) {
        for (uint32_t step = 0; step < kLightSteps; ++step) {
            const uint32_t level = kLightSteps - step;
            const uint64_t* cur = frontier[step & 1u];
            uint64_t* next = frontier[(step + 1u) & 1u];
            uint64_t any = 0;
            for (uint32_t r = 0; r < kLightRows; ++r) {
                const uint32_t ry = r % kLightSide, rz = r / kLightSide;
                uint64_t found = 0;
                if (in_box(r)) {
                    const uint64_t around = light_spread(cur[r], ry > 0 ? cur[r - 1] : 0u, ry + 1u < box.size[1] ? cur[r + 1] : 0u, rz > 0 ? cur[r - kLightSide] : 0u,
                                                         rz + 1u < box.size[2] ? cur[r + kLightSide] : 0u);
                    found = light_step(around, loaded[r].passable, sources ? light_equal(v[r], level) : 0u, reached[r]);
                }
                next[r] = found;
                reached[r] |= found;
                light_set(v[r], found, level);
                any |= found | (sources ? light_any(v[r]) & ~reached[r] : 0u);  // (a source of a lower level is still to come)
            }
            if (!any) break;
        }
    };
    if (sky_wanted) {
        // exposure above the box, a column at a time (the kernel: a wave takes a z, a lane an x, the word by a ballot), then inside it
        for (uint32_t rz = 0; rz < box.size[2]; ++rz) {
            open[rz] = 0;
            for (uint32_t rx = 0; rx < box.size[0]; ++rx) {
                uint32_t trips = 0;
                open[rz] |= column_open<FMT>(w, props, props_count, box.lo[0] + rx, box.lo[2] + rz, box.top, trips) ? uint64_t(1) << rx : 0u;
            }
        }
        for (uint32_t rz = 0; rz < box.size[2]; ++rz) {  // the slab walk
            uint64_t e = open[rz];
            for (uint32_t ry = box.size[1]; ry-- > 0;) {
                e &= loaded[light_row_of(ry, rz)].passable;
                frontier[0][light_row_of(ry, rz)] = e;
            }
        }
        for (uint32_t r = 0; r < kLightRows; ++r) {
            reached[r] = in_box(r) ? frontier[0][r] : 0u;
            light_set(sky[r], reached[r], kLightTop);
            if (in_box(r) && r % kLightSide + 1u == box.size[1]) acc.open_columns += popc64(reached[r]);
        }
        spread(sky, false);
    }
    if (block_wanted) {
        for (uint32_t r = 0; r < kLightRows; ++r) {
            for (uint32_t e = 0; e < 4; ++e) block[r].plane[e] = loaded[r].emit[e];
            acc.sources += popc64(light_any(block[r]));
            reached[r] = frontier[0][r] = light_equal(block[r], kLightTop);
        }
        spread(block, true);
    }
    for (uint32_t r = 0; r < kLightRows; ++r) light_fold_row(acc, box.size, r % kLightSide, r / kLightSide, sky[r], block[r]);
    if (info) *info = light_record(acc);
    if (field) {
        const uint32_t voxels = light_voxels(box.size), padded = light_round16(voxels);
        for (uint32_t rz = 0; rz < box.size[2]; ++rz)
            for (uint32_t ry = 0; ry < box.size[1]; ++ry)
                for (uint32_t rx = 0; rx < box.size[0]; ++rx)
                    field[light_field_row(box.size, ry, rz) + rx] = light_byte(sky[light_row_of(ry, rz)], block[light_row_of(ry, rz)], rx);
        for (uint32_t at = voxels; at < padded; ++at) field[at] = 0;
    }
}

// the whole of vx_light_boxes on one thread (the host test harness). field_stride: as the call takes it (0: the voxel count rounded up to 16)
template <int FMT, class W>
inline void light_boxes(const W& w, const uint8_t* lo, uint32_t lo_stride, uint32_t count, const vx_light_shape& s, uint8_t* fields, uint32_t field_stride,
                        vx_light_info* info) {
    const uint32_t stride = field_stride ? field_stride : light_round16(light_voxels(s.size));
    for (uint32_t n = 0; n < count; ++n) {
        int32_t at[3];
        __builtin_memcpy(at, lo + size_t(n) * lo_stride, 12);
        light_query<FMT>(w, at, s, fields ? fields + size_t(n) * stride : nullptr, info ? info + n : nullptr);
    }
}

// the rules of the call that need no device: what is wrong, naming the field, or null. (Alignment of device memory: blocks_runtime.cpp.)
inline const char* check_light(const void* lo, uint32_t lo_stride, uint32_t count, const vx_light_shape* s, const void* fields, uint32_t field_stride,
                               const void* info) {
    if (count == 0) return nullptr;  // nothing is read or written: nothing to refuse
    if (count > kMaxCount) return "count exceeds 16777216 (2^24)";
    if (!s) return "null shape";
    if (const char* what = lo_rule(lo, lo_stride, fields || info ? nullptr : "fields and info are both null")) return what;
    if (const char* what = size_rule(s->size, kLightSide, "size: every component must be 1..48")) return what;
    if (s->flags & ~uint32_t(VX_LIGHT_NO_SKY | VX_LIGHT_NO_BLOCKS)) return "flags holds a bit other than VX_LIGHT_NO_SKY and VX_LIGHT_NO_BLOCKS";
    if (s->flags == uint32_t(VX_LIGHT_NO_SKY | VX_LIGHT_NO_BLOCKS)) return "flags: VX_LIGHT_NO_SKY and VX_LIGHT_NO_BLOCKS together leave nothing to do";
    if (s->props_count > VX_LIGHT_MAX_PROPS) return "props_count exceeds VX_LIGHT_MAX_PROPS (4096)";
    if (s->props_count && !s->props) return "null props with props_count > 0";
    for (uint32_t k = 0; k < s->props_count; ++k)
        if (s->props[k] & 0xE0u) return "props: a byte has one of bits 5..7 set";
    const uint32_t voxels = light_voxels(s->size);
    if (fields) return field_stride_rule(count, field_stride, voxels, light_round16(voxels), "field_stride must be 0, or a multiple of 16 and at least size.x * size.y * size.z");
    return nullptr;
}

}  // namespace vxb

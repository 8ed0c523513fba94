// The first block along an axis (vx_scan_points, vx_scan_columns; include/voxel_hip.h): the reference's get_block(floor(pos))
// (gameplay.rs:161-201) looped along an axis, as vx_blocks.hpp's descent walked along a line through the world's OWN bytes. A descent that
// ends in air ends at an empty cell of side 2^L, and the walk goes on at the first coordinate beyond that cell: a scan from the top of a
// depth-14 world takes a few dozen descents, not 16,384. Integer-only and exact like the lookup it is built on; a voxel outside
// [0, 2^depth)^3 is air.
//   one column a lane (scan_point, scan_line: vx_scan_points' kernel)   every trip descends from the root to the current voxel.
//   a tile of 8 x 8 columns a wave (ColumnTile, tile_*: vx_scan_columns' kernel)   the tile is aligned to the world grid; the wave walks the
//       bricks of the grid along the axis. The descent to a brick hangs on wave-uniform values alone; where it ends above the brick the whole
//       wave steps over the empty cell, or every open lane answers with the LOD voxel; else each open lane runs the last three levels for its
//       eight voxels along the axis (vx_blocks.hpp's brick_column_along).
// scan_points and scan_columns run whole calls on one thread, lane by lane and tile by tile (the host test harness), and count loop trips.
// The reader W is vx_blocks.hpp's. The standard library and voxel_hip.h only -- no HIP header, no HIP call.
#pragma once

#include "vx_blocks.hpp"

namespace vxb {

constexpr uint32_t kTile = 8;  // vx_scan_columns: a wave's share is 8 x 8 columns aligned to the world grid

VXB_FN vx_scan_hit scan_none(uint32_t cell_log2 = 0u) {
    vx_scan_hit h = {VX_SCAN_NONE, 0u, cell_log2, 0u};
    return h;
}

// floor(p) saturated to int32; p is finite. (Compared before it is converted: a float beyond int32 has no defined conversion.)
VXB_FN int32_t floor_saturated(float p) {
    if (p >= 2147483648.0f) return 2147483647;
    if (p < -2147483648.0f) return -2147483647 - 1;
    const int32_t t = int32_t(p);  // towards zero
    return float(t) > p ? t - 1 : t;
}
VXB_FN bool is_finite(float p) { return p - p == 0.0f; }  // (inf - inf and NaN - NaN are NaN)

// The scan of one column whose (u, v) lie in the world, over the coordinates [first, last] of the axis, 0 <= first <= last < 2^depth, in
// travel order. Every trip descends from the root to the voxel at `c`: a value answers; air is an empty cell of side 2^L, and the next trip
// starts beyond it -- by at least one voxel, so the loop ends.
template <int FMT, class W>
VXB_FN vx_scan_hit scan_line(const W& w, uint32_t axis, bool positive, uint32_t u, uint32_t v, uint32_t first, uint32_t last, uint32_t& trips) {
    const Cursor top = root<FMT>(w);
    uint32_t c = positive ? first : last;
    for (;;) {
        uint32_t x, y, z;
        column_xyz(axis, u, v, c, x, y, z);
        Cursor at = top;
        descend<FMT>(w, at, x, y, z, 0);
        trips += 1;
        if (at.value) {
            vx_scan_hit h = {int32_t(c), at.value, at.level, 0u};
            return h;
        }
        const uint32_t cell = low_bits(int(at.level));
        if (positive) {
            if ((c | cell) >= last) return scan_none();
            c = (c | cell) + 1u;
        } else {
            if ((c & ~cell) <= first) return scan_none();
            c = (c & ~cell) - 1u;
        }
    }
}

// the part of the true range [a0, a1] of an axis that lies in the world, as [first, last]; false: none
VXB_FN bool clip_to_world(int64_t a0, int64_t a1, uint32_t depth, uint32_t& first, uint32_t& last) {
    const int64_t edge = int64_t(1) << depth;
    const int64_t f = a0 < 0 ? 0 : a0, l = a1 >= edge ? edge - 1 : a1;
    first = uint32_t(f);
    last = uint32_t(l);
    return f <= l;
}

// vx_scan_points for one position
template <int FMT, class W>
VXB_FN vx_scan_hit scan_point(const W& w, const float p[3], uint32_t direction, uint32_t reach, uint32_t& trips) {
    if (!(is_finite(p[0]) && is_finite(p[1]) && is_finite(p[2]))) return scan_none(VX_CELL_OUTSIDE);
    const int32_t sx = floor_saturated(p[0]), sy = floor_saturated(p[1]), sz = floor_saturated(p[2]);
    const uint32_t axis = direction >> 1;
    const bool positive = (direction & 1u) != 0;
    const int32_t a = axis == 0 ? sx : (axis == 1 ? sy : sz), u = axis == 0 ? sy : sx, v = axis == 2 ? sy : sz;
    const uint32_t depth = depth_of(w.head());
    // (a negative u or v is a large uint32) the column lies beside the world: no block, no load beyond the head
    if (uint32_t(u) >> depth || uint32_t(v) >> depth) return scan_none();
    // `reach` voxels from the start, in 64 bits (VX_SCAN_TO_EDGE from any int32 start ends beyond every world's far edge)
    const int64_t more = int64_t(reach) - 1;
    uint32_t first, last;
    if (!clip_to_world(positive ? int64_t(a) : int64_t(a) - more, positive ? int64_t(a) + more : int64_t(a), depth, first, last)) return scan_none();
    return scan_line<FMT>(w, axis, positive, uint32_t(u), uint32_t(v), first, last, trips);
}

// vx_scan_columns' share of work: the tiles of 8 x 8 columns aligned to the world grid that the box's footprint touches, numbered u
// fastest. Coordinates of u and v are kept modulo 2^32, as vx_blocks.hpp's Region keeps them (a side of the footprint is at most 2^24).
struct Columns {
    uint32_t lo[3], size[3];      // the box (lo: the int32's bits)
    uint32_t axis, positive;      // of the direction
    uint32_t u, v;                // the two other axes, u < v
    uint32_t lo_u, lo_v, size_u, size_v;  // the footprint (picked here: a kernel indexes no argument by a variable)
    uint32_t first[2], count[2];  // the tiles over (u, v): the first one's corner (a multiple of 8, modulo 2^32), how many along u and v
    int64_t a0, a1;               // the box's extent along the axis, [a0, a1], as it is
};

inline Columns plan_columns(const int32_t lo[3], const uint32_t size[3], int direction) {
    Columns p = {};
    p.axis = uint32_t(direction) >> 1;
    p.positive = uint32_t(direction) & 1u;
    p.u = p.axis == 0 ? 1u : 0u;
    p.v = p.axis == 2 ? 1u : 2u;
    for (int a = 0; a < 3; ++a) {
        p.lo[a] = uint32_t(lo[a]);
        p.size[a] = size[a];
    }
    const uint32_t uv[2] = {p.u, p.v};
    for (int k = 0; k < 2; ++k) {
        const int64_t l = int64_t(lo[uv[k]]), t0 = l >> kBrickLog2, t1 = (l + int64_t(size[uv[k]]) - 1) >> kBrickLog2;  // (floor: arithmetic shifts)
        p.first[k] = uint32_t(t0 * int64_t(kTile));
        p.count[k] = size[uv[k]] ? uint32_t(t1 - t0 + 1) : 0u;
    }
    p.lo_u = p.lo[p.u], p.lo_v = p.lo[p.v], p.size_u = size[p.u], p.size_v = size[p.v];
    p.a0 = int64_t(lo[p.axis]);
    p.a1 = int64_t(lo[p.axis]) + int64_t(size[p.axis]) - 1;
    return p;
}
inline uint64_t column_tiles(const Columns& p) { return p.size[p.axis] ? uint64_t(p.count[0]) * p.count[1] : 0u; }

// A tile, for its wave: everything here hangs on the tile's number and the call's arguments alone.
struct ColumnTile {
    uint32_t cu, cv;        // its corner in (u, v), modulo 2^32
    uint32_t depth;         // of the world
    uint32_t first, last;   // the box's extent along the axis inside the world
    uint32_t walk;          // there is something to walk: the tile lies in the world (whole tiles do or do not, from depth 3 on) and the
                            // extent is not empty
    uint32_t small;         // a world smaller than a brick: every lane scans its own column (scan_line), those that lie in it
};

template <class W>
VXB_FN ColumnTile enter_tile(const W& w, const Columns& p, uint32_t tile) {
    ColumnTile t;
    t.cu = p.first[0] + (tile % p.count[0]) * kTile;
    t.cv = p.first[1] + (tile / p.count[0]) * kTile;
    t.depth = depth_of(w.head());
    const bool some = clip_to_world(p.a0, p.a1, t.depth, t.first, t.last);
    t.small = t.depth < kBrickLog2 ? 1u : 0u;
    t.walk = (some && !(t.cu >> t.depth) && !(t.cv >> t.depth)) ? 1u : 0u;
    return t;
}

// Where in `out` the record of the tile's column (i, j) belongs; false: the column lies outside the box.
VXB_FN bool column_index(const Columns& p, const ColumnTile& t, uint32_t i, uint32_t j, uint32_t& index) {
    const uint32_t ru = t.cu + i - p.lo_u, rv = t.cv + j - p.lo_v;
    index = rv * p.size_u + ru;
    return ru < p.size_u && rv < p.size_v;
}

// the brick of the tile that holds coordinate c of the axis (wave-uniform)
template <int FMT, class W>
VXB_FN Brick tile_brick(const W& w, const Columns& p, const ColumnTile& t, uint32_t c) {
    uint32_t x, y, z;
    column_xyz(p.axis, t.cu, t.cv, c & ~(kBrick - 1u), x, y, z);
    return enter_brick_at<FMT>(w, x, y, z);
}

// One trip of an open lane, column (i, j) of the tile, the walk standing at c in brick b: true when the lane has its answer.
//   the descent ended above the brick in air: nothing, with no load (the wave steps over the cell: tile_advance);
//   it ended above the brick in a value, a LOD voxel of 8 and more: c is the first coordinate of that cell in the lane's range;
//   else the lane's eight voxels along the axis: the first in travel order, from c on and inside the extent, that holds a block.
template <int FMT, class W>
VXB_FN bool tile_lane(const W& w, const Columns& p, const ColumnTile& t, const Brick& b, uint32_t c, uint32_t i, uint32_t j, vx_scan_hit& hit) {
    if (b.at.done) {  // (wave-uniform)
        if (!b.at.value) return false;
        hit.coord = int32_t(c);
        hit.value = b.at.value;
        hit.cell_log2 = b.at.level;
        return true;
    }
    uint32_t value[kBrick], level[kBrick];
    brick_column_along<FMT, true>(w, b, p.axis, i, j, value, level);
    const uint32_t base = c & ~(kBrick - 1u), from = p.positive ? c : t.first, to = p.positive ? t.last : c;
    bool found = false;
    for (uint32_t k = 0; k < kBrick; ++k) {
        // (the first match going up, the last one going down: constant indices, so that the arrays stay in registers)
        const bool match = value[k] != 0 && base + k >= from && base + k <= to && (!found || !p.positive);
        hit.coord = match ? int32_t(base + k) : hit.coord;
        hit.value = match ? value[k] : hit.value;
        hit.cell_log2 = match ? level[k] : hit.cell_log2;
        found = found || match;
    }
    return found;
}

// the walk's next coordinate: beyond the empty cell the brick's descent ended at, or beyond the brick; false: the extent is used up
VXB_FN bool tile_advance(const Columns& p, const ColumnTile& t, const Brick& b, uint32_t& c) {
    const uint32_t cell = low_bits(int(b.at.level > kBrickLog2 ? b.at.level : kBrickLog2));
    if (p.positive) {
        if ((c | cell) >= t.last) return false;
        c = (c | cell) + 1u;
    } else {
        if ((c & ~cell) <= t.first) return false;
        c = (c & ~cell) - 1u;
    }
    return true;
}

// a lane of a tile in a world smaller than a brick
template <int FMT, class W>
VXB_FN vx_scan_hit tile_lane_small(const W& w, const Columns& p, const ColumnTile& t, uint32_t i, uint32_t j, uint32_t& trips) {
    const uint32_t u = t.cu + i, v = t.cv + j;
    if (!t.walk || u >> t.depth || v >> t.depth) return scan_none();
    return scan_line<FMT>(w, p.axis, p.positive != 0, u, v, t.first, t.last, trips);
}

// the whole of vx_scan_points on one thread (the host test harness); trips[i]: the loop trips of point i
template <int FMT, class W>
inline void scan_points(const W& w, const uint8_t* pos, uint32_t pos_stride, uint32_t count, int direction, uint32_t reach, vx_scan_hit* out, uint32_t* trips) {
    for (uint32_t n = 0; n < count; ++n) {
        float p[3];
        __builtin_memcpy(p, pos + uint64_t(n) * pos_stride, 12);
        uint32_t t = 0;
        out[n] = scan_point<FMT>(w, p, uint32_t(direction), reach, t);
        if (trips) trips[n] = t;
    }
}

// the whole of vx_scan_columns on one thread: what the kernel's lanes do, tile by tile (the host test harness); trips[tile]: the wave's loop
// trips (in a world smaller than a brick: the most any of its lanes took)
template <int FMT, class W>
inline void scan_columns(const W& w, const int32_t lo[3], const uint32_t size[3], int direction, vx_scan_hit* out, uint32_t* trips) {
    const Columns p = plan_columns(lo, size, direction);
    const uint64_t tiles = column_tiles(p);
    for (uint64_t n = 0; n < tiles; ++n) {
        const ColumnTile t = enter_tile(w, p, uint32_t(n));
        vx_scan_hit hit[kTile * kTile];
        bool open[kTile * kTile];
        uint32_t most = 0;
        for (uint32_t lane = 0; lane < kTile * kTile; ++lane) {
            hit[lane] = scan_none();
            open[lane] = t.walk && !t.small;
            if (t.small) {
                uint32_t own = 0;
                hit[lane] = tile_lane_small<FMT>(w, p, t, lane & 7u, lane >> 3, own);
                most = own > most ? own : most;
            }
        }
        if (t.walk && !t.small) {
            uint32_t c = p.positive ? t.first : t.last;
            for (;;) {
                const Brick b = tile_brick<FMT>(w, p, t, c);
                most += 1;
                bool any = false;
                for (uint32_t lane = 0; lane < kTile * kTile; ++lane) {
                    if (open[lane]) open[lane] = !tile_lane<FMT>(w, p, t, b, c, lane & 7u, lane >> 3, hit[lane]);
                    any = any || open[lane];
                }
                if (!any || !tile_advance(p, t, b, c)) break;
            }
        }
        for (uint32_t lane = 0; lane < kTile * kTile; ++lane) {
            uint32_t index;
            if (column_index(p, t, lane & 7u, lane >> 3, index)) out[index] = hit[lane];
        }
        if (trips) trips[n] = most;
    }
}

// the rules of both calls that need no device: what is wrong, naming the field, or null
inline const char* check_scan_points(const void* pos, uint32_t pos_stride, uint32_t count, int direction, uint32_t reach, const void* out) {
    if (direction < 0 || direction > 5) return "direction is none of VX_DIR_* (0..5)";
    if (count == 0) return nullptr;  // nothing is read or written: nothing more to refuse
    if (const char* what = check_points(pos, pos_stride, count, out)) return what;
    if (reach == 0) return "reach must be at least 1 (the start voxel counts)";
    return nullptr;
}
inline const char* check_scan_columns(const int32_t* lo, const uint32_t* size, int direction) {
    if (!lo) return "null lo";
    if (!size) return "null size";
    if (direction < 0 || direction > 5) return "direction is none of VX_DIR_* (0..5)";
    if (!size[0] || !size[1] || !size[2]) return nullptr;  // a box with no voxel: nothing to do
    const int a = direction >> 1, u = a == 0 ? 1 : 0, v = a == 2 ? 1 : 2;
    if (uint64_t(size[u]) * size[v] > kMaxCount) return "size: the footprint across the scan axis exceeds 16777216 (2^24) columns";
    if (size[a] > kMaxCount) return "size: the extent along the scan axis exceeds 16777216 (2^24) voxels";
    return nullptr;
}

}  // namespace vxb

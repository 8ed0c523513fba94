// Which block is at a position (vx_block_points, vx_read_region; include/voxel_hip.h): the descent of a point from the root through the
// world's OWN bytes, one level per bit of floor(p) -- the reference's get_block(floor(pos)) (gameplay.rs:161-201) asked of the serialized
// world instead of the host's. ESVO: the child descriptor words an octant holds (esvo.rs:74-101), what get_octant_ptr reads
// (svo.esvo.glsl:168-173, 283-290); CSVO: read_next_ptr and read_leaf (svo.csvo.glsl:53-133) across the chunk boundary with its material
// section. A pure lookup: no ray, none of a ray's start-inside-a-voxel quirks.
//
// The bytes come through a reader W the caller supplies (the kernels: buffer resources, kernels_blocks.hip; the host test harness: a
// byte vector, tests/cpp/blocks_on_host.cpp), every read of which beyond the world gives 0:
//   uint32_t W::head() const              the world's first dword: the bits of octree_scale = 2^-depth
//   uint32_t W::word(uint32_t i) const    ESVO: descriptors[i]              (the dword at byte 4 + 4 i)
//   uint32_t W::root_ptr() const          CSVO: the dword at byte 4 (svo.csvo.glsl:1-5)
//   uint32_t W::c32(uint32_t p) const     CSVO: the dword at descriptor byte p (byte 8 + p, any alignment)
//   uint32_t W::c8(uint32_t p) const      CSVO: the byte there
// The standard library and voxel_hip.h only -- no HIP header, no HIP call.
#pragma once

#include <cstdint>

#include "voxel_hip.h"
#include "vx_rules.hpp"

#if defined(__HIPCC__)
#define VXB_FN __host__ __device__ __forceinline__  // (a call would put its pointer arguments -- a position, a cursor -- into scratch)
#else
#define VXB_FN inline
#endif

namespace vxb {

constexpr int kEsvo = 0, kCsvo = 1;  // the two node formats (VX_SVO_ESVO_BIG is kEsvo through a reader with 64-bit addresses)
constexpr uint32_t kMaxDepth = 23;   // svo.esvo.glsl:21: no world is deeper
constexpr uint32_t kBrickLog2 = 3, kBrick = 8;  // vx_read_region: a workgroup's share is a cube of 8 x 8 x 8 voxels aligned to the world grid
constexpr uint32_t kMaxCount = 1u << 24;        // points of a call, voxels of a region

// the levels of the world, read off octree_scale's exponent (svo.csvo.glsl:254 does the same)
VXB_FN uint32_t depth_of(uint32_t head) {
    const uint32_t d = 127u - ((head >> 23) & 0xffu);
    return d <= kMaxDepth ? d : (d > 127u ? 0u : kMaxDepth);
}

VXB_FN uint32_t popc(uint32_t v) { return uint32_t(__builtin_popcount(v)); }
// (vx_device.hpp's low_bits, a second time: that file needs HIP)
VXB_FN uint32_t low_bits(int n) { return n >= 32 ? 0xffffffffu : (n <= 0 ? 0u : ((1u << n) - 1u)); }
// bytes taken by the pointer-table entries a 2-bit-per-child mask selects: tag 0,1,2,3 -> 0,1,2,4 bytes (vx_device.hpp's csvo_tag_bytes)
VXB_FN uint32_t tag_bytes(uint32_t m) { return popc(m & 0x5555u) + 2u * popc(m & 0xAAAAu) + popc(m & (m >> 1) & 0x5555u); }

// Where a descent stands: at a node whose cell is the cube of side 2^level that holds the point, or at its end.
struct Cursor {
    uint32_t level;     // log2 of the cell: of the node the cursor is at, or -- done -- of the leaf or the empty cell that answers
    uint32_t done;      // the descent has ended; `value` is the answer (0 = no block)
    uint32_t value;
    uint32_t ptr;       // ESVO: index of the node's own octant in descriptors[]; CSVO: the node's byte pointer
    uint32_t node;      // ESVO: child_mask << 8 | leaf_mask; CSVO: the header as 2 bits a child (1-bit headers spread to tag 01)
    uint32_t depth;     // CSVO: levels of nodes from here down (svo.csvo.glsl:254); a chunk at a lower LOD has fewer than its cell has bits
    uint32_t materials, pre_leaf;  // CSVO: the chunk's material section, the depth-2 node above (read_leaf's arguments)
};

// CSVO: the header of the node at p with `depth` levels below it, as 2 bits a child (vx_device.hpp's Trav::csvo_header)
template <class W>
VXB_FN uint32_t csvo_header(const W& w, uint32_t p, uint32_t depth) {
    const uint32_t raw = w.c32(p);
    uint32_t x = raw & 0xffu;
    x = (x | (x << 4)) & 0x0f0fu;
    x = (x | (x << 2)) & 0x3333u;
    x = (x | (x << 1)) & 0x5555u;
    return depth > 3 ? raw & 0xffffu : x;
}

// the cursor at the root: the whole world, [0, 2^depth)^3
template <int FMT, class W>
VXB_FN Cursor root(const W& w) {
    Cursor c = {};
    c.level = depth_of(w.head());
    if (FMT == kCsvo) {
        c.ptr = w.root_ptr();
        c.depth = c.level;
        c.node = csvo_header(w, c.ptr, c.depth);
        c.materials = c.pre_leaf = 0xffffffffu;
        if (c.depth == 2) c.pre_leaf = c.ptr;
    } else {
        // the preamble is an octant whose only child is the root (esvo.rs:179-188)
        c.node = w.word(0) & 0xffffu;
        const uint32_t p = w.word(4);
        c.ptr = (p & 0x80000000u) ? 4u + (p & 0x7fffffffu) : p;
    }
    return c;
}

// one level down, into child idx = x | y << 1 | z << 2 of the node the cursor is at
template <int FMT, class W>
VXB_FN void step(const W& w, Cursor& c, uint32_t idx) {
    c.level -= 1;
    if (FMT == kEsvo) {
        // both words of the child, asked for whether it exists or not (any address reads 0 or a word of the world): no branch, so the
        // steps of several cursors of one lane run side by side (brick_column)
        const uint32_t body = w.word(c.ptr + 4 + idx), masks = w.word(c.ptr + (idx >> 1));
        const bool child = ((c.node >> (8 + idx)) & 1u) != 0, leaf = ((c.node >> idx) & 1u) != 0;
        c.done = (!child || leaf) ? 1u : 0u;
        c.value = (child && leaf) ? body : 0u;
        c.node = ((idx & 1u) ? masks >> 16 : masks) & 0xffffu;
        c.ptr = (body & 0x80000000u) ? c.ptr + 4 + idx + (body & 0x7fffffffu) : body;
        return;
    }
    // (CSVO: worked out in locals and written to the cursor once, at the end: assignments to its fields under different conditions make the
    // compiler keep it in memory)
    const uint32_t tag = (c.node >> (idx * 2)) & 3u;
    uint32_t done = 0, value = 0, ptr = c.ptr, node = c.node, depth = c.depth, materials = c.materials, pre_leaf = c.pre_leaf;
    if (!tag || depth < 2) {
        done = 1;
        if (tag) {
            // read_leaf (svo.csvo.glsl:119-133; vx_device.hpp's csvo_read_leaf_at is its twin: change both): the block ids of a depth-2 node's leaves lie in the material section in the order of their bits
            const uint32_t section_offset = w.c32(pre_leaf + 1) & 0xffffu;
            const int bit_mark = int(ptr - (pre_leaf + 3)) * 8 + int(idx);
            const uint32_t v0 = w.c32(pre_leaf + 3) & low_bits(bit_mark < 32 ? bit_mark : 32);
            const uint32_t v1 = w.c32(pre_leaf + 7) & low_bits(bit_mark - 32 > 0 ? bit_mark - 32 : 0);
            value = w.c32(materials + section_offset * 4 + (popc(v0) + popc(v1)) * 4);
        }
    } else {
        // read_next_ptr (svo.csvo.glsl:53-116) on the normalised header, as the PUSH of vx_device.hpp's Trav::step_with reads it (its twin:
        // change both): the two lowest levels have no table
        const uint32_t offset = tag_bytes(node & ((1u << (idx * 2)) - 1u));
        uint32_t next = ptr + 3 + offset;
        bool crossed = false;
        if (depth >= 3) {
            const uint32_t table = ptr + (depth > 3 ? 2u : 1u);
            // an entry of 1, 2 or 4 bytes by its tag (a shift, not a table of masks: the compiler would keep one in scratch)
            const uint32_t e = w.c32(table + offset) & (0xffffffffu >> ((0x001018u >> ((tag - 1) * 8)) & 0xffu));
            crossed = (e & 0x80000000u) != 0;
            next = crossed ? e ^ 0x80000000u : table + tag_bytes(node) + e;
        }
        depth -= 1;
        ptr = next;
        if (crossed) {  // into a chunk: [lod:u8][material_bytes:u32][materials][nodes] (csvo.rs:217-227)
            const uint32_t child_lod = w.c8(next), material_bytes = w.c32(next + 1);
            materials = next + 5;
            ptr = next + 5 + material_bytes;
            depth = child_lod;
        }
        node = csvo_header(w, ptr, depth);
        pre_leaf = depth == 2 ? ptr : pre_leaf;
    }
    c.done = done; c.value = value; c.ptr = ptr; c.node = node; c.depth = depth; c.materials = materials; c.pre_leaf = pre_leaf;
}

// down to cells of side 2^stop around the voxel (x, y, z) of the world, or to the descent's end. A node that is still no leaf at a single
// voxel (no serializer writes one) ends as no block.
template <int FMT, class W>
VXB_FN void descend(const W& w, Cursor& c, uint32_t x, uint32_t y, uint32_t z, uint32_t stop) {
    while (!c.done && c.level > stop) {
        const uint32_t b = c.level - 1;
        step<FMT>(w, c, ((x >> b) & 1u) | (((y >> b) & 1u) << 1) | (((z >> b) & 1u) << 2));
    }
    if (!c.done && c.level == 0) c.done = 1;
}

// vx_block_points for one position
template <int FMT, class W>
VXB_FN vx_block_cell cell_at_point(const W& w, const float p[3]) {
    Cursor c = root<FMT>(w);
    const float size = float(1u << c.level);
    vx_block_cell r = {0u, VX_CELL_OUTSIDE};
    // (NaN fails every comparison; -0.0f >= 0)
    if (!(p[0] >= 0.0f && p[0] < size && p[1] >= 0.0f && p[1] < size && p[2] >= 0.0f && p[2] < size)) return r;
    descend<FMT>(w, c, uint32_t(p[0]), uint32_t(p[1]), uint32_t(p[2]), 0);
    r.value = c.value;
    r.cell_log2 = c.level;
    return r;
}

// vx_read_region's share of work: the bricks of 8^3 voxels aligned to the world grid that the box [lo, lo + size) touches, numbered x fastest.
// Coordinates are kept modulo 2^32: lo is an int32 and the box is at most 2^24 wide, so a wrapped coordinate is below 2^23 exactly when
// the true one lies in [0, 2^23) -- inside a world (the true one is within [-2^31, 2^31 + 2^24), which no multiple of 2^32 maps into it).
struct Region {
    uint32_t lo[3], size[3];     // the box (lo: the int32's bits)
    uint32_t first[3], count[3];  // its bricks: the first one's corner (a multiple of 8, modulo 2^32), how many along each axis
};

inline Region plan_region(const int32_t lo[3], const uint32_t size[3]) {
    Region r = {};
    for (int a = 0; a < 3; ++a) {
        r.lo[a] = uint32_t(lo[a]);
        r.size[a] = size[a];
        const int64_t b0 = int64_t(lo[a]) >> kBrickLog2, b1 = (int64_t(lo[a]) + int64_t(size[a]) - 1) >> kBrickLog2;  // (floor: arithmetic shifts)
        r.first[a] = uint32_t(b0 * int64_t(kBrick));
        r.count[a] = size[a] ? uint32_t(b1 - b0 + 1) : 0u;
    }
    return r;
}
inline uint64_t region_bricks(const Region& r) { return uint64_t(r.count[0]) * r.count[1] * r.count[2]; }

// A brick, for its wave: the descent to the brick's cell, once.
struct Brick {
    uint32_t corner[3];  // modulo 2^32
    uint32_t inside;     // the brick lies in the world (whole bricks do or do not: the world's edge is a multiple of 8 from depth 3 on;
                         // a shallower world is smaller than a brick, and the voxels are tested one by one)
    Cursor at;           // where the descent stands at the brick's cell, or where it ended above it
};

// the brick at `corner`: the descent from the root to its cell, or to where it ends above it
template <int FMT, class W>
VXB_FN Brick enter_brick_at(const W& w, uint32_t cx, uint32_t cy, uint32_t cz) {
    Brick b;
    b.corner[0] = cx;
    b.corner[1] = cy;
    b.corner[2] = cz;
    b.at = root<FMT>(w);
    const uint32_t edge = 1u << b.at.level;
    b.inside = (b.corner[0] < edge && b.corner[1] < edge && b.corner[2] < edge) ? 1u : 0u;
    if (b.inside) descend<FMT>(w, b.at, b.corner[0], b.corner[1], b.corner[2], kBrickLog2);
    return b;
}

template <int FMT, class W>
VXB_FN Brick enter_brick(const W& w, const Region& r, uint32_t brick) {
    const uint32_t bx = brick % r.count[0], byz = brick / r.count[0];
    return enter_brick_at<FMT>(w, r.first[0] + bx * kBrick, r.first[1] + (byz % r.count[1]) * kBrick, r.first[2] + (byz / r.count[1]) * kBrick);
}

// Where in `out` voxel (i, j, k) of the brick, 0..7 each, belongs; false: it lies outside the box.
VXB_FN bool box_index(const Region& r, const Brick& b, uint32_t i, uint32_t j, uint32_t k, uint32_t& index) {
    const uint32_t rx = b.corner[0] + i - r.lo[0], ry = b.corner[1] + j - r.lo[1], rz = b.corner[2] + k - r.lo[2];
    index = (rz * r.size[1] + ry) * r.size[0] + rx;
    return rx < r.size[0] && ry < r.size[1] && rz < r.size[2];
}

// a step of a cursor that may have ended already (it stays as it is then)
template <int FMT, class W>
VXB_FN Cursor step_live(const W& w, const Cursor& c, uint32_t idx) {
    Cursor n = c;
    step<FMT>(w, n, idx);
    return c.done ? c : n;
}

// A column of a brick runs along `axis`; its lane's (i, j) lie on the two other axes u < v in x, y, z order (axis 2: the (x, y) of
// vx_read_region). The child index x | y << 1 | z << 2 of the column's step h along the axis at one level, uv = u's bit | v's bit << 1:
VXB_FN uint32_t column_child(uint32_t axis, uint32_t uv, uint32_t h) {
    const uint32_t below = (1u << axis) - 1u;
    return (uv & below) | (h << axis) | ((uv & ~below) << 1);
}
// ... and the voxel (u, v, a) of such a column as (x, y, z)
VXB_FN void column_xyz(uint32_t axis, uint32_t u, uint32_t v, uint32_t a, uint32_t& x, uint32_t& y, uint32_t& z) {
    x = axis == 0 ? a : u;
    y = axis == 1 ? a : (axis == 0 ? u : v);
    z = axis == 2 ? a : v;
}

// The eight voxels (i, j, 0..7) of the brick, a lane's share: the last three levels of the descent, level by level -- the column's two
// cells of 4, its four cells of 2, its eight voxels: 14 steps, those of a level independent of one another -- or none of it where the
// brick's own descent ended above it (empty space, a LOD voxel of 8 and more, outside the world). KEEP_LEVEL: `level` receives log2 of the
// leaf, or of the empty cell, that answers for each voxel (vx_scan.hpp); without it `level` is not touched.
template <int FMT, bool KEEP_LEVEL, class W>
VXB_FN void brick_column_along(const W& w, const Brick& b, uint32_t axis, uint32_t i, uint32_t j, uint32_t value[kBrick], uint32_t* level) {
    // (wave-uniform: the brick is the wave's) outside the world, or the brick's own descent ended above it: the fill, with no load
    const uint32_t fill = (b.inside && b.at.done) ? b.at.value : 0u;
    for (uint32_t k = 0; k < kBrick; ++k) {
        value[k] = fill;
        if (KEEP_LEVEL) level[k] = b.at.level;
    }
    if (!b.inside || b.at.done) return;
    if (b.at.level < kBrickLog2) {  // a world smaller than a brick: voxel by voxel, those that lie in it
        const uint32_t world = 1u << b.at.level;
        for (uint32_t k = 0; k < kBrick; ++k) {
            uint32_t o[3];
            column_xyz(axis, i, j, k, o[0], o[1], o[2]);
            const uint32_t x = b.corner[0] + o[0], y = b.corner[1] + o[1], z = b.corner[2] + o[2];
            Cursor c = b.at;
            if (x < world && y < world && z < world) descend<FMT>(w, c, x, y, z, 0);
            value[k] = c.value;
            if (KEEP_LEVEL) level[k] = c.level;
        }
        return;
    }
    const uint32_t uv2 = ((i >> 2) & 1u) | (((j >> 2) & 1u) << 1), uv1 = ((i >> 1) & 1u) | (((j >> 1) & 1u) << 1), uv0 = (i & 1u) | ((j & 1u) << 1);
    Cursor c2[2], c1[4];
    for (uint32_t h = 0; h < 2; ++h) c2[h] = step_live<FMT>(w, b.at, column_child(axis, uv2, h));
    for (uint32_t q = 0; q < 4; ++q) c1[q] = step_live<FMT>(w, c2[q >> 1], column_child(axis, uv1, q & 1u));
    for (uint32_t k = 0; k < kBrick; ++k) {
        const Cursor c0 = step_live<FMT>(w, c1[k >> 1], column_child(axis, uv0, k & 1u));
        value[k] = c0.value;  // (no leaf at a single voxel: 0)
        if (KEEP_LEVEL) level[k] = c0.level;
    }
}

// vx_read_region's columns run along z
template <int FMT, class W>
VXB_FN void brick_column(const W& w, const Brick& b, uint32_t i, uint32_t j, uint32_t value[kBrick]) {
    brick_column_along<FMT, false>(w, b, 2u, i, j, value, nullptr);
}

// the whole region on one thread: what the kernel's lanes do, brick by brick (the host test harness)
template <int FMT, class W>
inline void read_region(const W& w, const int32_t lo[3], const uint32_t size[3], uint32_t* out) {
    const Region r = plan_region(lo, size);
    const uint64_t bricks = region_bricks(r);
    for (uint64_t n = 0; n < bricks; ++n) {
        const Brick b = enter_brick<FMT>(w, r, uint32_t(n));
        for (uint32_t lane = 0; lane < kBrick * kBrick; ++lane) {
            uint32_t value[kBrick], index;
            brick_column<FMT>(w, b, lane & 7u, lane >> 3, value);
            for (uint32_t k = 0; k < kBrick; ++k)
                if (box_index(r, b, lane & 7u, lane >> 3, k, index)) out[index] = value[k];
        }
    }
}

// the rules of both calls that need no device: what is wrong, naming the field, or null
inline const char* check_points(const void* pos, uint32_t pos_stride, uint32_t count, const void* out) {
    if (count == 0) return nullptr;  // nothing is read or written: nothing to refuse
    if (count > kMaxCount) return "count exceeds 16777216 (2^24)";
    if (!stride_ok(pos_stride)) return "pos_stride must be a multiple of 4 and >= 12";
    if (!aligned_to_4(pos)) return "pos must be aligned to 4 bytes";
    if (!pos) return "null pos";
    if (!out) return "null out";
    return nullptr;
}
inline const char* check_region(const int32_t* lo, const uint32_t* size) {
    if (!lo) return "null lo";
    if (!size) return "null size";
    const uint64_t xy = uint64_t(size[0]) * size[1];
    if (xy && size[2] && (xy > kMaxCount || xy * size[2] > kMaxCount)) return "size.x * size.y * size.z exceeds 16777216 (2^24) voxels";
    return nullptr;
}

}  // namespace vxb

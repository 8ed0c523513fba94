// What a batch of axis-aligned float boxes holds (vx_overlap_boxes; include/voxel_hip.h): the reference's overlap test of a player's AABB with
// a voxel (gameplay.rs:211-222), asked for every voxel a box covers of the world's OWN bytes through vx_blocks.hpp's descent. The work is
// shared out by BOX: a wave owns a box and walks the bricks of 8 x 8 x 8 voxels its cover touches (at most 9 an axis), x fastest; in a brick
// lane l takes the column (x, y) = (l & 7, l >> 3), eight voxels along z, as vx_read_region's lanes do.
//   the box: mn = origin + offset, mx = mn + extents, one fp32 add each (the order of gameplay.rs:212-217 and of the physics fan). A record is
//   a box when all nine components, mn and mx are finite and every extent is > 0 and <= 64.
//   the cover: per axis the voxels v with v + 1 > mn and v < mx -- floor(mn) .. ceil(mx) - 1 -- cut to the world [0, 2^depth). Compared and
//   clamped in float BEFORE the conversion to an integer: 3e9, -3e9 and 1e30 are valid coordinates, and converting them is not defined.
//   a lane accumulates over all bricks of its box: the count, min and max of x, y, z, and the smallest key (z, y, x relative to the cover's
//   first voxel, 7 bits each) with its value. One fold across the lanes after the last brick (the kernel: shuffles; overlap_boxes here: a
//   loop) gives the record.
// overlap_boxes runs the whole call on one thread, brick by brick as the kernel runs it (the host test harness).
// The reader W is vx_blocks.hpp's. The standard library and voxel_hip.h only -- no HIP header, no HIP call.
#pragma once

#include <cstddef>

#include "vx_list.hpp"

namespace vxb {

constexpr float kBoxMaxExtent = 64.0f;  // a cover is at most 65 voxels wide: 9 bricks an axis
constexpr uint32_t kBoxNoKey = 0xffffffffu;

// (NaN fails the comparison)
VXB_FN bool box_finite(float v) { return __builtin_fabsf(v) <= 3.402823466e38f; }

// The voxels a box covers, [first, last] per axis in SVO coordinates, cut to the world.
struct Cover {
    uint32_t valid;  // the record described a box
    uint32_t some;   // ... and its cover holds a voxel (first <= last on every axis); else first and last are 0
    int32_t first[3], last[3];
};

// one axis of box_cover. false: no voxel. `world`: 2^depth, exact in float
VXB_FN bool cover_axis(float mn, float mx, float world, int32_t& first, int32_t& last) {
    const float lo = __builtin_fmaxf(__builtin_floorf(mn), 0.0f);          // floor(mn), cut to the world's near edge
    const float hi = __builtin_fminf(__builtin_ceilf(mx), world) - 1.0f;   // ceil(mx) - 1, cut to its far edge (world <= 2^23: exact)
    const bool some = lo <= hi;                                            // (then 0 <= lo <= hi < 2^23: the conversions are exact)
    first = some ? int32_t(lo) : 0;
    last = some ? int32_t(hi) : 0;
    return some;
}

// the rule for a box and its cover. origin, offset, extents: the record's vectors; has_offset == false: mn = origin
VXB_FN Cover box_cover(const float origin[3], const float offset[3], const float extents[3], bool has_offset, uint32_t depth) {
    Cover c = {};
    const float world = float(1u << depth);
    bool valid = true, some = true;
    for (int a = 0; a < 3; ++a) {
        const float off = has_offset ? offset[a] : 0.0f;
        const float mn = has_offset ? origin[a] + off : origin[a];
        const float mx = mn + extents[a];
        valid = valid && box_finite(origin[a]) && box_finite(off) && box_finite(extents[a]) && extents[a] > 0.0f && extents[a] <= kBoxMaxExtent &&
                box_finite(mn) && box_finite(mx);
        some = cover_axis(mn, mx, world, c.first[a], c.last[a]) && some;
    }
    c.valid = valid ? 1u : 0u;
    c.some = (valid && some) ? 1u : 0u;
    if (!c.some)
        for (int a = 0; a < 3; ++a) c.first[a] = c.last[a] = 0;
    return c;
}

// the brick range of a cover that holds a voxel: the first brick's corner, and how many bricks along each axis (1..9)
struct BoxBricks {
    uint32_t corner[3], count[3];
};
VXB_FN BoxBricks cover_bricks(const Cover& c) {
    BoxBricks r;
    for (int a = 0; a < 3; ++a) {
        const uint32_t b0 = uint32_t(c.first[a]) >> kBrickLog2, b1 = uint32_t(c.last[a]) >> kBrickLog2;
        r.corner[a] = b0 * kBrick;
        r.count[a] = b1 - b0 + 1u;
    }
    return r;
}

// What a lane has seen of its box so far, and -- folded -- what the box holds.
struct BoxAcc {
    uint32_t count;
    int32_t mn[3], mx[3];  // of the counted voxels
    uint32_t key, value;   // the smallest (z - first.z) << 14 | (y - first.y) << 7 | (x - first.x) of them, and that voxel's value
};
VXB_FN BoxAcc box_acc_none() {
    BoxAcc a;
    a.count = 0;
    for (int k = 0; k < 3; ++k) a.mn[k] = 0x7fffffff, a.mx[k] = -1;
    a.key = kBoxNoKey;
    a.value = 0;
    return a;
}

// the fold of one answer into another (of a lane's into the box's: any order gives the same, a key belongs to one voxel)
VXB_FN void box_fold(BoxAcc& a, const BoxAcc& b) {
    a.count += b.count;
    for (int k = 0; k < 3; ++k) {
        a.mn[k] = b.mn[k] < a.mn[k] ? b.mn[k] : a.mn[k];
        a.mx[k] = b.mx[k] > a.mx[k] ? b.mx[k] : a.mx[k];
    }
    const bool take = b.key < a.key;
    a.value = take ? b.value : a.value;
    a.key = take ? b.key : a.key;
}

VXB_FN bool box_counts(uint32_t value, uint32_t only_value) { return only_value ? value == only_value : value != 0; }

// (wave-uniform) nothing in the brick can count: air, or one leaf above it that only_value refuses
VXB_FN bool box_brick_skipped(const Brick& b, uint32_t only_value) {
    return brick_is_air(b) || (b.at.done && !box_counts(b.at.value, only_value));
}

// What a lane does for one brick of its box: column (i, j) of the brick, the voxels of it that lie in the cover and count, into `acc`. A lane
// whose column lies outside the cover loads nothing; a brick whose descent ended above it (a LOD leaf of side 8 or more) is folded in with
// no load.
template <int FMT, class W>
VXB_FN void box_brick_lane(const W& w, const Cover& c, uint32_t only_value, const Brick& b, uint32_t i, uint32_t j, BoxAcc& acc) {
    const int32_t x = int32_t(b.corner[0] + i), y = int32_t(b.corner[1] + j), z0 = int32_t(b.corner[2]);
    if (x < c.first[0] || x > c.last[0] || y < c.first[1] || y > c.last[1]) return;
    uint32_t value[kBrick];
    if (b.at.done) {
        for (uint32_t k = 0; k < kBrick; ++k) value[k] = b.at.value;
    } else {
        brick_column<FMT>(w, b, i, j, value);
    }
    uint32_t mask = 0, first_value = 0;
    for (uint32_t k = kBrick; k-- > 0;) {  // (downwards: first_value ends as the lowest counted voxel's)
        const int32_t z = z0 + int32_t(k);
        const bool counted = z >= c.first[2] && z <= c.last[2] && box_counts(value[k], only_value);
        mask |= (counted ? 1u : 0u) << k;
        first_value = counted ? value[k] : first_value;
    }
    if (!mask) return;
    const int32_t z_lo = z0 + int32_t(__builtin_ctz(mask)), z_hi = z0 + 31 - int32_t(__builtin_clz(mask));
    BoxAcc mine;
    mine.count = popc(mask);
    mine.mn[0] = mine.mx[0] = x;
    mine.mn[1] = mine.mx[1] = y;
    mine.mn[2] = z_lo;
    mine.mx[2] = z_hi;
    mine.key = (uint32_t(z_lo - c.first[2]) << 14) | (uint32_t(y - c.first[1]) << 7) | uint32_t(x - c.first[0]);
    mine.value = first_value;
    box_fold(acc, mine);
}

VXB_FN vx_box_hit box_invalid() {
    vx_box_hit h = {};
    h.blocks = VX_BOX_INVALID;
    return h;
}

// the record of a box whose lanes' answers have been folded into `a`
VXB_FN vx_box_hit box_record(const BoxAcc& a) {
    vx_box_hit h = {};
    if (a.count == 0) return h;
    h.blocks = a.count;
    h.value = a.value;
    for (int k = 0; k < 3; ++k) h.lo[k] = a.mn[k], h.hi[k] = a.mx[k] + 1;
    return h;
}

// float[3] number i of a strided array (stride 0: the one vector)
inline void box_vector(const void* base, uint32_t stride, uint32_t i, float out[3]) {
    const unsigned char* p = static_cast<const unsigned char*>(base) + size_t(i) * stride;
    __builtin_memcpy(out, p, 12);
}

// the whole call on one thread: what the kernel's waves do, box by box and brick by brick (the host test harness)
template <int FMT, class W>
inline void overlap_boxes(const W& w, const vx_box_batch& boxes, uint32_t count, vx_box_hit* out) {
    const uint32_t depth = depth_of(w.head());
    for (uint32_t n = 0; n < count; ++n) {
        float origin[3], offset[3] = {0.0f, 0.0f, 0.0f}, extents[3];
        box_vector(boxes.origin, boxes.origin_stride, n, origin);
        if (boxes.offset) box_vector(boxes.offset, boxes.offset_stride, n, offset);
        box_vector(boxes.extents, boxes.extents_stride, n, extents);
        const Cover c = box_cover(origin, offset, extents, boxes.offset != nullptr, depth);
        if (!c.valid) {
            out[n] = box_invalid();
            continue;
        }
        BoxAcc lanes[kLanes];
        for (uint32_t lane = 0; lane < kLanes; ++lane) lanes[lane] = box_acc_none();
        if (c.some) {
            const BoxBricks r = cover_bricks(c);
            for (uint32_t bz = 0; bz < r.count[2]; ++bz)
                for (uint32_t by = 0; by < r.count[1]; ++by)
                    for (uint32_t bx = 0; bx < r.count[0]; ++bx) {
                        const Brick b = enter_brick_at<FMT>(w, r.corner[0] + bx * kBrick, r.corner[1] + by * kBrick, r.corner[2] + bz * kBrick);
                        if (box_brick_skipped(b, boxes.only_value)) continue;
                        for (uint32_t lane = 0; lane < kLanes; ++lane) box_brick_lane<FMT>(w, c, boxes.only_value, b, lane & 7u, lane >> 3, lanes[lane]);
                    }
        }
        BoxAcc all = box_acc_none();
        for (uint32_t lane = 0; lane < kLanes; ++lane) box_fold(all, lanes[lane]);
        out[n] = box_record(all);
    }
}

// the rules of the call that need no device: what is wrong, naming the field, or null. (Alignment of device memory: blocks_runtime.cpp.)
inline const char* check_boxes(const vx_box_batch* boxes, uint32_t count, const void* out) {
    if (count == 0) return nullptr;  // nothing is read or written: nothing to refuse
    if (count > kMaxCount) return "count exceeds 16777216 (2^24)";
    if (!boxes) return "null boxes";
    if (!out) return "null out";
    if (!boxes->origin) return "null origin";
    if (!boxes->extents) return "null extents";
    if (!stride_ok(boxes->origin_stride)) return "origin_stride must be a multiple of 4 and >= 12";
    if (boxes->offset && !stride_ok(boxes->offset_stride, true)) return "offset_stride must be 0, or a multiple of 4 and >= 12";
    if (!stride_ok(boxes->extents_stride, true)) return "extents_stride must be 0, or a multiple of 4 and >= 12";
    if (!aligned_to_4(boxes->origin)) return "origin must be aligned to 4 bytes";
    if (!aligned_to_4(boxes->offset)) return "offset must be aligned to 4 bytes";
    if (!aligned_to_4(boxes->extents)) return "extents must be aligned to 4 bytes";
    return nullptr;
}

}  // namespace vxb

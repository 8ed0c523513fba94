// A batch of float boxes moved through the world and stopped by blocks (vx_move_boxes; include/voxel_hip.h): the question the reference
// answers with a fan of picker rays a voxel apart (Aabb::generate_picker_tasks, svo_picker.rs:183-243) and apply_axial_physics
// (physics.rs:171-184), asked of every voxel ahead of the box, axis by axis, each axis from where the earlier ones left the box. The boxes
// are vx_boxes.hpp's, the work is shared out as there: a wave owns a box; per pass it walks the bricks of the swept slab -- the box's
// cross-section times the layers ahead of its leading face -- nearest brick layer first; in a brick lane l takes column (l & 7, l >> 3).
//   a lane keeps ONE key with its value: distance in layers << 14 | in-layer order key (7 bits per cross-section axis: vx_read_region's
//   order, z, then y, then x). The smallest key of the wave is the first counted voxel of the nearest layer; a nearer brick layer cannot be
//   beaten by a farther one, so the walk ends after the first brick layer in which any lane holds a key.
//   everything but four float operations a pass is integer work on vx_boxes.hpp's cover. Those four are written out one by one and built
//   without contraction (-ffp-contract=off), so that the record is the same bytes everywhere.
// The axis of a pass is a run-time value: vectors are read and written through pick3 / put3 (selects), never indexed by it -- an indexed
// register array would live in scratch.
// move_boxes runs the whole call on one thread, brick by brick as the kernel runs it (the host test harness).
// The reader W is vx_blocks.hpp's. The standard library and voxel_hip.h only -- no HIP header, no HIP call.
#pragma once

#include "vx_boxes.hpp"

namespace vxb {

template <class T>
VXB_FN T pick3(const T v[3], uint32_t a) { return a == 0 ? v[0] : (a == 1 ? v[1] : v[2]); }
template <class T>
VXB_FN void put3(T v[3], uint32_t a, T x) {
    v[0] = a == 0 ? x : v[0];
    v[1] = a == 1 ? x : v[1];
    v[2] = a == 2 ? x : v[2];
}

VXB_FN uint32_t move_axis(uint32_t order, uint32_t pass) { return (order >> (2u * pass)) & 3u; }
VXB_FN bool move_order_ok(uint32_t order) {
    const uint32_t a = move_axis(order, 0), b = move_axis(order, 1), c = move_axis(order, 2);
    return !(order & ~0x3fu) && a < 3 && b < 3 && c < 3 && a != b && a != c && b != c;
}

// the displacement d = motion * scale, and whether the record has one: every component of both finite, no |d| above VX_MOVE_MAX_TRAVEL
VXB_FN bool move_displacement(const float motion[3], float scale, float d[3]) {
    bool valid = true;
    for (int a = 0; a < 3; ++a) {
        d[a] = motion[a] * scale;
        valid = valid && box_finite(motion[a]) && __builtin_fabsf(d[a]) <= VX_MOVE_MAX_TRAVEL;  // (NaN and inf fail the comparison)
    }
    return valid;
}

// The slab a pass sweeps, as a cover: on axis `a` the layers ahead of the leading face -- d > 0: ceil(mx) .. ceil(mx + (d + skin)) - 1,
// d < 0: floor(mn + (d - skin)) .. floor(mn) - 1 --, on the two other axes cover_axis' voxels; all cut to the world in float before the
// conversion. some == 0: no voxel (an empty cross-section, or no layer inside the world).
VXB_FN Cover move_slab(const float mn[3], const float mx[3], uint32_t a, float d, float skin, float world) {
    Cover c = {};
    c.valid = 1u;
    bool some = true;
    for (uint32_t k = 0; k < 3; ++k) {
        const bool up = d > 0.0f;
        const float reach = up ? d + skin : d - skin;
        const float end = (up ? mx[k] : mn[k]) + reach;
        // along the travel: from the leading face to `end`; across it: the box's own extent
        const float from = k == a ? (up ? __builtin_ceilf(mx[k]) : __builtin_floorf(end)) : __builtin_floorf(mn[k]);
        const float to = k == a ? (up ? __builtin_ceilf(end) : __builtin_floorf(mn[k])) : __builtin_ceilf(mx[k]);
        const float lo = __builtin_fmaxf(from, 0.0f);
        const float hi = __builtin_fminf(to, world) - 1.0f;  // (to <= world <= 2^23: exact; below 0: whatever, lo > hi)
        const bool any = lo <= hi;                            // (then 0 <= lo <= hi < 2^23: the conversions are exact)
        c.first[k] = any ? int32_t(lo) : 0;
        c.last[k] = any ? int32_t(hi) : 0;
        some = some && any;
    }
    c.some = some ? 1u : 0u;
    return c;
}

// What a lane holds of a pass: the smallest key it has seen, and that voxel's value
struct MoveKey {
    uint32_t key, value;
};
VXB_FN MoveKey move_key_none() { return MoveKey{kBoxNoKey, 0u}; }
VXB_FN void move_fold(MoveKey& a, const MoveKey& b) {  // (a key belongs to one voxel: any order gives the same)
    const bool take = b.key < a.key;
    a.value = take ? b.value : a.value;
    a.key = take ? b.key : a.key;
}

// What a lane does for one brick of a pass: column (i, j) of the brick, the nearest counted voxel of it inside the slab `s`, into `best`.
// A lane whose column lies outside the slab loads nothing; a brick whose descent ended above it (a LOD leaf of side 8 or more) needs none.
template <int FMT, class W>
VXB_FN void move_brick_lane(const W& w, const Cover& s, uint32_t a, bool up, uint32_t only_value, const Brick& b, uint32_t i, uint32_t j, MoveKey& best) {
    const int32_t x = int32_t(b.corner[0] + i), y = int32_t(b.corner[1] + j), z0 = int32_t(b.corner[2]);
    if (x < s.first[0] || x > s.last[0] || y < s.first[1] || y > s.last[1]) return;
    uint32_t value[kBrick];
    if (b.at.done) {
        for (uint32_t k = 0; k < kBrick; ++k) value[k] = b.at.value;
    } else {
        brick_column<FMT>(w, b, i, j, value);
    }
    uint32_t mask = 0, lowest = 0, highest = 0;
    for (uint32_t k = 0; k < kBrick; ++k) {
        const int32_t z = z0 + int32_t(k);
        const bool counted = z >= s.first[2] && z <= s.last[2] && box_counts(value[k], only_value);
        lowest = (counted && !mask) ? value[k] : lowest;
        highest = counted ? value[k] : highest;
        mask |= (counted ? 1u : 0u) << k;
    }
    if (!mask) return;
    // along z the distance falls with z when the box moves down it; in every other case the column's lowest counted voxel has its smallest key
    const bool top = a == 2 && !up;
    const int32_t z = z0 + (top ? 31 - int32_t(__builtin_clz(mask)) : int32_t(__builtin_ctz(mask)));
    const uint32_t rel[3] = {uint32_t(x - s.first[0]), uint32_t(y - s.first[1]), uint32_t(z - s.first[2])};
    const uint32_t span = uint32_t(pick3(s.last, a) - pick3(s.first, a));
    const uint32_t along = pick3(rel, a), dist = up ? along : span - along;
    const uint32_t u = a == 0 ? rel[1] : rel[0], v = a == 2 ? rel[1] : rel[2];  // the two other axes in x, y, z order
    MoveKey mine;
    mine.key = (dist << 14) | (v << 7) | u;
    mine.value = top ? highest : lowest;
    move_fold(best, mine);
}

// the corner of brick (layer, bu, bv) of a pass's slab, the layers counted from the box: r = cover_bricks(slab)
VXB_FN void move_brick_corner(const BoxBricks& r, uint32_t a, bool up, uint32_t layer, uint32_t bu, uint32_t bv, uint32_t& cx, uint32_t& cy, uint32_t& cz) {
    const uint32_t layers = pick3(r.count, a);
    const uint32_t ca = pick3(r.corner, a) + (up ? layer : layers - 1u - layer) * kBrick;
    const uint32_t cu = (a == 0 ? r.corner[1] : r.corner[0]) + bu * kBrick, cv = (a == 2 ? r.corner[1] : r.corner[2]) + bv * kBrick;
    column_xyz(a, cu, cv, ca, cx, cy, cz);
}

// What a pass amounts to, from the wave's smallest key: how far the box moves along the axis, whether something lay ahead, and what
struct MoveStep {
    float m;
    uint32_t found, value;
};
VXB_FN MoveStep move_step(const Cover& s, uint32_t a, float d, float skin, float mn_a, float mx_a, const MoveKey& best) {
    MoveStep r = {d, 0u, 0u};
    if (best.key == kBoxNoKey) return r;
    const bool up = d > 0.0f;
    const int32_t dist = int32_t(best.key >> 14);
    const int32_t v = up ? pick3(s.first, a) + dist : pick3(s.last, a) - dist;
    const float gap = up ? float(v) - mx_a : mn_a - float(v + 1);  // (|v| < 2^23: exact)
    const float room = gap - skin;
    const float most = room > 0.0f ? room : 0.0f;
    const float want = up ? d : -d;
    const float go = most < want ? most : want;
    r.m = up ? go : -go;
    r.found = 1u;
    r.value = best.value;
    return r;
}

VXB_FN vx_move_hit move_invalid() {
    vx_move_hit h = {};
    h.contacts = VX_MOVE_INVALID;
    return h;
}

// A box on its way: the record's vectors, mn and mx as the passes so far left them, and the answer so far
struct MoveBox {
    float origin[3], offset[3], extents[3], mn[3], mx[3], d[3];
    vx_move_hit hit;
};

// the box and its displacement from the record's vectors; false: the record is invalid
VXB_FN bool move_begin(MoveBox& m, const float origin[3], const float offset[3], const float extents[3], bool has_offset, const float motion[3], float scale,
                       uint32_t depth) {
    const bool box = box_cover(origin, offset, extents, has_offset, depth).valid != 0;
    const bool moves = move_displacement(motion, scale, m.d);
    for (int a = 0; a < 3; ++a) {
        m.origin[a] = origin[a];
        m.offset[a] = has_offset ? offset[a] : 0.0f;
        m.extents[a] = extents[a];
        m.mn[a] = has_offset ? origin[a] + offset[a] : origin[a];
        m.mx[a] = m.mn[a] + extents[a];
    }
    m.hit = vx_move_hit{};
    return box && moves;
}

// the end of the pass of axis a: the three adds, and the record's words for that axis
VXB_FN void move_end_pass(MoveBox& m, uint32_t a, bool has_offset, const MoveStep& st) {
    const float d = pick3(m.d, a);
    const float origin = pick3(m.origin, a) + st.m;
    const float mn = has_offset ? origin + pick3(m.offset, a) : origin;
    const float mx = mn + pick3(m.extents, a);
    put3(m.origin, a, origin);
    put3(m.mn, a, mn);
    put3(m.mx, a, mx);
    put3(m.hit.moved, a, st.m);
    put3(m.hit.value, a, st.value);
    m.hit.contacts |= st.found << (2u * a + (d > 0.0f ? 1u : 0u));
}

// the whole call on one thread: what the kernel's waves do, box by box, pass by pass and brick by brick (the host test harness)
template <int FMT, class W>
inline void move_boxes(const W& w, const vx_box_batch& boxes, const void* motion, uint32_t motion_stride, uint32_t count, const vx_move_shape& shape,
                       vx_move_hit* out) {
    const uint32_t depth = depth_of(w.head());
    const float world = float(1u << depth);
    const bool has_offset = boxes.offset != nullptr;
    for (uint32_t n = 0; n < count; ++n) {
        float origin[3], offset[3] = {0.0f, 0.0f, 0.0f}, extents[3], mot[3];
        box_vector(boxes.origin, boxes.origin_stride, n, origin);
        if (has_offset) box_vector(boxes.offset, boxes.offset_stride, n, offset);
        box_vector(boxes.extents, boxes.extents_stride, n, extents);
        box_vector(motion, motion_stride, n, mot);
        MoveBox m;
        if (!move_begin(m, origin, offset, extents, has_offset, mot, shape.scale, depth)) {
            out[n] = move_invalid();
            continue;
        }
        for (uint32_t pass = 0; pass < 3; ++pass) {
            const uint32_t a = move_axis(shape.order, pass);
            const float d = pick3(m.d, a);
            MoveStep st = {0.0f, 0u, 0u};
            if (d != 0.0f) {
                const bool up = d > 0.0f;
                const Cover s = move_slab(m.mn, m.mx, a, d, shape.skin, world);
                MoveKey lanes[kLanes], best = move_key_none();
                for (uint32_t lane = 0; lane < kLanes; ++lane) lanes[lane] = move_key_none();
                if (s.some) {
                    const BoxBricks r = cover_bricks(s);
                    const uint32_t layers = pick3(r.count, a), nu = a == 0 ? r.count[1] : r.count[0], nv = a == 2 ? r.count[1] : r.count[2];
                    for (uint32_t layer = 0; layer < layers; ++layer) {
                        for (uint32_t bv = 0; bv < nv; ++bv)
                            for (uint32_t bu = 0; bu < nu; ++bu) {
                                uint32_t cx, cy, cz;
                                move_brick_corner(r, a, up, layer, bu, bv, cx, cy, cz);
                                const Brick b = enter_brick_at<FMT>(w, cx, cy, cz);
                                if (box_brick_skipped(b, boxes.only_value)) continue;
                                for (uint32_t lane = 0; lane < kLanes; ++lane) move_brick_lane<FMT>(w, s, a, up, boxes.only_value, b, lane & 7u, lane >> 3, lanes[lane]);
                            }
                        bool any = false;  // (the kernel: a ballot)
                        for (uint32_t lane = 0; lane < kLanes; ++lane) any = any || lanes[lane].key != kBoxNoKey;
                        if (any) break;
                    }
                }
                for (uint32_t lane = 0; lane < kLanes; ++lane) move_fold(best, lanes[lane]);
                st = move_step(s, a, d, shape.skin, pick3(m.mn, a), pick3(m.mx, a), best);
            }
            move_end_pass(m, a, has_offset, st);
        }
        for (int a = 0; a < 3; ++a) m.hit.origin[a] = m.origin[a];
        out[n] = m.hit;
    }
}

// the rules of the call that need no device: what is wrong, naming the field, or null. (Alignment of device memory: blocks_runtime.cpp.)
inline const char* check_move(const vx_box_batch* boxes, const void* motion, uint32_t motion_stride, uint32_t count, const vx_move_shape* shape,
                              const void* out) {
    if (!shape) return "null shape";
    if (!box_finite(shape->scale)) return "scale must be finite";
    if (!(shape->skin >= 0.0f && shape->skin <= 1.0f)) return "skin must lie in [0, 1]";
    if (!move_order_ok(shape->order)) return "order must hold a permutation of the axes 0, 1, 2 in bits 0..5 and no other bit";
    if (shape->flags) return "flags must be 0";
    if (count == 0) return nullptr;  // nothing is read or written: nothing more to refuse
    if (const char* what = check_boxes(boxes, count, out)) return what;
    if (!motion) return "null motion";
    if (!stride_ok(motion_stride, true)) return "motion_stride must be 0, or a multiple of 4 and >= 12";
    if (!aligned_to_4(motion)) return "motion must be aligned to 4 bytes";
    return nullptr;
}

}  // namespace vxb

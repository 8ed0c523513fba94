// The squared distance to the nearest block, per cell, in a batch of boxes (vx_distance_boxes; include/voxel_hip.h): the distance transform a
// caller of the reference would run on the host over get_block (gameplay.rs:161-201), asked of the world's OWN bytes. vx_flood.hpp's box,
// brick loading and rows of 32 bits once more; what follows the loading is the exact separable transform, all in integers. A workgroup of 256
// threads owns one box of up to 32 x 32 x 32 cells.
//   rows: the cells (0..size.x, ry, rz) of the box are bit rx of row rz * 32 + ry, as vx_flood.hpp keeps them. Loading is vx_flood.hpp's
//   (FloodBox, enter_brick_at, flood_brick_lane under distance_load_shape); a loaded row holds PASSABLE bits. Without a match_value one load
//   under pass_value gives the targets, ~row & mask. With one, a load under 0 gives the air and a load under match_value the air and the
//   matching cells: the targets are the second without the first. VX_DISTANCE_TO_AIR complements the row within its mask (distance_row).
//   x: the distance along a row is read off its word (distance_row_x): the nearest set bit at or below rx by count-leading-zeros, at or above
//   by count-trailing-zeros, squared; kDistanceNone when the word is 0.
//   y, z: one min-plus pass a line (distance_pass_at, distance_pass), out[i] = min_j(in[j] + (i - j)^2). kDistanceNone + 31^2 fits a uint32 and stays above every
//   real value (at most 3 * 31^2), and the result is cut to kDistanceNone: "none" stays "none".
//   the field's entry of cell (rx, ry, rz) is at (rz * size.y + ry) * size.x + rx, vx_read_region's layout, 16 bits each.
//   the record's fold (DistanceAcc): targets are the cells whose value is 0; faces ORed; "largest value, then first in the field's order" is
//   the maximum of value << 15 | (32767 - entry) (distance_key).
// distance_query runs a whole query on one thread, pass by pass as the kernel's workgroup runs it; distance_boxes the whole call (the host
// test harness). The reader W is vx_blocks.hpp's. The standard library and voxel_hip.h only -- no HIP header, no HIP call.
#pragma once

#include <cstddef>

#include "vx_flood.hpp"

namespace vxb {

constexpr uint32_t kDistanceMaxCount = 1u << 20;  // boxes of a call
constexpr uint32_t kDistanceNone = VX_DISTANCE_NONE;
constexpr uint32_t kDistanceCells = kFloodRows * kFloodSide;  // 32,768: an entry's number has 15 bits

VXB_FN uint32_t distance_voxels(const vx_distance_shape& s) { return s.size[0] * s.size[1] * s.size[2]; }
// the bytes of a query's field that are written: 2 a cell, rounded up to 16
VXB_FN uint32_t distance_field_bytes(const vx_distance_shape& s) { return flood_round16(2u * distance_voxels(s)); }
// (1u << 32 is no mask: the full row is named)
VXB_FN uint32_t distance_row_mask(uint32_t side) { return side >= 32u ? 0xffffffffu : (1u << side) - 1u; }

// a cell's rule
VXB_FN bool distance_target(uint32_t value, const vx_distance_shape& s) {
    const bool is = s.match_value ? value == s.match_value : !flood_passable(value, s.pass_value);
    return (s.flags & VX_DISTANCE_TO_AIR) ? !is : is;
}

// What vx_flood.hpp's loading takes: the box, no seed cell to report, and the value that passes -- pass_value, or for the second load of a
// call with a match_value that value.
VXB_FN vx_flood_shape distance_load_shape(const vx_distance_shape& s, bool second) {
    vx_flood_shape f = {{s.size[0], s.size[1], s.size[2]}, {0u, 0u, 0u}, 0u, second ? s.match_value : s.pass_value, 0u};
    return f;
}
VXB_FN bool distance_loads_twice(const vx_distance_shape& s) { return s.match_value != 0u; }
// The box of a query and the bricks of its cover, modulo 2^32 as vxb::Region keeps a box.
VXB_FN FloodBox distance_box(const int32_t lo[3], const vx_distance_shape& s) {
    FloodBox b;
    for (int a = 0; a < 3; ++a) {
        b.lo[a] = uint32_t(lo[a]);
        b.first[a] = b.lo[a] & ~(kBrick - 1u);
        b.count[a] = ((b.lo[a] & (kBrick - 1u)) + s.size[a] + kBrick - 1u) >> kBrickLog2;
    }
    return b;
}

// A row's target word from what was loaded: `first` under distance_load_shape(s, false), `second` under (s, true) (not read without a
// match_value); masked to size.x, complemented within the mask under VX_DISTANCE_TO_AIR.
VXB_FN uint32_t distance_row(const vx_distance_shape& s, uint32_t first, uint32_t second) {
    const uint32_t mask = distance_row_mask(s.size[0]);
    const uint32_t is = (s.match_value ? second & ~first : ~first) & mask;
    return (s.flags & VX_DISTANCE_TO_AIR) ? ~is & mask : is;
}

// The squared distance along x from cell rx (0..31) to the nearest set bit of `word`; kDistanceNone: the word is 0.
VXB_FN uint32_t distance_row_x(uint32_t word, uint32_t rx) {
    const uint32_t below = word & ((2u << rx) - 1u);  // bits 0..rx (rx == 31: 2u << 31 is 0, the mask all ones)
    const uint32_t above = (word >> rx) << rx;        // bits rx..31
    const uint32_t down = below ? rx - (31u - uint32_t(__builtin_clz(below))) : kFloodSide;
    const uint32_t up = above ? uint32_t(__builtin_ctz(above)) - rx : kFloodSide;
    const uint32_t d = down < up ? down : up;
    return d >= kFloodSide ? kDistanceNone : d * d;
}

// One entry of a min-plus pass over a line: min over j of in[j] + (i - j)^2. `in` has kFloodSide entries; those behind the line's end hold
// kDistanceNone, or a copy of the line's last entry -- farther from every i of the line than that entry itself --, so that no minimum takes
// them and the sums need no bound check. in[j] <= kDistanceNone, so a sum fits; the result is at most kDistanceNone, and is kDistanceNone
// exactly when every in[j] is: "none" stays "none".
VXB_FN uint32_t distance_pass_at(const uint32_t in[kFloodSide], uint32_t i) {
    uint32_t m = kDistanceNone;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (uint32_t j = 0; j < kFloodSide; ++j) {
        const uint32_t d = i > j ? i - j : j - i, v = in[j] + d * d;
        m = v < m ? v : m;
    }
    return m;
}
// The pass over a line of n entries: out[i] for i < n; out[n...] is not written. `in` and `out` are different arrays.
VXB_FN void distance_pass(const uint32_t in[kFloodSide], uint32_t out[kFloodSide], uint32_t n) {
    for (uint32_t i = 0; i < n; ++i) out[i] = distance_pass_at(in, i);
}

VXB_FN uint32_t distance_entry(const vx_distance_shape& s, uint32_t rx, uint32_t ry, uint32_t rz) { return (rz * s.size[1] + ry) * s.size[0] + rx; }
VXB_FN uint32_t distance_pack(uint32_t rx, uint32_t ry, uint32_t rz) { return rx | ry << 8 | rz << 16; }
// the faces of the box cell (rx, ry, rz) lies on
VXB_FN uint32_t distance_cell_faces(const vx_distance_shape& s, uint32_t rx, uint32_t ry, uint32_t rz) {
    return (rx == 0u ? 1u : 0u) | (rx + 1u == s.size[0] ? 2u : 0u) | (ry == 0u ? 4u : 0u) | (ry + 1u == s.size[1] ? 8u : 0u) | (rz == 0u ? 16u : 0u) |
           (rz + 1u == s.size[2] ? 32u : 0u);
}
// "largest value, then first in the field's order" as a plain maximum
VXB_FN uint32_t distance_key(uint32_t value, uint32_t entry) { return value << 15 | (kDistanceCells - 1u - entry); }

// What the final values say of a box: folded cell by cell, then across the threads (a sum, an OR, a maximum: any order gives the same)
struct DistanceAcc {
    uint32_t targets, faces, key;
};
VXB_FN DistanceAcc distance_acc() {
    DistanceAcc a = {0u, 0u, 0u};
    return a;
}
VXB_FN void distance_fold_cell(DistanceAcc& a, const vx_distance_shape& s, uint32_t rx, uint32_t ry, uint32_t rz, uint32_t value) {
    const uint32_t key = distance_key(value, distance_entry(s, rx, ry, rz));
    a.targets += value == 0u ? 1u : 0u;
    a.faces |= value == 0u ? distance_cell_faces(s, rx, ry, rz) : 0u;
    a.key = key > a.key ? key : a.key;
}
VXB_FN void distance_fold(DistanceAcc& a, const DistanceAcc& b) {
    a.targets += b.targets;
    a.faces |= b.faces;
    a.key = b.key > a.key ? b.key : a.key;
}
VXB_FN vx_distance_info distance_record(const DistanceAcc& a, const vx_distance_shape& s) {
    const uint32_t entry = kDistanceCells - 1u - (a.key & (kDistanceCells - 1u)), row = entry / s.size[0];
    vx_distance_info r = {a.targets, a.key >> 15, distance_pack(entry % s.size[0], row % s.size[1], row / s.size[1]), a.faces};
    return r;
}

// A whole query on one thread, as the kernel's workgroup runs it. field: distance_field_bytes(s) / 2 entries, or null; info: a record, or
// null.
template <int FMT, class W>
inline void distance_query(const W& w, const int32_t lo[3], const vx_distance_shape& s, uint16_t* field, vx_distance_info* info) {
    const uint32_t voxels = distance_voxels(s), padded = distance_field_bytes(s) / 2u;
    const vx_flood_shape load[2] = {distance_load_shape(s, false), distance_load_shape(s, true)};
    const FloodBox box = distance_box(lo, s);
    static thread_local uint32_t rows[kFloodRows];
    static thread_local uint16_t dist[kDistanceCells];
    for (uint32_t r = 0; r < kFloodRows; ++r) rows[r] = 0;
    // loading: the brick rows of the cover, one after the other (the kernel: four waves take them in turn)
    for (uint32_t n = 0; n < box.count[1] * box.count[2]; ++n) {
        const uint32_t cy = box.first[1] + (n % box.count[1]) * kBrick, cz = box.first[2] + (n / box.count[1]) * kBrick;
        uint32_t first[kFloodLanes], second[kFloodLanes], unused = 0;
        for (uint32_t lane = 0; lane < kFloodLanes; ++lane) first[lane] = second[lane] = 0;
        for (uint32_t bx = 0; bx < box.count[0]; ++bx) {
            const Brick b = enter_brick_at<FMT>(w, box.first[0] + bx * kBrick, cy, cz);
            for (uint32_t lane = 0; lane < kFloodLanes; ++lane) {
                flood_brick_lane<FMT>(w, load[0], box, b, lane & 7u, lane >> 3, first[lane], unused);
                if (distance_loads_twice(s)) flood_brick_lane<FMT>(w, load[1], box, b, lane & 7u, lane >> 3, second[lane], unused);
            }
        }
        for (uint32_t lane = 0; lane < kFloodLanes; ++lane) {
            const uint32_t ry = cy + (lane & 7u) - box.lo[1], rz = cz + (lane >> 3) - box.lo[2];
            if (ry < s.size[1] && rz < s.size[2]) rows[flood_row_of(ry, rz)] = distance_row(s, first[lane], second[lane]);
        }
    }
    uint32_t in[kFloodSide], out[kFloodSide];
    // pass y: the columns (x, z) along y, x from the rows' bits (the kernel: thread t owns x = t & 31, z = (t >> 5) + 8 k)
    for (uint32_t rz = 0; rz < s.size[2]; ++rz)
        for (uint32_t rx = 0; rx < s.size[0]; ++rx) {
            for (uint32_t ry = 0; ry < kFloodSide; ++ry) in[ry] = ry < s.size[1] ? distance_row_x(rows[flood_row_of(ry, rz)], rx) : kDistanceNone;
            distance_pass(in, out, s.size[1]);
            for (uint32_t ry = 0; ry < s.size[1]; ++ry) dist[distance_entry(s, rx, ry, rz)] = uint16_t(out[ry]);
        }
    // pass z: the columns (x, y) along z, in place, and the fold of the final values
    DistanceAcc acc = distance_acc();
    for (uint32_t ry = 0; ry < s.size[1]; ++ry)
        for (uint32_t rx = 0; rx < s.size[0]; ++rx) {
            for (uint32_t rz = 0; rz < kFloodSide; ++rz) in[rz] = rz < s.size[2] ? dist[distance_entry(s, rx, ry, rz)] : kDistanceNone;
            distance_pass(in, out, s.size[2]);
            for (uint32_t rz = 0; rz < s.size[2]; ++rz) {
                dist[distance_entry(s, rx, ry, rz)] = uint16_t(out[rz]);
                distance_fold_cell(acc, s, rx, ry, rz, out[rz]);
            }
        }
    if (field) {
        for (uint32_t at = 0; at < voxels; ++at) field[at] = dist[at];
        for (uint32_t at = voxels; at < padded; ++at) field[at] = uint16_t(kDistanceNone);
    }
    if (info) *info = distance_record(acc, s);
}

// the whole of vx_distance_boxes on one thread (the host test harness). field_stride: as the call takes it, in bytes (0:
// distance_field_bytes)
template <int FMT, class W>
inline void distance_boxes(const W& w, const uint8_t* lo, uint32_t lo_stride, uint32_t count, const vx_distance_shape& s, uint8_t* fields, uint32_t field_stride,
                           vx_distance_info* info) {
    const uint32_t stride = field_stride ? field_stride : distance_field_bytes(s);
    static thread_local uint16_t field[kDistanceCells];
    for (uint32_t n = 0; n < count; ++n) {
        int32_t at[3];
        __builtin_memcpy(at, lo + size_t(n) * lo_stride, 12);
        distance_query<FMT>(w, at, s, fields ? field : nullptr, info ? info + n : nullptr);
        if (fields) __builtin_memcpy(fields + size_t(n) * stride, field, distance_field_bytes(s));  // (whatever the alignment of `fields`)
    }
}

// the rules of the call that need no device: what is wrong, naming the field, or null. (Alignment of device memory: blocks_runtime.cpp.)
inline const char* check_distance(const void* lo, uint32_t lo_stride, uint32_t count, const vx_distance_shape* s, const void* fields, uint32_t field_stride,
                                  const void* info) {
    if (count == 0) return nullptr;  // nothing is read or written: nothing to refuse
    if (count > kDistanceMaxCount) return "count exceeds 1048576 (2^20)";
    if (!s) return "null shape";
    if (const char* what = lo_rule(lo, lo_stride, fields || info ? nullptr : "fields and info are both null")) return what;
    if (const char* what = size_rule(s->size, kFloodSide, "size: every component must be 1..32")) return what;
    if (s->flags & ~uint32_t(VX_DISTANCE_TO_AIR)) return "flags holds a bit other than VX_DISTANCE_TO_AIR";
    if (s->match_value && s->pass_value) return "pass_value must be 0 with a match_value";
    const uint32_t packed = distance_field_bytes(*s);
    const char* const at_least = "field_stride must be 0, or a multiple of 16 and at least 2 * size.x * size.y * size.z";
    if (fields)
        if (const char* what = field_stride_rule(count, field_stride, 2u * distance_voxels(*s), packed, at_least)) return what;
    const uint64_t lo_bytes = lo_span(count, lo_stride), field_bytes = fields ? field_span(count, field_stride, packed) : 0u;
    const uint64_t info_bytes = info ? uint64_t(count) * sizeof(vx_distance_info) : 0u;
    if (spans_meet(fields, field_bytes, lo, lo_bytes)) return "fields overlaps lo";
    if (spans_meet(info, info_bytes, lo, lo_bytes)) return "info overlaps lo";
    if (spans_meet(fields, field_bytes, info, info_bytes)) return "fields overlaps info";
    return nullptr;
}

}  // namespace vxb

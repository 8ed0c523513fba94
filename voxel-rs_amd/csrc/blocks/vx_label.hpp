// The loose pieces of the blocks in a batch of boxes (vx_label_boxes; include/voxel_hip.h): the connected-component labelling a caller of the
// reference would run on the host over get_block (gameplay.rs:161-201), asked of the world's OWN bytes. vx_flood.hpp's machinery turned
// inside out: its box, brick loading and rows of 32 bits, flooding the SOLID cells, seeded from the box's faces, then peeling the loose
// pieces off one by one. A workgroup of 256 threads owns one box of up to 32 x 32 x 32 cells.
//   rows: the cells (0..size.x, ry, rz) of the box are bit rx of row rz * 32 + ry, as vx_flood.hpp keeps them; rows and bits beyond the size
//   stay 0. Loading is vx_flood.hpp's (FloodBox, enter_brick_at, flood_brick_lane under label_load_shape: no seed, the same pass_value); a
//   loaded row holds the PASSABLE bits, and solid = ~row & label_row_mask(size.x) (label_solid_row).
//   a row's anchors (label_anchor_row): the x faces are bit 0 and bit size.x - 1 -- the same bit when size.x == 1 --, the y and z faces are
//   whole rows.
//   three words a row: solid, settled (held, or of a labelled piece) and piece (of the flood that is running). A step (label_step) is
//   vx_flood.hpp's flood_step with solid for passable and settled | piece for reached.
//   the budget (label_flood): the one loop every flood runs, over a callable that takes a step; see there.
//   the seed of a piece: the least key row << 5 | ctz(bits) over the rows' unsettled solid bits (label_seed_key): least rz, then ry, then rx.
//   a piece's fold (LabelAcc, label_fold_row, label_piece): cells, the x bits ORed, least and largest ry and rz, faces -- sums, ORs, minima
//   and maxima: any order gives the same.
// label_query runs a whole query on one thread, brick by brick, row by row and step by step as the kernel's workgroup runs it; label_boxes
// the whole call (the host test harness). The reader W is vx_blocks.hpp's. The standard library and voxel_hip.h only -- no HIP header, no
// HIP call.
#pragma once

#include <cstddef>

#include "vx_flood.hpp"

namespace vxb {

constexpr uint32_t kLabelMaxCount = 1u << 20;  // boxes of a call: a query may run thousands of steps, and the launch must end in bounded time
constexpr uint32_t kLabelMaxBytes = 1u << 24;  // of all piece records of a call (the fields: vx_rules.hpp)
constexpr uint32_t kLabelNoSeed = 0xffffffffu;

VXB_FN uint32_t label_voxels(const vx_label_shape& s) { return s.size[0] * s.size[1] * s.size[2]; }
VXB_FN uint32_t label_pack(uint32_t rx, uint32_t ry, uint32_t rz) { return rx | ry << 8 | rz << 16; }

// The bits a row of `side` cells (1..32) has. side == 32: 1u << 32 is no mask (the shift is undefined, and on the device it gives 1 << 0), so
// the full row is named.
VXB_FN uint32_t label_row_mask(uint32_t side) { return side >= 32u ? 0xffffffffu : (1u << side) - 1u; }

// a cell's rule: the complement of flood_passable
VXB_FN bool label_solid(uint32_t value, uint32_t pass_value) { return !flood_passable(value, pass_value); }
// a row's solid bits from the passable bits flood_brick_lane loaded
VXB_FN uint32_t label_solid_row(uint32_t passable, uint32_t side) { return ~passable & label_row_mask(side); }

// What vx_flood.hpp's loading takes: the box, no seed cell to report (seed_at 0: the value it keeps is not used), the same pass_value.
VXB_FN vx_flood_shape label_load_shape(const vx_label_shape& s) {
    vx_flood_shape f = {{s.size[0], s.size[1], s.size[2]}, {0u, 0u, 0u}, 0u, s.pass_value, 0u};
    return f;
}
// The box of a query and the bricks of its cover, modulo 2^32 as vxb::Region keeps a box.
VXB_FN FloodBox label_box(const int32_t lo[3], const vx_label_shape& s) {
    FloodBox b;
    for (int a = 0; a < 3; ++a) {
        b.lo[a] = uint32_t(lo[a]);
        b.first[a] = b.lo[a] & ~(kBrick - 1u);
        b.count[a] = ((b.lo[a] & (kBrick - 1u)) + s.size[a] + kBrick - 1u) >> kBrickLog2;
    }
    return b;
}

// The cells of row (ry, rz) that lie on a face of the box that `faces` names. (1u << (size.x - 1): size.x is 1..32, the shift 0..31.)
VXB_FN uint32_t label_face_row(const vx_label_shape& s, uint32_t faces, uint32_t ry, uint32_t rz) {
    if (((faces & 4u) && ry == 0u) || ((faces & 8u) && ry + 1u == s.size[1]) || ((faces & 16u) && rz == 0u) || ((faces & 32u) && rz + 1u == s.size[2]))
        return label_row_mask(s.size[0]);
    return ((faces & 1u) ? 1u : 0u) | ((faces & 2u) ? 1u << (s.size[0] - 1u) : 0u);
}
VXB_FN uint32_t label_anchor_row(const vx_label_shape& s, uint32_t ry, uint32_t rz) { return label_face_row(s, s.anchor_faces, ry, rz); }
// the faces of the box the cells `bits` of row (ry, rz) lie on
VXB_FN uint32_t label_faces(const vx_label_shape& s, uint32_t ry, uint32_t rz, uint32_t bits) {
    if (!bits) return 0u;
    return (bits & 1u) | (((bits >> (s.size[0] - 1u)) & 1u) << 1) | (ry == 0u ? 4u : 0u) | (ry + 1u == s.size[1] ? 8u : 0u) | (rz == 0u ? 16u : 0u) |
           (rz + 1u == s.size[2] ? 32u : 0u);
}

// One step of a row: the solid cells next to the frontier that no flood has taken yet.
VXB_FN uint32_t label_step(uint32_t f, uint32_t ym, uint32_t yp, uint32_t zm, uint32_t zp, uint32_t solid, uint32_t settled, uint32_t piece) {
    return flood_step(f, ym, yp, zm, zp, solid, settled | piece);
}

// The budget of a query's floods, and the one loop every flood runs. step(keep) takes one step of the flood -- the next layer from the last --
// and says whether it found a cell; with `keep` the cells it finds join the flood, without they are discarded. Layer 0, the seeds, is in place
// before. The flood is complete (true) when a step finds nothing: its depth is the number of steps that did, and used += depth. When the
// budget is spent -- used + depth == max_steps -- one PROBING step is still taken, with keep false, to tell a complete flood from a cut one:
// if it finds a cell the flood is cut (false), used = max_steps and VX_LABEL_CUT is set. At most max_steps - used + 1 steps.
struct LabelBudget {
    uint32_t used, max_steps, flags;
};
template <class Step>
VXB_FN bool label_flood(LabelBudget& b, Step step) {
    const uint32_t left = b.max_steps - b.used;
    for (uint32_t depth = 0; depth <= left; ++depth) {
        const bool probing = depth == left;
        if (!step(!probing)) {
            b.used += depth;
            return true;
        }
        if (probing) break;
    }
    b.used = b.max_steps;
    b.flags |= VX_LABEL_CUT;
    return false;
}

// The first unsettled solid cell of row r as a key that orders by rz, then ry, then rx; kLabelNoSeed: the row has none.
VXB_FN uint32_t label_seed_key(uint32_t r, uint32_t solid, uint32_t settled) {
    const uint32_t bits = solid & ~settled;
    return bits ? (r << 5 | uint32_t(__builtin_ctz(bits))) : kLabelNoSeed;
}
VXB_FN uint32_t label_key_row(uint32_t key) { return key >> 5; }
VXB_FN uint32_t label_key_bit(uint32_t key) { return 1u << (key & 31u); }

// What the rows say of a piece (or of all solid cells: cells and faces): folded row by row, then across the threads.
struct LabelAcc {
    uint32_t cells, xbits, ylo, yhi, zlo, zhi, faces;
};
VXB_FN LabelAcc label_acc() {
    LabelAcc a = {0u, 0u, kFloodSide, 0u, kFloodSide, 0u, 0u};
    return a;
}
VXB_FN void label_fold_row(LabelAcc& a, const vx_label_shape& s, uint32_t ry, uint32_t rz, uint32_t bits) {
    if (!bits) return;
    a.cells += popc(bits);
    a.xbits |= bits;
    a.ylo = ry < a.ylo ? ry : a.ylo;
    a.yhi = ry > a.yhi ? ry : a.yhi;
    a.zlo = rz < a.zlo ? rz : a.zlo;
    a.zhi = rz > a.zhi ? rz : a.zhi;
    a.faces |= label_faces(s, ry, rz, bits);
}
VXB_FN void label_fold(LabelAcc& a, const LabelAcc& b) {
    a.cells += b.cells;
    a.xbits |= b.xbits;
    a.ylo = b.ylo < a.ylo ? b.ylo : a.ylo;
    a.yhi = b.yhi > a.yhi ? b.yhi : a.yhi;
    a.zlo = b.zlo < a.zlo ? b.zlo : a.zlo;
    a.zhi = b.zhi > a.zhi ? b.zhi : a.zhi;
    a.faces |= b.faces;
}
// the record of a piece that has a cell, seeded at `key`
VXB_FN vx_label_piece label_piece(const LabelAcc& a, uint32_t key) {
    const uint32_t row = label_key_row(key);
    vx_label_piece p = {a.cells, label_pack(uint32_t(__builtin_ctz(a.xbits)), a.ylo, a.zlo), label_pack(31u - uint32_t(__builtin_clz(a.xbits)), a.yhi, a.zhi),
                        label_pack(key & 31u, row & (kFloodSide - 1u), row / kFloodSide) | a.faces << 24};
    return p;
}
VXB_FN vx_label_info label_record(uint32_t solid, uint32_t held, uint32_t pieces, uint32_t loose, uint32_t faces, const LabelBudget& b) {
    vx_label_info r = {solid, held, pieces, loose, solid - held - loose, b.used, faces, b.flags};
    return r;
}

// A whole query on one thread, as the kernel's workgroup runs it. field: round16(voxels) bytes, or null; pieces: s.max_pieces records, or
// null; info: a record, or null.
template <int FMT, class W>
inline void label_query(const W& w, const int32_t lo[3], const vx_label_shape& s, uint8_t* field, vx_label_piece* pieces, vx_label_info* info) {
    const uint32_t voxels = label_voxels(s), padded = flood_round16(voxels);
    const vx_flood_shape load = label_load_shape(s);
    const FloodBox box = label_box(lo, s);
    static thread_local uint32_t solid[kFloodRows], settled[kFloodRows], piece[kFloodRows], frontier[2][kFloodRows];
    for (uint32_t r = 0; r < kFloodRows; ++r) solid[r] = settled[r] = piece[r] = frontier[0][r] = frontier[1][r] = 0;
    // loading: the brick rows of the cover, one after the other (the kernel: four waves take them in turn)
    for (uint32_t n = 0; n < box.count[1] * box.count[2]; ++n) {
        const uint32_t cy = box.first[1] + (n % box.count[1]) * kBrick, cz = box.first[2] + (n / box.count[1]) * kBrick;
        uint32_t row[kFloodLanes], unused = 0;
        for (uint32_t lane = 0; lane < kFloodLanes; ++lane) row[lane] = 0;
        for (uint32_t bx = 0; bx < box.count[0]; ++bx) {
            const Brick b = enter_brick_at<FMT>(w, box.first[0] + bx * kBrick, cy, cz);
            for (uint32_t lane = 0; lane < kFloodLanes; ++lane) flood_brick_lane<FMT>(w, load, box, b, lane & 7u, lane >> 3, row[lane], unused);
        }
        for (uint32_t lane = 0; lane < kFloodLanes; ++lane) {
            const uint32_t ry = cy + (lane & 7u) - box.lo[1], rz = cz + (lane >> 3) - box.lo[2];
            if (ry < s.size[1] && rz < s.size[2]) solid[flood_row_of(ry, rz)] = label_solid_row(row[lane], s.size[0]);
        }
    }
    const auto in_box = [&](uint32_t r) { return (r & (kFloodSide - 1u)) < s.size[1] && r / kFloodSide < s.size[2]; };
    // the bytes of a row's cells `bits`
    const auto write = [&](uint32_t r, uint32_t bits, uint32_t byte) {
        if (field)
            for (uint32_t m = bits; m; m &= m - 1u) field[flood_field_row(load, r & (kFloodSide - 1u), r / kFloodSide) + uint32_t(__builtin_ctz(m))] = uint8_t(byte);
    };
    if (field)
        for (uint32_t at = 0; at < padded; ++at) field[at] = uint8_t(VX_LABEL_AIR);
    for (uint32_t r = 0; r < kFloodRows; ++r) write(r, solid[r], VX_LABEL_MORE);
    // a step of the running flood: frontier[phase] -> frontier[phase ^ 1], every row by its owner (the kernel: thread t owns rows t + 256 k)
    uint32_t phase = 0;
    const auto step = [&](bool keep) {
        const uint32_t* cur = frontier[phase];
        uint32_t* next = frontier[phase ^ 1u];
        uint32_t any = 0;
        for (uint32_t t = 0; t < kFloodThreads; ++t)
            for (uint32_t k = 0; k < kFloodOwned; ++k) {
                const uint32_t r = t + k * kFloodThreads, ry = r & (kFloodSide - 1u), rz = r / kFloodSide;
                uint32_t found = 0;
                if (in_box(r))
                    found = label_step(cur[r], ry > 0 ? cur[r - 1] : 0u, ry + 1u < s.size[1] ? cur[r + 1] : 0u, rz > 0 ? cur[r - kFloodSide] : 0u,
                                       rz + 1u < s.size[2] ? cur[r + kFloodSide] : 0u, solid[r], settled[r], piece[r]);
                next[r] = found;
                if (keep) piece[r] |= found;
                any |= found;
            }
        phase ^= 1u;
        return any != 0;
    };
    LabelBudget budget = {0u, s.max_steps, 0u};
    // held: from the solid cells on the anchor faces. Complete or cut, the layers the budget covered are held.
    for (uint32_t r = 0; r < kFloodRows; ++r) piece[r] = frontier[phase][r] = in_box(r) ? solid[r] & label_anchor_row(s, r & (kFloodSide - 1u), r / kFloodSide) : 0u;
    bool going = label_flood(budget, step);
    uint32_t held = 0, loose = 0, count = 0;
    for (uint32_t r = 0; r < kFloodRows; ++r) {
        write(r, piece[r], VX_LABEL_HELD);
        held += popc(piece[r]);
        settled[r] = piece[r];
        piece[r] = 0;
    }
    // the pieces, one by one. (After a complete flood the frontier written last is empty: the seed goes there.)
    while (going && count < s.max_pieces) {
        uint32_t key = kLabelNoSeed;
        for (uint32_t r = 0; r < kFloodRows; ++r) {
            const uint32_t k = label_seed_key(r, solid[r], settled[r]);
            key = k < key ? k : key;
        }
        if (key == kLabelNoSeed) break;
        piece[label_key_row(key)] = frontier[phase][label_key_row(key)] = label_key_bit(key);
        going = label_flood(budget, step);
        LabelAcc acc = label_acc();
        for (uint32_t r = 0; r < kFloodRows; ++r) {
            if (going) {
                write(r, piece[r], count + 1u);
                label_fold_row(acc, s, r & (kFloodSide - 1u), r / kFloodSide, piece[r]);
                settled[r] |= piece[r];
            }
            piece[r] = 0;
        }
        if (!going) break;
        if (pieces) pieces[count] = label_piece(acc, key);
        loose += acc.cells;
        ++count;
    }
    if (pieces)
        for (uint32_t k = count; k < s.max_pieces; ++k) pieces[k] = vx_label_piece{0u, 0u, 0u, 0u};
    if (info) {
        LabelAcc all = label_acc();
        for (uint32_t r = 0; r < kFloodRows; ++r) label_fold_row(all, s, r & (kFloodSide - 1u), r / kFloodSide, solid[r]);
        *info = label_record(all.cells, held, count, loose, all.faces, budget);
    }
}

// the whole of vx_label_boxes on one thread (the host test harness). field_stride: as the call takes it (0: the voxel count rounded up to 16)
template <int FMT, class W>
inline void label_boxes(const W& w, const uint8_t* lo, uint32_t lo_stride, uint32_t count, const vx_label_shape& s, uint8_t* fields, uint32_t field_stride,
                        vx_label_piece* pieces, vx_label_info* info) {
    const uint32_t stride = field_stride ? field_stride : flood_round16(label_voxels(s));
    for (uint32_t n = 0; n < count; ++n) {
        int32_t at[3];
        __builtin_memcpy(at, lo + size_t(n) * lo_stride, 12);
        label_query<FMT>(w, at, s, fields ? fields + size_t(n) * stride : nullptr, pieces ? pieces + size_t(n) * s.max_pieces : nullptr, info ? info + n : nullptr);
    }
}

// the rules of the call that need no device: what is wrong, naming the field, or null. (Alignment of device memory: blocks_runtime.cpp.)
inline const char* check_label(const void* lo, uint32_t lo_stride, uint32_t count, const vx_label_shape* s, const void* fields, uint32_t field_stride,
                               const void* pieces, const void* info) {
    if (count == 0) return nullptr;  // nothing is read or written: nothing to refuse
    if (count > kLabelMaxCount) return "count exceeds 1048576 (2^20)";
    if (!s) return "null shape";
    if (const char* what = lo_rule(lo, lo_stride, fields || pieces || info ? nullptr : "fields, pieces and info are all null")) return what;
    if (const char* what = size_rule(s->size, kFloodSide, "size: every component must be 1..32")) return what;
    if (s->anchor_faces & ~uint32_t(VX_LABEL_ALL_FACES)) return "anchor_faces holds a bit above bit 5";
    if (s->max_pieces > VX_LABEL_MAX_PIECES) return "max_pieces exceeds VX_LABEL_MAX_PIECES (250)";
    if (s->max_steps > VX_LABEL_MAX_STEPS) return "max_steps exceeds VX_LABEL_MAX_STEPS (4096)";
    if (s->flags) return "flags must be 0";
    if (pieces && s->max_pieces == 0) return "pieces with max_pieces == 0";
    const uint32_t packed = flood_round16(label_voxels(*s));
    const char* const at_least = "field_stride must be 0, or a multiple of 16 and at least size.x * size.y * size.z";
    if (fields)
        if (const char* what = field_stride_rule(count, field_stride, label_voxels(*s), packed, at_least)) return what;
    const uint64_t piece_bytes = pieces ? uint64_t(count) * s->max_pieces * sizeof(vx_label_piece) : 0u;
    if (piece_bytes > kLabelMaxBytes) return "count * max_pieces * 16 exceeds 16777216 (2^24) bytes";
    const uint64_t lo_bytes = lo_span(count, lo_stride), field_bytes = fields ? field_span(count, field_stride, packed) : 0u;
    const uint64_t info_bytes = info ? uint64_t(count) * sizeof(vx_label_info) : 0u;
    if (spans_meet(fields, field_bytes, lo, lo_bytes)) return "fields overlaps lo";
    if (spans_meet(pieces, piece_bytes, lo, lo_bytes)) return "pieces overlaps lo";
    if (spans_meet(info, info_bytes, lo, lo_bytes)) return "info overlaps lo";
    if (spans_meet(fields, field_bytes, pieces, piece_bytes)) return "fields overlaps pieces";
    if (spans_meet(fields, field_bytes, info, info_bytes)) return "fields overlaps info";
    if (spans_meet(pieces, piece_bytes, info, info_bytes)) return "pieces overlaps info";
    return nullptr;
}

}  // namespace vxb

// TEST HARNESS ONLY: voxel-rs_amd/csrc/blocks/vx_block_scratch.hpp -- what a block entry point's host-memory call keeps in pinned scratch --
// as a stand-alone program over the header alone. Every source and destination is a heap block of exactly the size the ABI allows (an input
// of n items at stride s is s * (n - 1) + 12 bytes, one value for a stride of 0; the scratch is exactly the layout's end; a caller's fields
// are stride * (n - 1) + packed bytes), so a read of `stride` bytes of the last item or a write of a rounded size is a finding of the
// sanitizer build (-fsanitize=address,undefined). tests/test_block_scratch_on_host.py builds and runs it, plain and sanitized. The layouts
// are the chains of ScratchLayout::take that blocks_runtime.cpp writes, said again here, against offsets worked out by hand from the
// arithmetic the entry points had before the header (round16(v) = v rounded up to 16). Never linked into the product libraries.
//
//   block_scratch_on_host          prints a line a section, "<section>: ok, <n> checks"; the first failure ends it with status 1
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <memory>

#include "vx_block_scratch.hpp"

namespace {

using vxb::ScratchLayout;
using Bytes = std::unique_ptr<uint8_t[]>;

long g_checks = 0;
#define CHECK(cond)                                                                  \
    do {                                                                             \
        ++g_checks;                                                                  \
        if (!(cond)) {                                                               \
            std::printf("FAILED at line %d: %s\n", __LINE__, #cond);                 \
            std::exit(1);                                                            \
        }                                                                            \
    } while (0)

void section(const char* name) {
    std::printf("%s: ok, %ld checks\n", name, g_checks);
    g_checks = 0;
}

constexpr size_t kCounts[] = {1, 2, 5};  // 5 * 12 = 60 is no multiple of 16: every rounding rounds
constexpr uint32_t kStrides[] = {0, 12, 16, 28};

// byte j of item i of the vector called `tag`
uint8_t value_of(unsigned tag, size_t i, size_t j) { return uint8_t(tag * 67 + i * 13 + j * 3 + 1); }

size_t source_bytes(uint32_t stride, size_t n) { return stride ? size_t(stride) * (n - 1) + 12 : 12; }

// `n` items (one for a stride of 0) at `stride` in a block of exactly the bytes the ABI allows, 0xEE between the items
Bytes make_source(unsigned tag, uint32_t stride, size_t n) {
    const size_t bytes = source_bytes(stride, n);
    Bytes b(new uint8_t[bytes]);
    std::memset(b.get(), 0xEE, bytes);
    for (size_t i = 0; i < (stride ? n : 1); ++i)
        for (size_t j = 0; j < 12; ++j) b[size_t(stride) * i + j] = value_of(tag, i, j);
    return b;
}

// what a kernel reads as item i of a vector at `base` with `stride`: item 0 for a stride of 0
bool item_is(const void* base, uint32_t stride, unsigned tag, size_t i) {
    const uint8_t* p = static_cast<const uint8_t*>(base) + size_t(stride) * i;
    for (size_t j = 0; j < 12; ++j)
        if (p[j] != value_of(tag, stride ? i : 0, j)) return false;
    return true;
}

void test_packing() {
    for (const size_t n : kCounts)
        for (const uint32_t stride : kStrides) {
            const Bytes src = make_source(1, stride, n);
            const size_t kept = vxb::packed3_bytes(src.get(), stride, n);
            CHECK(kept == (stride ? 12 * n : 12));
            CHECK(vxb::packed3_stride(stride) == (stride ? 12u : 0u));
            Bytes to(new uint8_t[kept]);
            vxb::pack3(to.get(), src.get(), stride, n);
            for (size_t i = 0; i < n; ++i) CHECK(item_is(to.get(), vxb::packed3_stride(stride), 1, i));
        }
    // a null optional vector keeps nothing and writes nothing
    CHECK(vxb::packed3_bytes(nullptr, 12, 5) == 0 && vxb::packed3_bytes(nullptr, 0, 5) == 0);
    Bytes none(new uint8_t[0]);
    vxb::pack3(none.get(), nullptr, 12, 5);
    vxb::pack3(none.get(), nullptr, 0, 5);
    section("packing");
}

// a vx_box_batch over exact-size sources: offset_stride < 0: no offset
struct HostBoxes {
    Bytes origin, offset, extents;
    vx_box_batch batch;
    HostBoxes(size_t n, uint32_t origin_stride, int offset_stride, uint32_t extents_stride) {
        origin = make_source(2, origin_stride, n);
        if (offset_stride >= 0) offset = make_source(3, uint32_t(offset_stride), n);
        extents = make_source(4, extents_stride, n);
        batch = {origin.get(), offset.get(), extents.get(), origin_stride, offset_stride < 0 ? 0u : uint32_t(offset_stride), extents_stride, 77u};
    }
};

void test_boxes() {
    const int offset_strides[] = {-1, 0, 12, 16, 28};
    for (const size_t n : kCounts)
        for (const uint32_t origin_stride : {12u, 16u, 28u})
            for (const int offset_stride : offset_strides)
                for (const uint32_t extents_stride : kStrides) {
                    const HostBoxes b(n, origin_stride, offset_stride, extents_stride);
                    const size_t n_offset = offset_stride < 0 ? 0 : (offset_stride ? n : 1), n_extents = extents_stride ? n : 1;
                    const size_t kept = vxb::packed_boxes_bytes(b.batch, n);
                    CHECK(kept == 12 * (n + n_offset + n_extents));  // nothing rounded between the vectors
                    Bytes scratch(new uint8_t[kept]);
                    const vx_box_batch k = vxb::pack_boxes(b.batch, n, scratch.get(), scratch.get());  // (the device's view: the same bytes)
                    CHECK(k.origin == scratch.get() && k.origin_stride == 12 && k.only_value == 77u);
                    CHECK(offset_stride < 0 ? k.offset == nullptr : k.offset == scratch.get() + 12 * n);
                    CHECK(k.extents == scratch.get() + 12 * (n + n_offset));
                    CHECK(k.offset_stride == (offset_stride > 0 ? 12u : 0u) && k.extents_stride == (extents_stride ? 12u : 0u));
                    for (size_t i = 0; i < n; ++i) {
                        CHECK(item_is(k.origin, k.origin_stride, 2, i) && item_is(k.extents, k.extents_stride, 4, i));
                        if (k.offset) CHECK(item_is(k.offset, k.offset_stride, 3, i));
                    }
                }
    section("boxes");
}

// ---- the eight layouts, as blocks_runtime.cpp chains them -----------------------------------------------------------------------------------

// vx_block_points (records of 8 bytes), vx_scan_points (16): the positions | the records
struct Points { size_t at_pos, at_out, end; };
Points lay_points(size_t n, size_t record) {
    ScratchLayout lay;
    Points p = {};
    p.at_pos = lay.take(12 * n);
    p.at_out = lay.take(n * record, 16);
    p.end = lay.end;
    return p;
}

// vx_overlap_boxes (records of 32 bytes), and vx_move_boxes (48) with the motions behind the boxes
struct Boxes { size_t at_boxes, at_motion, at_out, end; };
Boxes lay_boxes(const vx_box_batch& b, size_t n, const void* motion, uint32_t motion_stride, size_t record) {
    ScratchLayout lay;
    Boxes p = {};
    p.at_boxes = lay.take(vxb::packed_boxes_bytes(b, n));
    p.at_motion = lay.take(vxb::packed3_bytes(motion, motion_stride, n));
    p.at_out = lay.take(n * record, 16);
    p.end = lay.end;
    return p;
}

// vx_flood_points: the positions | the records of 16 bytes | the fields; vx_light_boxes: the props (4096 bytes) in front
struct Fields { size_t at_props, at_pos, at_info, at_fields, end; };
Fields lay_fields(size_t n, bool props, bool info, bool fields, size_t packed) {
    ScratchLayout lay;
    Fields p = {};
    p.at_props = lay.take(props ? VX_LIGHT_MAX_PROPS : 0);
    p.at_pos = lay.take(12 * n, props ? 16 : 1);
    p.at_info = lay.take(info ? 16 * n : 0, 16);
    p.at_fields = lay.take(fields ? n * packed : 0, 16);
    p.end = lay.end;
    return p;
}

// vx_walk_points: the positions | the goals, or the one | the records of 32 bytes | the paths | the fields
struct Walk { size_t at_pos, at_goal, at_info, at_paths, at_fields, end; };
Walk lay_walk(size_t n, const void* goal, uint32_t goal_stride, bool info, size_t path_capacity, bool fields, size_t packed) {
    ScratchLayout lay;
    Walk p = {};
    p.at_pos = lay.take(12 * n);
    p.at_goal = lay.take(vxb::packed3_bytes(goal, goal_stride, n), 16);
    p.at_info = lay.take(info ? 32 * n : 0, 16);
    p.at_paths = lay.take(n * path_capacity * 4, 16);
    p.at_fields = lay.take(fields ? n * packed : 0, 16);
    p.end = lay.end;
    return p;
}

bool points_are(const Points& p, size_t at_out, size_t end) { return p.at_pos == 0 && p.at_out == at_out && p.end == end && p.at_out % 16 == 0; }
bool boxes_are(const Boxes& p, size_t at_motion, size_t at_out, size_t end) {
    return p.at_boxes == 0 && p.at_motion == at_motion && p.at_out == at_out && p.end == end && p.at_motion % 4 == 0 && p.at_out % 16 == 0;
}
bool fields_are(const Fields& p, size_t at_pos, size_t at_info, size_t at_fields, size_t end) {
    return p.at_props == 0 && p.at_pos == at_pos && p.at_info == at_info && p.at_fields == at_fields && p.end == end && p.at_pos % 4 == 0 && p.at_info % 16 == 0 &&
           p.at_fields % 16 == 0;
}
bool walk_is(const Walk& p, size_t at_goal, size_t at_info, size_t at_paths, size_t at_fields, size_t end) {
    return p.at_pos == 0 && p.at_goal == at_goal && p.at_info == at_info && p.at_paths == at_paths && p.at_fields == at_fields && p.end == end && p.at_goal % 16 == 0 &&
           p.at_info % 16 == 0 && p.at_paths % 16 == 0 && p.at_fields % 16 == 0;
}

void test_layouts() {
    // the running layout itself
    ScratchLayout lay;
    CHECK(lay.take(0) == 0 && lay.end == 0 && lay.take(0, 16) == 0 && lay.end == 0);
    CHECK(lay.take(5) == 0 && lay.take(3) == 5 && lay.take(4, 4) == 8 && lay.take(1, 16) == 16 && lay.end == 17 && lay.take(0, 16) == 32 && lay.end == 32);

    // points: at_out = round16(12 n), end = at_out + 8 n        n = 1: 16, 24    n = 2: round16(24) = 32, 48    n = 5: round16(60) = 64, 104
    CHECK(points_are(lay_points(1, 8), 16, 24) && points_are(lay_points(2, 8), 32, 48) && points_are(lay_points(5, 8), 64, 104));
    // scan: the same, end = at_out + 16 n                       n = 1: 16, 32    n = 2: 32, 64    n = 5: 64, 144
    CHECK(points_are(lay_points(1, 16), 16, 32) && points_are(lay_points(2, 16), 32, 64) && points_are(lay_points(5, 16), 64, 144));

    uint8_t some[12] = {};  // (only asked whether it is null)
    const vx_box_batch each = {some, some, some, 16, 28, 12, 0}, shared = {some, some, some, 12, 0, 0, 0}, bare = {some, nullptr, some, 64, 0, 0, 0};
    // boxes, a vector each a box: 36 n of inputs, at_out = round16(36 n), end = at_out + 32 n
    //   n = 1: 36 -> 48, 80    n = 2: 72 -> 80, 144    n = 5: 180 -> 192, 352
    CHECK(boxes_are(lay_boxes(each, 1, nullptr, 0, 32), 36, 48, 80) && boxes_are(lay_boxes(each, 2, nullptr, 0, 32), 72, 80, 144));
    CHECK(boxes_are(lay_boxes(each, 5, nullptr, 0, 32), 180, 192, 352));
    // boxes, one offset and one extents: 12 n + 24     n = 1: 36 -> 48, 80    n = 2: 48 -> 48, 112    n = 5: 84 -> 96, 256
    CHECK(boxes_are(lay_boxes(shared, 1, nullptr, 0, 32), 36, 48, 80) && boxes_are(lay_boxes(shared, 2, nullptr, 0, 32), 48, 48, 112));
    CHECK(boxes_are(lay_boxes(shared, 5, nullptr, 0, 32), 84, 96, 256));
    // boxes, no offset and one extents: 12 n + 12      n = 1: 24 -> 32, 64    n = 2: 36 -> 48, 112    n = 5: 72 -> 80, 240
    CHECK(boxes_are(lay_boxes(bare, 1, nullptr, 0, 32), 24, 32, 64) && boxes_are(lay_boxes(bare, 2, nullptr, 0, 32), 36, 48, 112));
    CHECK(boxes_are(lay_boxes(bare, 5, nullptr, 0, 32), 72, 80, 240));
    // move, a vector each a box and a motion each: at_motion = 36 n, at_out = round16(48 n) = 48 n, end = 96 n
    CHECK(boxes_are(lay_boxes(each, 1, some, 16, 48), 36, 48, 96) && boxes_are(lay_boxes(each, 2, some, 16, 48), 72, 96, 192));
    CHECK(boxes_are(lay_boxes(each, 5, some, 16, 48), 180, 240, 480));
    // move, one offset, one extents, one motion: at_motion = 12 n + 24, at_out = round16(12 n + 36), end = at_out + 48 n
    //   n = 1: 36, 48, 96    n = 2: 48, round16(60) = 64, 160    n = 5: 84, 96, 336
    CHECK(boxes_are(lay_boxes(shared, 1, some, 0, 48), 36, 48, 96) && boxes_are(lay_boxes(shared, 2, some, 0, 48), 48, 64, 160));
    CHECK(boxes_are(lay_boxes(shared, 5, some, 0, 48), 84, 96, 336));
    // move, no offset, one extents, a motion each: at_motion = 12 n + 12, at_out = round16(24 n + 12)
    //   n = 1: 24, round16(36) = 48, 96    n = 2: 36, round16(60) = 64, 160    n = 5: 72, round16(132) = 144, 384
    CHECK(boxes_are(lay_boxes(bare, 1, some, 12, 48), 24, 48, 96) && boxes_are(lay_boxes(bare, 2, some, 12, 48), 36, 64, 160));
    CHECK(boxes_are(lay_boxes(bare, 5, some, 12, 48), 72, 144, 384));

    // flood, fields of 17 voxels (32 bytes packed): at_info = round16(12 n), at_fields = at_info + 16 n, end = at_fields + 32 n
    //   n = 1: 16, 32, 64    n = 2: 32, 64, 128    n = 5: 64, 144, 304
    CHECK(fields_are(lay_fields(1, false, true, true, 32), 0, 16, 32, 64) && fields_are(lay_fields(2, false, true, true, 32), 0, 32, 64, 128));
    CHECK(fields_are(lay_fields(5, false, true, true, 32), 0, 64, 144, 304));
    // flood, n = 5, fields of 3 voxels (16 bytes): end = 144 + 80; without records: the fields at 64, end = 64 + 160; without fields: end = 144
    CHECK(fields_are(lay_fields(5, false, true, true, 16), 0, 64, 144, 224) && fields_are(lay_fields(5, false, false, true, 32), 0, 64, 64, 224));
    CHECK(fields_are(lay_fields(5, false, true, false, 32), 0, 64, 144, 144));
    // light: the same behind 4096 bytes of props     n = 1: 4112, 4128, 4160    n = 2: 4128, 4160, 4224    n = 5: 4160, 4240, 4400
    CHECK(fields_are(lay_fields(1, true, true, true, 32), 4096, 4112, 4128, 4160) && fields_are(lay_fields(2, true, true, true, 32), 4096, 4128, 4160, 4224));
    CHECK(fields_are(lay_fields(5, true, true, true, 32), 4096, 4160, 4240, 4400));
    CHECK(fields_are(lay_fields(5, true, false, true, 32), 4096, 4160, 4160, 4320) && fields_are(lay_fields(5, true, true, false, 32), 4096, 4160, 4240, 4240));

    // walk, a goal each, records, paths of 4 entries (16 n bytes), fields of 32 bytes:
    //   at_goal = round16(12 n), at_info = at_goal + round16(12 n), at_paths = at_info + 32 n, at_fields = at_paths + 16 n, end = at_fields + 32 n
    //   n = 1: 16, 32, 64, 80, 112    n = 2: 32, 64, 128, 160, 224    n = 5: 64, 128, 288, 368, 528
    CHECK(walk_is(lay_walk(1, some, 16, true, 4, true, 32), 16, 32, 64, 80, 112) && walk_is(lay_walk(2, some, 16, true, 4, true, 32), 32, 64, 128, 160, 224));
    CHECK(walk_is(lay_walk(5, some, 16, true, 4, true, 32), 64, 128, 288, 368, 528));
    // walk, n = 5, the one goal (12 bytes, rounded to 16): 64, 80, 240, 320, 480; no goal: 64, 64, 224, 304, 464
    CHECK(walk_is(lay_walk(5, some, 0, true, 4, true, 32), 64, 80, 240, 320, 480) && walk_is(lay_walk(5, nullptr, 0, true, 4, true, 32), 64, 64, 224, 304, 464));
    // walk, n = 5, a goal each: no paths: the fields at 288, end 448; no records: paths at 128, fields at 208, end 368; no fields: end 368;
    // the fields alone, no goal: at 64, end 224
    CHECK(walk_is(lay_walk(5, some, 12, true, 0, true, 32), 64, 128, 288, 288, 448) && walk_is(lay_walk(5, some, 12, false, 4, true, 32), 64, 128, 128, 208, 368));
    CHECK(walk_is(lay_walk(5, some, 12, true, 4, false, 32), 64, 128, 288, 368, 368) && walk_is(lay_walk(5, nullptr, 0, false, 0, true, 32), 64, 64, 64, 64, 224));
    section("layouts");
}

// A whole host-memory call's scratch, of exactly the layout's end: vx_walk_points' inputs packed into it and read again as the kernel reads
// them (the layout with the most parts; positions at stride 28, the goals in every form).
void test_a_call() {
    for (const size_t n : kCounts)
        for (const int goal_stride : {-1, 0, 12, 16}) {
            const Bytes pos = make_source(5, 28, n), goal = goal_stride < 0 ? Bytes() : make_source(6, uint32_t(goal_stride), n);
            const uint32_t stride = goal_stride < 0 ? 0u : uint32_t(goal_stride);
            const Walk at = lay_walk(n, goal.get(), stride, true, 4, true, 32);
            Bytes scratch(new uint8_t[at.end]);
            vxb::pack3(scratch.get() + at.at_pos, pos.get(), 28, n);
            vxb::pack3(scratch.get() + at.at_goal, goal.get(), stride, n);
            std::memset(scratch.get() + at.at_info, 0, at.end - at.at_info);  // (the kernel's part)
            for (size_t i = 0; i < n; ++i) {
                CHECK(item_is(scratch.get() + at.at_pos, 12, 5, i));
                if (goal) CHECK(item_is(scratch.get() + at.at_goal, vxb::packed3_stride(stride), 6, i));
            }
        }
    section("a call");
}

void test_spreading() {
    for (const size_t voxels : {size_t(3), size_t(17)}) {
        const size_t packed = (voxels + 15) & ~size_t(15);  // 16, 32: with padding behind the voxels
        for (const size_t n : kCounts)
            for (const size_t stride : {packed, packed + 16}) {
                Bytes from(new uint8_t[n * packed]);
                for (size_t i = 0; i < n * packed; ++i) from[i] = uint8_t(i * 7 + 3) | 1u;  // (never the sentinel's even byte)
                const size_t bytes = stride * (n - 1) + packed;
                Bytes to(new uint8_t[bytes]);
                std::memset(to.get(), 0xA4, bytes);
                vxb::spread_fields(to.get(), stride, from.get(), packed, n);
                for (size_t i = 0; i < n; ++i) {
                    CHECK(std::memcmp(to.get() + i * stride, from.get() + i * packed, packed) == 0);
                    for (size_t j = packed; j < stride && i + 1 < n; ++j) CHECK(to[i * stride + j] == 0xA4);  // between two fields: the caller's
                }
            }
    }
    section("spreading");
}

}  // namespace

int main() {
    test_packing();
    test_boxes();
    test_layouts();
    test_a_call();
    test_spreading();
    return 0;
}

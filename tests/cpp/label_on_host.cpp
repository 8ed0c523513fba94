// TEST HARNESS ONLY: vx_label_boxes' answer (voxel-rs_amd/csrc/blocks/vx_label.hpp) compiled for the host, as a stand-alone program -- the
// whole call on one thread, box by box: the bricks, rows, steps and floods the kernel's workgroup walks, with loops where the kernel has
// threads -- over a world frame read from a file into a heap block of exactly its size (every read range-checked, as the device's buffer
// resource checks it; a sanitizer build of this program sees any that is not), the boxes read through their stride from a heap block of
// exactly the input file's size, into heap blocks of exactly the bytes the call may write. tests/test_label_on_host.py runs it, plain and
// built with -fsanitize=address,undefined; tests/test_label.py holds the GPU's bytes against its output. Never linked into the product
// libraries; the product has no CPU path.
//
//   label_on_host <svo_type> <world.bin> label <lo.bin> <lo_stride> <count> <size.x> <size.y> <size.z> <anchor_faces> <max_pieces> <max_steps>
//                 <pass_value> <field_stride> <fields.bin | -> <pieces.bin | -> <info.bin | ->
//                                  -> fields.bin: count * field_stride bytes (field_stride 0: the voxel count rounded up to 16), what the call
//                                  leaves untouched 0x5a; pieces.bin: count * max_pieces vx_label_piece records; info.bin: `count`
//                                  vx_label_info records; "-": that output is null
//   label_on_host rules            prints what check_label refuses
#include "on_host.hpp"
#include "vx_label.hpp"

using namespace on_host;
const char* const on_host::program = "label_on_host";

namespace {

int usage() {
    std::fprintf(stderr, "usage: label_on_host <svo_type> <world.bin> label <lo.bin> <lo_stride> <count> <size x y z> <anchor_faces> <max_pieces> <max_steps> "
                         "<pass_value> <field_stride> <fields.bin | -> <pieces.bin | -> <info.bin | ->\n       label_on_host rules\n");
    return 2;
}

int rules() {
    alignas(16) static int32_t v[64];
    alignas(16) static uint8_t fields[2 * 4096];
    static vx_label_piece pieces[2 * 250];
    static vx_label_info info[2];
    const unsigned char* bytes = reinterpret_cast<const unsigned char*>(v);
    const vx_label_shape ok = {{16, 16, 16}, VX_LABEL_ALL_FACES, 250, 4096, 0, 0};
    const auto check = [&](const vx_label_shape& s, uint32_t count = 1, uint32_t field_stride = 0) { return vxb::check_label(v, 12, count, &s, fields, field_stride, pieces, info); };
    say("packed", vxb::check_label(v, 12, 2, &ok, fields, 0, pieces, info));
    say("stride 64", vxb::check_label(v, 64, 1, &ok, fields, 0, pieces, info));
    say("fields only", vxb::check_label(v, 12, 2, &ok, fields, 0, nullptr, nullptr));
    say("pieces only", vxb::check_label(v, 12, 2, &ok, nullptr, 0, pieces, nullptr));
    say("info only", vxb::check_label(v, 12, 2, &ok, nullptr, 0, nullptr, info));
    say("info only, any stride", vxb::check_label(v, 12, 2, &ok, nullptr, 7, nullptr, info));
    say("count 0", vxb::check_label(nullptr, 0, 0, nullptr, nullptr, 0, nullptr, nullptr));
    {   // (the largest count: its boxes have to exist for the overlap rule, so they come from the heap)
        std::vector<int32_t> many(size_t(3) << 20);
        std::vector<vx_label_info> records(size_t(1) << 20);
        say("count 2^20", vxb::check_label(many.data(), 12, 1u << 20, &ok, nullptr, 0, nullptr, records.data()));
        say("too many", vxb::check_label(many.data(), 12, (1u << 20) + 1u, &ok, nullptr, 0, nullptr, records.data()));
    }
    say("null shape", vxb::check_label(v, 12, 1, nullptr, fields, 0, pieces, info));
    say("null lo", vxb::check_label(nullptr, 12, 1, &ok, fields, 0, pieces, info));
    say("no output", vxb::check_label(v, 12, 1, &ok, nullptr, 0, nullptr, nullptr));
    for (uint32_t stride : {0u, 4u, 8u, 13u, 14u}) say("lo_stride " + std::to_string(stride), vxb::check_label(v, stride, 1, &ok, fields, 0, pieces, info));
    for (int off : {1, 2, 3}) say("lo + " + std::to_string(off), vxb::check_label(bytes + off, 12, 1, &ok, fields, 0, pieces, info));
    vx_label_shape s = ok;
    for (int a = 0; a < 3; ++a)
        for (uint32_t side : {0u, 33u, 0xffffffffu}) {
            s = ok, s.size[a] = side;
            say("size[" + std::to_string(a) + "] " + std::to_string(side), check(s));
        }
    s = ok, s.size[0] = s.size[1] = s.size[2] = 32;
    say("largest box", vxb::check_label(v, 12, 1, &s, nullptr, 0, pieces, info));
    s = ok, s.size[0] = s.size[1] = s.size[2] = 1;
    say("smallest box", check(s));
    for (uint32_t faces : {0u, 4u, 0x3fu, 0x40u, 0x80000000u}) {
        s = ok, s.anchor_faces = faces;
        say("anchor_faces " + std::to_string(faces), check(s));
    }
    for (uint32_t most : {0u, 250u, 251u}) {
        s = ok, s.max_pieces = most;
        say("max_pieces " + std::to_string(most), vxb::check_label(v, 12, 1, &s, fields, 0, nullptr, info));
    }
    s = ok, s.max_pieces = 0;
    say("pieces with max_pieces 0", check(s));
    for (uint32_t steps : {0u, 4096u, 4097u}) {
        s = ok, s.max_steps = steps;
        say("max_steps " + std::to_string(steps), check(s));
    }
    for (uint32_t flags : {1u, 0x80000000u}) {
        s = ok, s.flags = flags;
        say("flags " + std::to_string(flags), check(s));
    }
    s = ok, s.pass_value = 0xffffffffu;
    say("any pass_value", check(s));
    for (uint32_t stride : {4097u, 4104u, 4080u, 4096u, 4112u, 16u, 8192u}) say("field_stride " + std::to_string(stride), vxb::check_label(v, 12, 1, &ok, fields, stride, nullptr, nullptr));
    {
        std::vector<int32_t> many(size_t(3) * 4200);
        std::vector<uint8_t> big((size_t(1) << 24) + 8192);
        s = ok, s.max_pieces = 0;
        say("field bytes 2^24", vxb::check_label(many.data(), 12, 2048, &s, big.data(), 8192, nullptr, nullptr));
        say("field bytes 2^24 + 8192", vxb::check_label(many.data(), 12, 2049, &s, big.data(), 8192, nullptr, nullptr));
        say("piece bytes 2^24", vxb::check_label(many.data(), 12, 4194, &ok, nullptr, 0, big.data(), nullptr));       // 4,194 * 250 * 16 = 16,776,000
        say("piece bytes 2^24 + 2784", vxb::check_label(many.data(), 12, 4195, &ok, nullptr, 0, big.data(), nullptr));  // 4,195 * 250 * 16 = 16,780,000
    }
    // overlaps: an output on lo, two outputs on one another; side by side is allowed
    alignas(16) static uint8_t block[4096 + 64];
    s = ok, s.size[0] = s.size[1] = s.size[2] = 4, s.max_pieces = 2;  // a field of 64 bytes, 32 bytes of pieces, 32 of info
    say("fields on lo", vxb::check_label(block + 32, 12, 1, &s, block, 0, nullptr, nullptr));
    say("fields beside lo", vxb::check_label(block + 64, 12, 1, &s, block, 0, nullptr, nullptr));
    say("pieces on lo", vxb::check_label(block + 16, 12, 1, &s, nullptr, 0, block, nullptr));
    say("info on lo", vxb::check_label(block + 28, 12, 1, &s, nullptr, 0, nullptr, block));
    say("info beside lo", vxb::check_label(block + 32, 12, 1, &s, nullptr, 0, nullptr, block));
    say("fields on pieces", vxb::check_label(v, 12, 1, &s, block, 0, block + 48, nullptr));
    say("fields on info", vxb::check_label(v, 12, 1, &s, block + 16, 0, nullptr, block));
    say("pieces on info", vxb::check_label(v, 12, 1, &s, nullptr, 0, block + 16, block));
    say("all side by side", vxb::check_label(v, 12, 1, &s, block, 0, block + 64, block + 96));
    say("strided fields between", vxb::check_label(v, 12, 2, &s, block, 128, block + 64, nullptr));  // (spans, first byte to last: the gap counts)
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc == 2 && !std::strcmp(argv[1], "rules")) return rules();
    if (argc != 18 || std::strcmp(argv[3], "label")) return usage();
    const int svo_type = svo_type_of(argv[1]);
    if (svo_type < 0) return usage();
    std::vector<uint8_t> world, raw;
    if (!load(argv[2], world) || !load(argv[4], raw)) return 1;
    const HostWorld w = {world.data(), world.size()};
    const auto u32 = [argv](int i) { return u32_of(argv[i]); };
    const uint32_t lo_stride = u32(5), count = u32(6), field_stride = u32(14);
    const vx_label_shape s = {{u32(7), u32(8), u32(9)}, u32(10), u32(11), u32(12), u32(13), 0u};
    // (the shape's own rules first, on one box and a record that lies apart: the sizes below come from a shape that has passed them; the
    // whole call's rules again below, on the blocks it writes to)
    alignas(16) static uint8_t apart[32];
    if (const char* refused = vxb::check_label(raw.data(), 12, (count && raw.size() >= 12) ? 1u : 0u, &s, nullptr, 0, nullptr, apart)) return refuse(refused);
    if (count > vxb::kLabelMaxCount) return refuse("count exceeds 1048576 (2^20)");
    if (field_stride % 16u) return refuse("field_stride must be 0, or a multiple of 16");
    const size_t packed = vxb::flood_round16(vxb::label_voxels(s));
    Fields fields(given(argv[15]), count, field_stride ? field_stride : packed, packed);
    Output<vx_label_piece> pieces(given(argv[16]), size_t(count) * s.max_pieces);
    Output<vx_label_info> info(given(argv[17]), count);
    if (too_short(raw, count, lo_stride, "lo.bin")) return 1;
    if (const char* refused = vxb::check_label(raw.data(), lo_stride, count, &s, fields.data(), field_stride, pieces.data(), info.data())) return refuse(refused);
    with_format(svo_type, [&](auto format) {
        vxb::label_boxes<decltype(format)::value>(w, raw.data(), lo_stride, count, s, fields.data(), field_stride, pieces.data(), info.data());
    });
    return fields.write(argv[15]) && pieces.write(argv[16]) && info.write(argv[17]) ? 0 : 1;
}

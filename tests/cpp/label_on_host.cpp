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
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "vx_label.hpp"

namespace {

// vx_blocks.hpp's reader over a byte vector: a dword or a byte that does not lie wholly inside it reads 0
struct HostWorld {
    const uint8_t* bytes;
    uint64_t size;
    uint32_t u32_at(uint64_t off) const {
        uint32_t v = 0;
        if (off + 4 <= size) std::memcpy(&v, bytes + off, 4);
        return v;
    }
    uint32_t head() const { return u32_at(0); }
    uint32_t root_ptr() const { return u32_at(4); }
    uint32_t word(uint32_t i) const { return u32_at(4ull + 4ull * i); }
    uint32_t c32(uint32_t p) const { return u32_at(8ull + p); }
    uint32_t c8(uint32_t p) const { return 8ull + p < size ? bytes[8ull + p] : 0u; }
};

bool read_file(const char* path, std::vector<uint8_t>& out) {
    std::ifstream f(path, std::ios::binary | std::ios::ate);
    if (!f) return false;
    const std::streamsize n = f.tellg();
    f.seekg(0);
    out.resize(size_t(n));  // (exactly the file's size: the sanitizer's red zone starts at its end)
    return n == 0 || bool(f.read(reinterpret_cast<char*>(out.data()), n));
}

bool write_file(const char* path, const void* data, size_t bytes) {
    std::ofstream f(path, std::ios::binary);
    return f && (bytes == 0 || bool(f.write(static_cast<const char*>(data), std::streamsize(bytes))));
}

int usage() {
    std::fprintf(stderr, "usage: label_on_host <svo_type> <world.bin> label <lo.bin> <lo_stride> <count> <size x y z> <anchor_faces> <max_pieces> <max_steps> "
                         "<pass_value> <field_stride> <fields.bin | -> <pieces.bin | -> <info.bin | ->\n       label_on_host rules\n");
    return 2;
}

void say(const std::string& what, const char* refused) { std::printf("%s: %s\n", what.c_str(), refused ? refused : "ok"); }

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
    const int svo_type = std::atoi(argv[1]);
    if (svo_type != VX_SVO_ESVO && svo_type != VX_SVO_CSVO) return usage();
    std::vector<uint8_t> world, raw;
    if (!read_file(argv[2], world)) { std::fprintf(stderr, "label_on_host: cannot read %s\n", argv[2]); return 1; }
    if (!read_file(argv[4], raw)) { std::fprintf(stderr, "label_on_host: cannot read %s\n", argv[4]); return 1; }
    const HostWorld w = {world.data(), world.size()};
    const auto u32 = [argv](int i) { return uint32_t(std::strtoul(argv[i], nullptr, 10)); };
    const uint32_t lo_stride = u32(5), count = u32(6), field_stride = u32(14);
    const vx_label_shape s = {{u32(7), u32(8), u32(9)}, u32(10), u32(11), u32(12), u32(13), 0u};
    const bool want_fields = std::strcmp(argv[15], "-") != 0, want_pieces = std::strcmp(argv[16], "-") != 0, want_info = std::strcmp(argv[17], "-") != 0;
    // (the shape's own rules first, on one box and a record that lies apart: the sizes below come from a shape that has passed them; the
    // whole call's rules again below, on the blocks it writes to)
    alignas(16) static uint8_t apart[32];
    if (const char* refused = vxb::check_label(raw.data(), 12, (count && raw.size() >= 12) ? 1u : 0u, &s, nullptr, 0, nullptr, apart)) {
        std::fprintf(stderr, "label_on_host: %s\n", refused);
        return 1;
    }
    if (count > vxb::kLabelMaxCount) { std::fprintf(stderr, "label_on_host: count exceeds 1048576 (2^20)\n"); return 1; }
    if (field_stride % 16u) { std::fprintf(stderr, "label_on_host: field_stride must be 0, or a multiple of 16\n"); return 1; }
    const size_t packed = vxb::flood_round16(vxb::label_voxels(s)), stride = field_stride ? field_stride : packed;
    // exactly up to the last byte the call may write: the last query's rounded voxel count, not its whole stride
    const size_t field_bytes = want_fields && count ? size_t(count - 1u) * stride + packed : 0u;
    std::vector<uint8_t> fields(field_bytes, uint8_t(0x5a));
    std::vector<vx_label_piece> pieces(want_pieces ? size_t(count) * s.max_pieces : 0u);
    std::vector<vx_label_info> info(want_info ? count : 0u);
    if (!pieces.empty()) std::memset(pieces.data(), 0x5a, pieces.size() * sizeof(vx_label_piece));
    if (!info.empty()) std::memset(info.data(), 0x5a, info.size() * sizeof(vx_label_info));
    if (count && raw.size() < size_t(count - 1u) * lo_stride + 12u) { std::fprintf(stderr, "label_on_host: lo.bin is too short\n"); return 1; }
    uint8_t* const f = want_fields ? fields.data() : nullptr;
    vx_label_piece* const p = want_pieces ? pieces.data() : nullptr;
    vx_label_info* const r = want_info ? info.data() : nullptr;
    if (const char* refused = vxb::check_label(raw.data(), lo_stride, count, &s, f, field_stride, p, r)) {
        std::fprintf(stderr, "label_on_host: %s\n", refused);
        return 1;
    }
    if (svo_type == VX_SVO_CSVO) vxb::label_boxes<vxb::kCsvo>(w, raw.data(), lo_stride, count, s, f, field_stride, p, r);
    else vxb::label_boxes<vxb::kEsvo>(w, raw.data(), lo_stride, count, s, f, field_stride, p, r);
    if (want_fields) {  // (written out at the whole stride: the tail of the last query as the sentinel)
        fields.resize(size_t(count) * stride, uint8_t(0x5a));
        if (!write_file(argv[15], fields.data(), fields.size())) return 1;
    }
    if (want_pieces && !write_file(argv[16], pieces.data(), pieces.size() * sizeof(vx_label_piece))) return 1;
    if (want_info && !write_file(argv[17], info.data(), info.size() * sizeof(vx_label_info))) return 1;
    return 0;
}

// TEST HARNESS ONLY: vx_overlap_boxes' answer (voxel-rs_amd/csrc/blocks/vx_boxes.hpp) compiled for the host, as a stand-alone program -- the
// whole call on one thread, box by box and brick by brick as the kernel runs it, with a loop where the kernel shuffles -- over a world frame
// read from a file into a heap block of exactly its size (every read range-checked, as the device's buffer resource checks it; a sanitizer
// build of this program sees any that is not), the boxes' vectors read through their strides from a heap block of exactly the input file's
// size, into a heap block of exactly `count` records. tests/test_boxes_on_host.py runs it, plain and built with -fsanitize=address,undefined
// -fsanitize=float-cast-overflow (the float-to-integer conversions of the cover); tests/test_boxes.py holds the GPU's records against its
// output. Never linked into the product libraries; the product has no CPU path.
//
//   boxes_on_host <svo_type> <world.bin> boxes <raw.bin> <count> <origin_at> <origin_stride> <offset_at> <offset_stride> <extents_at>
//                 <extents_stride> <only_value> <out.bin>
//                                  the vectors lie in raw.bin from byte *_at on (offset_at -1: no offset, a null pointer)
//                                  -> out.bin: `count` vx_box_hit records
//   boxes_on_host rules            prints what check_boxes refuses
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "vx_boxes.hpp"

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

int usage() {
    std::fprintf(stderr, "usage: boxes_on_host <svo_type> <world.bin> boxes <raw.bin> <count> <origin_at> <origin_stride> <offset_at> <offset_stride> "
                         "<extents_at> <extents_stride> <only_value> <out.bin>\n       boxes_on_host rules\n");
    return 2;
}

void say(const char* what, const char* refused) { std::printf("%s: %s\n", what, refused ? refused : "ok"); }

int rules() {
    alignas(16) static float v[64];
    static vx_box_hit out[2];
    const unsigned char* bytes = reinterpret_cast<const unsigned char*>(v);
    const vx_box_batch ok = {v, v + 3, v + 6, 12, 12, 12, 0};
    say("packed", vxb::check_boxes(&ok, 2, out));
    vx_box_batch b = ok;
    b.offset = nullptr, b.offset_stride = 7;  // (a stride nobody steps by)
    say("no offset", vxb::check_boxes(&b, 2, out));
    b = ok, b.offset_stride = b.extents_stride = 0;
    say("one offset, one extents", vxb::check_boxes(&b, 2, out));
    b = ok, b.origin_stride = b.offset_stride = b.extents_stride = 64, b.only_value = 0xffffffffu;
    say("entities", vxb::check_boxes(&b, 1u << 24, out));
    say("count 0", vxb::check_boxes(nullptr, 0, nullptr));
    say("too many", vxb::check_boxes(&ok, (1u << 24) + 1u, out));
    say("null boxes", vxb::check_boxes(nullptr, 1, out));
    say("null out", vxb::check_boxes(&ok, 1, nullptr));
    b = ok, b.origin = nullptr;
    say("null origin", vxb::check_boxes(&b, 1, out));
    b = ok, b.extents = nullptr;
    say("null extents", vxb::check_boxes(&b, 1, out));
    for (uint32_t stride : {0u, 4u, 8u, 13u, 14u}) {
        b = ok, b.origin_stride = stride;
        say(("origin_stride " + std::to_string(stride)).c_str(), vxb::check_boxes(&b, 1, out));
    }
    for (uint32_t stride : {4u, 8u, 13u, 18u}) {
        b = ok, b.offset_stride = stride;
        say(("offset_stride " + std::to_string(stride)).c_str(), vxb::check_boxes(&b, 1, out));
        b = ok, b.extents_stride = stride;
        say(("extents_stride " + std::to_string(stride)).c_str(), vxb::check_boxes(&b, 1, out));
    }
    for (int off : {1, 2, 3}) {
        b = ok, b.origin = bytes + off;
        say(("origin + " + std::to_string(off)).c_str(), vxb::check_boxes(&b, 1, out));
        b = ok, b.offset = bytes + 12 + off;
        say(("offset + " + std::to_string(off)).c_str(), vxb::check_boxes(&b, 1, out));
        b = ok, b.extents = bytes + 24 + off;
        say(("extents + " + std::to_string(off)).c_str(), vxb::check_boxes(&b, 1, out));
    }
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc == 2 && !std::strcmp(argv[1], "rules")) return rules();
    if (argc != 14 || std::strcmp(argv[3], "boxes")) return usage();
    const int svo_type = std::atoi(argv[1]);
    if (svo_type != VX_SVO_ESVO && svo_type != VX_SVO_CSVO) return usage();
    std::vector<uint8_t> world, raw;
    if (!read_file(argv[2], world)) { std::fprintf(stderr, "boxes_on_host: cannot read %s\n", argv[2]); return 1; }
    if (!read_file(argv[4], raw)) { std::fprintf(stderr, "boxes_on_host: cannot read %s\n", argv[4]); return 1; }
    const HostWorld w = {world.data(), world.size()};
    const uint32_t count = uint32_t(std::strtoul(argv[5], nullptr, 10));
    const long long origin_at = std::atoll(argv[6]), offset_at = std::atoll(argv[8]), extents_at = std::atoll(argv[10]);
    vx_box_batch b = {};
    b.origin = raw.data() + origin_at;
    b.offset = offset_at < 0 ? nullptr : raw.data() + offset_at;
    b.extents = raw.data() + extents_at;
    b.origin_stride = uint32_t(std::strtoul(argv[7], nullptr, 10));
    b.offset_stride = uint32_t(std::strtoul(argv[9], nullptr, 10));
    b.extents_stride = uint32_t(std::strtoul(argv[11], nullptr, 10));
    b.only_value = uint32_t(std::strtoul(argv[12], nullptr, 10));
    std::vector<vx_box_hit> out(count);  // (exactly `count` records: a record written beyond them is a heap overflow)
    if (const char* refused = vxb::check_boxes(&b, count, out.data())) { std::fprintf(stderr, "boxes_on_host: %s\n", refused); return 1; }
    if (count) std::memset(out.data(), 0x5a, out.size() * sizeof(vx_box_hit));
    if (svo_type == VX_SVO_CSVO) vxb::overlap_boxes<vxb::kCsvo>(w, b, count, out.data());
    else vxb::overlap_boxes<vxb::kEsvo>(w, b, count, out.data());
    std::ofstream f(argv[13], std::ios::binary);
    if (!f) return 1;
    if (count && !f.write(reinterpret_cast<const char*>(out.data()), std::streamsize(out.size() * sizeof(vx_box_hit)))) return 1;
    return 0;
}

// TEST HARNESS ONLY: vx_light_boxes' answer (voxel-rs_amd/csrc/blocks/vx_light.hpp) compiled for the host, as a stand-alone program -- the
// whole call on one thread, box by box: the bricks, columns, rows and steps the kernel's workgroup walks, with loops where the kernel has
// threads -- over a world frame read from a file into a heap block of exactly its size (every read range-checked, as the device's buffer
// resource checks it; a sanitizer build of this program sees any that is not), the boxes read through their stride from a heap block of
// exactly the input file's size, the props from a heap block of exactly props_count bytes, into heap blocks of exactly the bytes the call may
// write. tests/test_light_on_host.py runs it, plain and built with -fsanitize=address,undefined; tests/test_light.py holds the GPU's bytes
// against its output. Never linked into the product libraries; the product has no CPU path.
//
//   light_on_host <svo_type> <world.bin> light <lo.bin> <lo_stride> <count> <size.x> <size.y> <size.z> <flags> <props.bin | -> <field_stride>
//                 <fields.bin | -> <info.bin | ->
//                                  -> props.bin: the table, its size props_count ("-": null props, props_count 0); fields.bin: count *
//                                  field_stride bytes (field_stride 0: the voxel count rounded up to 16), what the call leaves untouched 0x5a;
//                                  info.bin: `count` vx_light_info records; "-": that output is null
//   light_on_host rules            prints what check_light refuses
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "vx_light.hpp"

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
    std::fprintf(stderr, "usage: light_on_host <svo_type> <world.bin> light <lo.bin> <lo_stride> <count> <size x y z> <flags> <props.bin | -> <field_stride> "
                         "<fields.bin | -> <info.bin | ->\n       light_on_host rules\n");
    return 2;
}

void say(const std::string& what, const char* refused) { std::printf("%s: %s\n", what.c_str(), refused ? refused : "ok"); }

int rules() {
    alignas(16) static int32_t v[64];
    static uint8_t fields[16], table[4097];
    static vx_light_info info[2];
    const unsigned char* bytes = reinterpret_cast<const unsigned char*>(v);
    table[3] = 0x1f;
    const vx_light_shape ok = {{16, 16, 16}, 0, table, 16};
    const auto check = [&](const vx_light_shape& s, uint32_t count = 1, uint32_t field_stride = 0) { return vxb::check_light(v, 12, count, &s, fields, field_stride, info); };
    say("packed", vxb::check_light(v, 12, 2, &ok, fields, 0, info));
    say("stride 64", vxb::check_light(v, 64, 1, &ok, fields, 0, info));
    say("fields only", vxb::check_light(v, 12, 2, &ok, fields, 0, nullptr));
    say("info only", vxb::check_light(v, 12, 2, &ok, nullptr, 0, info));
    say("info only, any stride", vxb::check_light(v, 12, 1u << 24, &ok, nullptr, 7, info));
    say("count 0", vxb::check_light(nullptr, 0, 0, nullptr, nullptr, 0, nullptr));
    say("too many", vxb::check_light(v, 12, (1u << 24) + 1u, &ok, nullptr, 0, info));
    say("null shape", vxb::check_light(v, 12, 1, nullptr, fields, 0, info));
    say("null lo", vxb::check_light(nullptr, 12, 1, &ok, fields, 0, info));
    say("no output", vxb::check_light(v, 12, 1, &ok, nullptr, 0, nullptr));
    for (uint32_t stride : {0u, 4u, 8u, 13u, 14u}) say("lo_stride " + std::to_string(stride), vxb::check_light(v, stride, 1, &ok, fields, 0, info));
    for (int off : {1, 2, 3}) say("lo + " + std::to_string(off), vxb::check_light(bytes + off, 12, 1, &ok, fields, 0, info));
    vx_light_shape s = ok;
    for (int a = 0; a < 3; ++a)
        for (uint32_t side : {0u, 49u, 0xffffffffu}) {
            s = ok, s.size[a] = side;
            say("size[" + std::to_string(a) + "] " + std::to_string(side), check(s));
        }
    s = ok, s.size[0] = s.size[1] = s.size[2] = 48;
    say("largest box", check(s));
    s = ok, s.size[0] = s.size[1] = s.size[2] = 1;
    say("smallest box", check(s));
    for (uint32_t flags : {1u, 2u, 3u, 4u, 0x80000000u}) {
        s = ok, s.flags = flags;
        say("flags " + std::to_string(flags), check(s));
    }
    s = ok, s.props_count = 4096;
    say("props_count 4096", check(s));
    s = ok, s.props_count = 4097;
    say("props_count 4097", check(s));
    s = ok, s.props = nullptr;
    say("null props", check(s));
    s = ok, s.props = nullptr, s.props_count = 0;
    say("no props", check(s));
    for (uint32_t bad : {0x20u, 0x40u, 0x80u}) {
        table[9] = uint8_t(bad | 0x1fu);
        say("props byte " + std::to_string(bad), check(ok));
        s = ok, s.props_count = 9;
        say("props byte " + std::to_string(bad) + " behind props_count", check(s));
    }
    table[9] = 0;
    for (uint32_t stride : {4097u, 4104u, 4080u, 4096u, 4112u, 16u, 8192u}) say("field_stride " + std::to_string(stride), check(ok, 1, stride));
    say("field bytes 2^24", check(ok, 2048, 8192));
    say("field bytes 2^24 + 8192", check(ok, 2049, 8192));
    s = ok, s.size[0] = s.size[1] = s.size[2] = 46;
    say("151 boxes of 46^3", check(s, 151));  // (46^3 = 97,336, rounded up 97,344: 172 of them fit, the benchmark's 151 among them)
    say("172 boxes of 46^3", check(s, 172));
    say("173 boxes of 46^3", check(s, 173));
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc == 2 && !std::strcmp(argv[1], "rules")) return rules();
    if (argc != 15 || std::strcmp(argv[3], "light")) return usage();
    const int svo_type = std::atoi(argv[1]);
    if (svo_type != VX_SVO_ESVO && svo_type != VX_SVO_CSVO) return usage();
    std::vector<uint8_t> world, raw, table;
    if (!read_file(argv[2], world)) { std::fprintf(stderr, "light_on_host: cannot read %s\n", argv[2]); return 1; }
    if (!read_file(argv[4], raw)) { std::fprintf(stderr, "light_on_host: cannot read %s\n", argv[4]); return 1; }
    const bool has_props = std::strcmp(argv[11], "-") != 0;
    if (has_props && !read_file(argv[11], table)) { std::fprintf(stderr, "light_on_host: cannot read %s\n", argv[11]); return 1; }
    const HostWorld w = {world.data(), world.size()};
    const auto u32 = [argv](int i) { return uint32_t(std::strtoul(argv[i], nullptr, 10)); };
    const uint32_t lo_stride = u32(5), count = u32(6), field_stride = u32(12);
    const vx_light_shape s = {{u32(7), u32(8), u32(9)}, u32(10), has_props ? table.data() : nullptr, uint32_t(table.size())};
    const bool want_fields = std::strcmp(argv[13], "-") != 0, want_info = std::strcmp(argv[14], "-") != 0;
    std::vector<vx_light_info> info(want_info ? count : 0u);
    // (a one-byte block stands in for an output that has no byte to receive: never written, never null by accident)
    uint8_t none = 0;
    if (const char* refused = vxb::check_light(raw.data(), lo_stride, count, &s, want_fields ? &none : nullptr, field_stride, want_info ? &none : nullptr)) {
        std::fprintf(stderr, "light_on_host: %s\n", refused);
        return 1;
    }
    const size_t packed = vxb::light_round16(vxb::light_voxels(s.size)), stride = field_stride ? field_stride : packed;
    // exactly up to the last byte the call may write: the last query's rounded voxel count, not its whole stride
    const size_t field_bytes = want_fields && count ? size_t(count - 1u) * stride + packed : 0u;
    std::vector<uint8_t> fields(field_bytes, uint8_t(0x5a));
    if (want_info && count) std::memset(info.data(), 0x5a, info.size() * sizeof(vx_light_info));
    if (count && raw.size() < size_t(count - 1u) * lo_stride + 12u) { std::fprintf(stderr, "light_on_host: lo.bin is too short\n"); return 1; }
    uint8_t* const f = want_fields ? fields.data() : nullptr;
    vx_light_info* const r = want_info ? info.data() : nullptr;
    if (svo_type == VX_SVO_CSVO) vxb::light_boxes<vxb::kCsvo>(w, raw.data(), lo_stride, count, s, f, field_stride, r);
    else vxb::light_boxes<vxb::kEsvo>(w, raw.data(), lo_stride, count, s, f, field_stride, r);
    if (want_fields) {  // (written out at the whole stride: the tail of the last query as the sentinel)
        fields.resize(size_t(count) * stride, uint8_t(0x5a));
        if (!write_file(argv[13], fields.data(), fields.size())) return 1;
    }
    if (want_info && !write_file(argv[14], info.data(), info.size() * sizeof(vx_light_info))) return 1;
    return 0;
}

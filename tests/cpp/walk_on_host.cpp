// TEST HARNESS ONLY: vx_walk_points' answer (voxel-rs_amd/csrc/blocks/vx_walk.hpp) compiled for the host, as a stand-alone program -- the
// whole call on one thread, query by query: the bricks, rows, steps and back-trace candidates the kernel's workgroup walks, with loops where
// the kernel has threads -- over a world frame read from a file into a heap block of exactly its size (every read range-checked, as the
// device's buffer resource checks it; a sanitizer build of this program sees any that is not), the positions and goals read through their
// strides from heap blocks of exactly the input files' sizes, into heap blocks of exactly the bytes the call may write.
// tests/test_walk_on_host.py runs it, plain and built with -fsanitize=address,undefined; tests/test_walk.py holds the GPU's bytes against its
// output. Never linked into the product libraries; the product has no CPU path.
//
//   walk_on_host <svo_type> <world.bin> walk <points.bin> <pos_stride> <goals.bin | -> <goal_stride> <count> <size.x> <size.y> <size.z>
//                <seed_at.x> <seed_at.y> <seed_at.z> <max_steps> <pass_value> <height> <climb> <drop> <path_capacity> <flags> <field_stride>
//                <fields.bin | -> <paths.bin | -> <info.bin | ->
//                                  -> fields.bin: count * field_stride bytes (field_stride 0: the voxel count rounded up to 16), what the call
//                                  leaves untouched 0x5a; paths.bin: count * path_capacity uint32; info.bin: `count` vx_walk_info records;
//                                  "-": that input or output is null
//   walk_on_host rules             prints what check_walk refuses
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "vx_walk.hpp"

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
    std::fprintf(stderr, "usage: walk_on_host <svo_type> <world.bin> walk <points.bin> <pos_stride> <goals.bin | -> <goal_stride> <count> <size x y z> <seed_at x y z> "
                         "<max_steps> <pass_value> <height> <climb> <drop> <path_capacity> <flags> <field_stride> <fields.bin | -> <paths.bin | -> <info.bin | ->\n"
                         "       walk_on_host rules\n");
    return 2;
}

void say(const std::string& what, const char* refused) { std::printf("%s: %s\n", what.c_str(), refused ? refused : "ok"); }

int rules() {
    alignas(16) static float v[64];
    static uint8_t fields[2 * 32768];
    static uint32_t paths[2 * 252];
    static vx_walk_info info[2];
    const unsigned char* bytes = reinterpret_cast<const unsigned char*>(v);
    const vx_walk_shape ok = {{17, 12, 17}, {8, 6, 8}, 250, 0, 2, 1, 3, 252, 0};  // 3,468 voxels: 3,472 bytes a field
    const auto check = [&](const vx_walk_shape& s) { return vxb::check_walk(v, 12, v, 12, 1, &s, fields, 0, paths, info); };
    say("packed", vxb::check_walk(v, 12, v, 12, 2, &ok, fields, 0, paths, info));
    say("entities", vxb::check_walk(v, 64, v, 64, 1, &ok, fields, 0, paths, info));
    say("one goal", vxb::check_walk(v, 12, v, 0, 2, &ok, fields, 0, paths, info));
    say("no goal", vxb::check_walk(v, 12, nullptr, 0, 2, &ok, fields, 0, nullptr, info));
    say("no goal, any goal_stride", vxb::check_walk(v, 12, nullptr, 7, 2, &ok, fields, 0, nullptr, info));
    say("fields only", vxb::check_walk(v, 12, v, 12, 2, &ok, fields, 0, nullptr, nullptr));
    say("info only", vxb::check_walk(v, 12, v, 12, 2, &ok, nullptr, 0, nullptr, info));
    say("paths only", vxb::check_walk(v, 12, v, 12, 2, &ok, nullptr, 0, paths, nullptr));
    say("info only, any stride", vxb::check_walk(v, 12, v, 12, 1u << 24, &ok, nullptr, 7, nullptr, info));
    say("count 0", vxb::check_walk(nullptr, 0, nullptr, 0, 0, nullptr, nullptr, 0, nullptr, nullptr));
    say("too many", vxb::check_walk(v, 12, v, 12, (1u << 24) + 1u, &ok, nullptr, 0, nullptr, info));
    say("null shape", vxb::check_walk(v, 12, v, 12, 1, nullptr, fields, 0, paths, info));
    say("null pos", vxb::check_walk(nullptr, 12, v, 12, 1, &ok, fields, 0, paths, info));
    say("no output", vxb::check_walk(v, 12, v, 12, 1, &ok, nullptr, 0, nullptr, nullptr));
    say("paths without goal", vxb::check_walk(v, 12, nullptr, 0, 1, &ok, fields, 0, paths, info));
    for (uint32_t stride : {0u, 4u, 8u, 13u, 14u}) say("pos_stride " + std::to_string(stride), vxb::check_walk(v, stride, v, 12, 1, &ok, fields, 0, paths, info));
    for (int off : {1, 2, 3}) say("pos + " + std::to_string(off), vxb::check_walk(bytes + off, 12, v, 12, 1, &ok, fields, 0, paths, info));
    for (uint32_t stride : {4u, 8u, 13u, 14u, 16u}) say("goal_stride " + std::to_string(stride), vxb::check_walk(v, 12, v, stride, 1, &ok, fields, 0, paths, info));
    for (int off : {1, 2, 3}) say("goal + " + std::to_string(off), vxb::check_walk(v, 12, bytes + off, 12, 1, &ok, fields, 0, paths, info));
    vx_walk_shape s = ok;
    for (int a = 0; a < 3; ++a)
        for (uint32_t side : {0u, 33u, 0xffffffffu}) {
            s = ok, s.size[a] = side, s.seed_at[a] = 0;
            say("size[" + std::to_string(a) + "] " + std::to_string(side), check(s));
        }
    for (int a = 0; a < 3; ++a) {
        s = ok, s.seed_at[a] = 17;
        say("seed_at[" + std::to_string(a) + "] 17", check(s));
    }
    for (uint32_t h : {0u, 1u, 4u, 5u, 0xffffffffu}) {
        s = ok, s.height = h;
        say("height " + std::to_string(h), check(s));
    }
    s = ok, s.size[1] = 31, s.height = 1;
    say("31 layers and 1", check(s));
    s = ok, s.size[1] = 31, s.height = 2;
    say("31 layers and 2", check(s));
    s = ok, s.size[1] = 28, s.height = 4;
    say("28 layers and 4", check(s));
    s = ok, s.size[1] = 32, s.height = 1;
    say("32 layers and 1", check(s));
    s = ok, s.size[0] = s.size[2] = 32, s.size[1] = 28, s.height = 4, s.seed_at[0] = s.seed_at[2] = 31, s.seed_at[1] = 27;
    say("largest box", check(s));
    s = ok, s.size[0] = s.size[1] = s.size[2] = 1, s.seed_at[0] = s.seed_at[1] = s.seed_at[2] = 0, s.max_steps = 0, s.height = 1, s.climb = 0, s.drop = 0, s.path_capacity = 0;
    say("smallest box", check(s));
    s = ok, s.max_steps = 251;
    say("max_steps 251", check(s));
    for (uint32_t c : {0u, 1u, 2u, 0xffffffffu}) {
        s = ok, s.climb = c;
        say("climb " + std::to_string(c), check(s));
    }
    for (uint32_t d : {0u, 3u, 4u, 0xffffffffu}) {
        s = ok, s.drop = d;
        say("drop " + std::to_string(d), check(s));
    }
    for (uint32_t c : {0u, 4u, 6u, 252u, 253u, 256u}) {
        s = ok, s.path_capacity = c;
        say("path_capacity " + std::to_string(c), check(s));
    }
    for (uint32_t flags : {1u, 2u, 3u, 0x80000000u}) {
        s = ok, s.flags = flags;
        say("flags " + std::to_string(flags), check(s));
    }
    s = ok, s.pass_value = 0xffffffffu;
    say("any pass_value", check(s));
    for (uint32_t stride : {3468u, 3470u, 3456u, 3472u, 16u, 4096u}) say("field_stride " + std::to_string(stride), vxb::check_walk(v, 12, v, 12, 1, &ok, fields, stride, paths, info));
    say("field bytes 2^24", vxb::check_walk(v, 12, v, 12, 4096, &ok, fields, 4096, nullptr, info));
    say("field bytes 2^24 + 4096", vxb::check_walk(v, 12, v, 12, 4097, &ok, fields, 4096, nullptr, info));
    say("field bytes by the default stride", vxb::check_walk(v, 12, v, 12, 4833, &ok, fields, 0, nullptr, info));  // (4,833 * 3,472 > 2^24 >= 4,832 * 3,472)
    say("field bytes by the default stride, one fewer", vxb::check_walk(v, 12, v, 12, 4832, &ok, fields, 0, nullptr, info));
    say("path bytes 2^24", vxb::check_walk(v, 12, v, 12, 16644, &ok, nullptr, 0, paths, info));  // (16,644 * 1,008 <= 2^24 < 16,645 * 1,008)
    say("path bytes beyond 2^24", vxb::check_walk(v, 12, v, 12, 16645, &ok, nullptr, 0, paths, info));
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc == 2 && !std::strcmp(argv[1], "rules")) return rules();
    if (argc != 26 || std::strcmp(argv[3], "walk")) return usage();
    const int svo_type = std::atoi(argv[1]);
    if (svo_type != VX_SVO_ESVO && svo_type != VX_SVO_CSVO) return usage();
    const bool want_goals = std::strcmp(argv[6], "-") != 0;
    std::vector<uint8_t> world, raw, goals;
    if (!read_file(argv[2], world)) { std::fprintf(stderr, "walk_on_host: cannot read %s\n", argv[2]); return 1; }
    if (!read_file(argv[4], raw)) { std::fprintf(stderr, "walk_on_host: cannot read %s\n", argv[4]); return 1; }
    if (want_goals && !read_file(argv[6], goals)) { std::fprintf(stderr, "walk_on_host: cannot read %s\n", argv[6]); return 1; }
    const HostWorld w = {world.data(), world.size()};
    const auto u32 = [argv](int i) { return uint32_t(std::strtoul(argv[i], nullptr, 10)); };
    const uint32_t pos_stride = u32(5), goal_stride = u32(7), count = u32(8), field_stride = u32(22);
    const vx_walk_shape s = {{u32(9), u32(10), u32(11)}, {u32(12), u32(13), u32(14)}, u32(15), u32(16), u32(17), u32(18), u32(19), u32(20), u32(21)};
    const bool want_fields = std::strcmp(argv[23], "-") != 0, want_paths = std::strcmp(argv[24], "-") != 0, want_info = std::strcmp(argv[25], "-") != 0;
    // (a one-byte block stands in for an output that has no byte to receive: never written, never null by accident)
    uint8_t none = 0;
    if (const char* refused = vxb::check_walk(raw.data(), pos_stride, want_goals ? goals.data() : nullptr, goal_stride, count, &s, want_fields ? &none : nullptr, field_stride,
                                              want_paths ? &none : nullptr, want_info ? &none : nullptr)) {
        std::fprintf(stderr, "walk_on_host: %s\n", refused);
        return 1;
    }
    const size_t stride = field_stride ? field_stride : vxb::flood_round16(vxb::walk_voxels(s));
    // exactly up to the last byte the call may write: the last query's rounded voxel count, not its whole stride
    const size_t field_bytes = want_fields && count ? size_t(count - 1u) * stride + vxb::flood_round16(vxb::walk_voxels(s)) : 0u;
    std::vector<uint8_t> fields(field_bytes, uint8_t(0x5a));
    std::vector<uint32_t> paths(want_paths ? size_t(count) * s.path_capacity : 0u, 0x5a5a5a5au);
    std::vector<vx_walk_info> info(want_info ? count : 0u);
    if (want_info && count) std::memset(info.data(), 0x5a, info.size() * sizeof(vx_walk_info));
    if (count && raw.size() < size_t(count - 1u) * pos_stride + 12u) { std::fprintf(stderr, "walk_on_host: points.bin is too short\n"); return 1; }
    if (count && want_goals && goals.size() < size_t(count - 1u) * goal_stride + 12u) { std::fprintf(stderr, "walk_on_host: goals.bin is too short\n"); return 1; }
    uint8_t* const f = want_fields ? fields.data() : nullptr;
    uint32_t* const p = want_paths ? paths.data() : nullptr;
    vx_walk_info* const r = want_info ? info.data() : nullptr;
    const uint8_t* const g = want_goals ? goals.data() : nullptr;
    if (svo_type == VX_SVO_CSVO) vxb::walk_points<vxb::kCsvo>(w, raw.data(), pos_stride, g, goal_stride, count, s, f, field_stride, p, r);
    else vxb::walk_points<vxb::kEsvo>(w, raw.data(), pos_stride, g, goal_stride, count, s, f, field_stride, p, r);
    if (want_fields) {  // (written out at the whole stride: the tail of the last query as the sentinel)
        fields.resize(size_t(count) * stride, uint8_t(0x5a));
        if (!write_file(argv[23], fields.data(), fields.size())) return 1;
    }
    if (want_paths && !write_file(argv[24], paths.data(), paths.size() * 4u)) return 1;
    if (want_info && !write_file(argv[25], info.data(), info.size() * sizeof(vx_walk_info))) return 1;
    return 0;
}

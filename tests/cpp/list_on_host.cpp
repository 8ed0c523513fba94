// TEST HARNESS ONLY: vx_list_region's list (voxel-rs_amd/csrc/blocks/vx_list.hpp) compiled for the host, as a stand-alone program -- the
// whole call on one thread, count, prefix and write, brick by brick as the kernels run it, with array indexing where the kernel shuffles --
// over a world frame read from a file into a heap block of exactly its size (every read range-checked, as the device's buffer resource checks
// it; a sanitizer build of this program sees any that is not), into a heap block of exactly `capacity` records. tests/test_list_on_host.py
// runs it; tests/test_list.py holds the GPU's records against its output. Never linked into the product libraries; the product has no CPU
// path.
//
//   list_on_host <svo_type> <world.bin> list <lox> <loy> <loz> <sx> <sy> <sz> <flags> <capacity> <out.bin>
//                                  -> out.bin: uint32 total, uint32 bricks, then the `capacity` records of the buffer, which was filled with
//                                     0x5a before the call (so what the call left alone can be seen)
//   list_on_host rules             prints what check_list refuses
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "vx_list.hpp"

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
    std::fprintf(stderr, "usage: list_on_host <svo_type> <world.bin> list <lox> <loy> <loz> <sx> <sy> <sz> <flags> <capacity> <out.bin>\n"
                         "       list_on_host rules\n");
    return 2;
}

void say(const char* what, const char* refused) { std::printf("%s: %s\n", what, refused ? refused : "ok"); }

int rules() {
    static vx_block_at out[2];
    static uint32_t total;
    const int32_t lo[3] = {-3, 0, 5};
    const uint32_t ok[3] = {256, 256, 256}, big[3] = {256, 256, 257}, line[3] = {1, 1, 1u << 24}, none[3] = {0xffffffffu, 0, 0xffffffffu};
    say("plain", vxb::check_list(lo, ok, 0, out, 2, &total));
    say("faces", vxb::check_list(lo, ok, VX_LIST_FACES, out, 2, &total));
    say("exposed", vxb::check_list(lo, ok, VX_LIST_EXPOSED, out, 2, &total));
    say("exposed faces", vxb::check_list(lo, line, VX_LIST_EXPOSED | VX_LIST_FACES, out, 0xffffffffu, &total));
    say("count only", vxb::check_list(lo, ok, 0, nullptr, 0, &total));
    say("no voxel", vxb::check_list(lo, none, 0, nullptr, 7, nullptr));
    for (uint32_t flags : {4u, 8u, 7u, 0x80000000u, 0xffffffffu}) say(("flags " + std::to_string(flags)).c_str(), vxb::check_list(lo, ok, flags, out, 2, &total));
    say("no voxel, bad flags", vxb::check_list(lo, none, 4, nullptr, 0, nullptr));
    say("too large", vxb::check_list(lo, big, 0, out, 2, &total));
    say("null lo", vxb::check_list(nullptr, ok, 0, out, 2, &total));
    say("null size", vxb::check_list(lo, nullptr, 0, out, 2, &total));
    say("null total", vxb::check_list(lo, ok, 0, out, 2, nullptr));
    say("null total, count only", vxb::check_list(lo, ok, 0, nullptr, 0, nullptr));
    say("null out", vxb::check_list(lo, ok, 0, nullptr, 1, &total));
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc == 2 && !std::strcmp(argv[1], "rules")) return rules();
    if (argc != 13 || std::strcmp(argv[3], "list")) return usage();
    const int svo_type = std::atoi(argv[1]);
    if (svo_type != VX_SVO_ESVO && svo_type != VX_SVO_CSVO) return usage();
    std::vector<uint8_t> world;
    if (!read_file(argv[2], world)) { std::fprintf(stderr, "list_on_host: cannot read %s\n", argv[2]); return 1; }
    const HostWorld w = {world.data(), world.size()};
    int32_t lo[3];
    uint32_t size[3];
    for (int a = 0; a < 3; ++a) {
        lo[a] = int32_t(std::strtol(argv[4 + a], nullptr, 10));
        size[a] = uint32_t(std::strtoul(argv[7 + a], nullptr, 10));
    }
    const uint32_t flags = uint32_t(std::strtoul(argv[10], nullptr, 10)), capacity = uint32_t(std::strtoul(argv[11], nullptr, 10));
    std::vector<vx_block_at> out(capacity);  // (exactly `capacity` records: a record written beyond them is a heap overflow)
    uint32_t total = 0x5a5a5a5au;
    if (const char* refused = vxb::check_list(lo, size, flags, capacity ? out.data() : nullptr, capacity, &total)) { std::fprintf(stderr, "list_on_host: %s\n", refused); return 1; }
    if (capacity) std::memset(out.data(), 0x5a, out.size() * sizeof(vx_block_at));
    const uint64_t bricks = size[0] && size[1] && size[2] ? vxb::region_bricks(vxb::plan_region(lo, size)) : 0;
    std::vector<uint32_t> counts(size_t(bricks) + 1);  // (exactly the workspace the call is given)
    if (bricks == 0) total = 0;
    else if (svo_type == VX_SVO_CSVO) total = vxb::list_region<vxb::kCsvo>(w, lo, size, flags, capacity ? out.data() : nullptr, capacity, counts.data());
    else total = vxb::list_region<vxb::kEsvo>(w, lo, size, flags, capacity ? out.data() : nullptr, capacity, counts.data());
    const uint32_t head[2] = {total, uint32_t(bricks)};
    std::ofstream f(argv[12], std::ios::binary);
    if (!f || !f.write(reinterpret_cast<const char*>(head), sizeof head)) return 1;
    if (capacity && !f.write(reinterpret_cast<const char*>(out.data()), std::streamsize(out.size() * sizeof(vx_block_at)))) return 1;
    return 0;
}

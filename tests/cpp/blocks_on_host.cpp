// TEST HARNESS ONLY: the block lookup of vx_block_points and vx_read_region (voxel-rs_amd/csrc/blocks/vx_blocks.hpp) compiled for the host, as a
// stand-alone program -- the descent a kernel's lane makes and the brick-by-brick region routine, over a world frame read from a file into a heap
// block of exactly its size (every read range-checked, as the device's buffer resource checks it; a sanitizer build of this program sees any
// that is not). tests/test_blocks_on_host.py runs it; tests/test_blocks.py holds the GPU's records against its output. Never linked into the
// product libraries; the product has no CPU path.
//
//   blocks_on_host <svo_type> <world.bin> points <points.bin> <stride> <count> <out.bin>     `count` float[3] at `stride` bytes -> vx_block_cell records
//   blocks_on_host <svo_type> <world.bin> region <lox> <loy> <loz> <sx> <sy> <sz> <out.bin>  -> sx * sy * sz uint32, x fastest
//   blocks_on_host rules                                                                       prints what check_points / check_region refuse
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "vx_blocks.hpp"

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
    return f && f.write(static_cast<const char*>(data), std::streamsize(bytes));
}

int usage() {
    std::fprintf(stderr, "usage: blocks_on_host <svo_type> <world.bin> points <points.bin> <stride> <count> <out.bin>\n"
                         "       blocks_on_host <svo_type> <world.bin> region <lox> <loy> <loz> <sx> <sy> <sz> <out.bin>\n"
                         "       blocks_on_host rules\n");
    return 2;
}

void say(const char* what, const char* refused) { std::printf("%s: %s\n", what, refused ? refused : "ok"); }

int rules() {
    alignas(8) static float p[8];
    static vx_block_cell out[2];
    const int32_t lo[3] = {-3, 0, 5};
    const uint32_t ok[3] = {256, 256, 256}, big[3] = {256, 256, 257}, huge[3] = {0xffffffffu, 0xffffffffu, 2}, none[3] = {0xffffffffu, 0, 0xffffffffu};
    say("packed", vxb::check_points(p, 12, 2, out));
    say("entity", vxb::check_points(p, 64, 1u << 24, out));
    say("nothing", vxb::check_points(nullptr, 12, 0, nullptr));
    say("nothing at a bad stride", vxb::check_points(reinterpret_cast<const uint8_t*>(p) + 1, 5, 0, nullptr));
    for (uint32_t stride : {0u, 4u, 8u, 13u, 14u, 18u}) say(("stride " + std::to_string(stride)).c_str(), vxb::check_points(p, stride, 2, out));
    say("misaligned", vxb::check_points(reinterpret_cast<const uint8_t*>(p) + 2, 12, 2, out));
    say("null pos", vxb::check_points(nullptr, 12, 2, out));
    say("null out", vxb::check_points(p, 12, 2, nullptr));
    say("too many", vxb::check_points(p, 12, (1u << 24) + 1, out));
    say("region", vxb::check_region(lo, ok));
    say("region none", vxb::check_region(lo, none));
    say("region big", vxb::check_region(lo, big));
    say("region huge", vxb::check_region(lo, huge));
    say("null lo", vxb::check_region(nullptr, ok));
    say("null size", vxb::check_region(lo, nullptr));
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc == 2 && !std::strcmp(argv[1], "rules")) return rules();
    if (argc < 4) return usage();
    const int svo_type = std::atoi(argv[1]);
    if (svo_type != VX_SVO_ESVO && svo_type != VX_SVO_CSVO) return usage();
    std::vector<uint8_t> world;
    if (!read_file(argv[2], world)) { std::fprintf(stderr, "blocks_on_host: cannot read %s\n", argv[2]); return 1; }
    const HostWorld w = {world.data(), world.size()};

    if (!std::strcmp(argv[3], "points") && argc == 8) {
        std::vector<uint8_t> points;
        if (!read_file(argv[4], points)) { std::fprintf(stderr, "blocks_on_host: cannot read %s\n", argv[4]); return 1; }
        const uint32_t stride = uint32_t(std::strtoul(argv[5], nullptr, 10)), count = uint32_t(std::strtoul(argv[6], nullptr, 10));
        std::vector<vx_block_cell> out(count);
        if (const char* refused = vxb::check_points(points.data(), stride, count, out.data())) { std::fprintf(stderr, "blocks_on_host: %s\n", refused); return 1; }
        if (count && points.size() < size_t(count - 1) * stride + 12) { std::fprintf(stderr, "blocks_on_host: %s is too short\n", argv[4]); return 1; }
        for (uint32_t i = 0; i < count; ++i) {
            float p[3];
            std::memcpy(p, points.data() + size_t(i) * stride, 12);
            out[i] = svo_type == VX_SVO_CSVO ? vxb::cell_at_point<vxb::kCsvo>(w, p) : vxb::cell_at_point<vxb::kEsvo>(w, p);
        }
        return write_file(argv[7], out.data(), out.size() * sizeof(vx_block_cell)) ? 0 : 1;
    }
    if (!std::strcmp(argv[3], "region") && argc == 11) {
        int32_t lo[3];
        uint32_t size[3];
        for (int a = 0; a < 3; ++a) {
            lo[a] = int32_t(std::strtol(argv[4 + a], nullptr, 10));
            size[a] = uint32_t(std::strtoul(argv[7 + a], nullptr, 10));
        }
        if (const char* refused = vxb::check_region(lo, size)) { std::fprintf(stderr, "blocks_on_host: %s\n", refused); return 1; }
        std::vector<uint32_t> out(size_t(size[0]) * size[1] * size[2], 0xdeadbeefu);  // (every voxel of the box has to be written)
        if (svo_type == VX_SVO_CSVO) vxb::read_region<vxb::kCsvo>(w, lo, size, out.data());
        else vxb::read_region<vxb::kEsvo>(w, lo, size, out.data());
        return write_file(argv[10], out.data(), out.size() * 4) ? 0 : 1;
    }
    return usage();
}

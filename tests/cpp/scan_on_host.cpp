// TEST HARNESS ONLY: the scans of vx_scan_points and vx_scan_columns (voxel-rs_amd/csrc/blocks/vx_scan.hpp) compiled for the host, as a
// stand-alone program -- the walk a kernel's lane makes and the tile-by-tile columns routine, over a world frame read from a file into a heap
// block of exactly its size (every read range-checked, as the device's buffer resource checks it; a sanitizer build of this program sees any
// that is not). tests/test_scan_on_host.py runs it; tests/test_scan.py holds the GPU's records against its output. Never linked into the
// product libraries; the product has no CPU path.
//
//   scan_on_host <svo_type> <world.bin> points <points.bin> <stride> <count> <direction> <reach> <out.bin> <trips.bin>
//                                                  `count` float[3] at `stride` bytes -> vx_scan_hit records; uint32 loop trips a point
//   scan_on_host <svo_type> <world.bin> columns <lox> <loy> <loz> <sx> <sy> <sz> <direction> <out.bin> <trips.bin>
//                                                  -> size[u] * size[v] vx_scan_hit records, u fastest; uint32 loop trips a tile
//   scan_on_host rules                             prints what check_scan_points / check_scan_columns refuse
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "vx_scan.hpp"

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
    return f && (bytes == 0 || f.write(static_cast<const char*>(data), std::streamsize(bytes)));
}

int usage() {
    std::fprintf(stderr, "usage: scan_on_host <svo_type> <world.bin> points <points.bin> <stride> <count> <direction> <reach> <out.bin> <trips.bin>\n"
                         "       scan_on_host <svo_type> <world.bin> columns <lox> <loy> <loz> <sx> <sy> <sz> <direction> <out.bin> <trips.bin>\n"
                         "       scan_on_host rules\n");
    return 2;
}

void say(const char* what, const char* refused) { std::printf("%s: %s\n", what, refused ? refused : "ok"); }

int rules() {
    alignas(8) static float p[8];
    static vx_scan_hit out[2];
    const int32_t lo[3] = {-3, 0, 5};
    const uint32_t ok[3] = {4096, 1u << 24, 4096}, wide[3] = {4097, 7, 4096}, none[3] = {0xffffffffu, 0, 0xffffffffu}, flat[3] = {1u << 24, 1, 1},
                   deep[3] = {1, (1u << 24) + 1, 1};
    say("packed", vxb::check_scan_points(p, 12, 2, VX_DIR_NEG_Y, 1, out));
    say("entity", vxb::check_scan_points(p, 64, 1u << 24, VX_DIR_POS_Z, VX_SCAN_TO_EDGE, out));
    say("nothing", vxb::check_scan_points(nullptr, 12, 0, VX_DIR_NEG_X, 0, nullptr));
    say("nothing at a bad stride", vxb::check_scan_points(reinterpret_cast<const uint8_t*>(p) + 1, 5, 0, VX_DIR_NEG_X, 7, nullptr));
    say("nothing in no direction", vxb::check_scan_points(nullptr, 12, 0, 6, 1, nullptr));
    for (uint32_t stride : {0u, 4u, 8u, 13u, 14u, 18u}) say(("stride " + std::to_string(stride)).c_str(), vxb::check_scan_points(p, stride, 2, 0, 1, out));
    say("misaligned", vxb::check_scan_points(reinterpret_cast<const uint8_t*>(p) + 2, 12, 2, 0, 1, out));
    say("null pos", vxb::check_scan_points(nullptr, 12, 2, 0, 1, out));
    say("null out", vxb::check_scan_points(p, 12, 2, 0, 1, nullptr));
    say("too many", vxb::check_scan_points(p, 12, (1u << 24) + 1, 0, 1, out));
    say("no reach", vxb::check_scan_points(p, 12, 2, 0, 0, out));
    for (int d : {-1, 6, 255}) say(("points direction " + std::to_string(d)).c_str(), vxb::check_scan_points(p, 12, 2, d, 1, out));
    say("columns", vxb::check_scan_columns(lo, ok, VX_DIR_NEG_Y));
    say("columns none", vxb::check_scan_columns(lo, none, VX_DIR_NEG_Y));
    say("columns flat", vxb::check_scan_columns(lo, flat, VX_DIR_POS_Z));
    say("columns wide", vxb::check_scan_columns(lo, wide, VX_DIR_POS_Y));
    say("columns wide along x", vxb::check_scan_columns(lo, ok, VX_DIR_NEG_X));
    say("columns deep", vxb::check_scan_columns(lo, deep, VX_DIR_NEG_Y));
    say("columns deep across", vxb::check_scan_columns(lo, deep, VX_DIR_NEG_X));
    for (int d : {-1, 6, 255}) say(("columns direction " + std::to_string(d)).c_str(), vxb::check_scan_columns(lo, ok, d));
    say("null lo", vxb::check_scan_columns(nullptr, ok, 0));
    say("null size", vxb::check_scan_columns(lo, nullptr, 0));
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc == 2 && !std::strcmp(argv[1], "rules")) return rules();
    if (argc < 4) return usage();
    const int svo_type = std::atoi(argv[1]);
    if (svo_type != VX_SVO_ESVO && svo_type != VX_SVO_CSVO) return usage();
    std::vector<uint8_t> world;
    if (!read_file(argv[2], world)) { std::fprintf(stderr, "scan_on_host: cannot read %s\n", argv[2]); return 1; }
    const HostWorld w = {world.data(), world.size()};

    if (!std::strcmp(argv[3], "points") && argc == 11) {
        std::vector<uint8_t> points;
        if (!read_file(argv[4], points)) { std::fprintf(stderr, "scan_on_host: cannot read %s\n", argv[4]); return 1; }
        const uint32_t stride = uint32_t(std::strtoul(argv[5], nullptr, 10)), count = uint32_t(std::strtoul(argv[6], nullptr, 10));
        const int direction = std::atoi(argv[7]);
        const uint32_t reach = uint32_t(std::strtoul(argv[8], nullptr, 10));
        std::vector<vx_scan_hit> out(count);
        std::vector<uint32_t> trips(count);
        std::memset(out.data(), 0x5a, out.size() * sizeof(vx_scan_hit));  // (every record has to be written, its padding too)
        if (const char* refused = vxb::check_scan_points(points.data(), stride, count, direction, reach, out.data())) { std::fprintf(stderr, "scan_on_host: %s\n", refused); return 1; }
        if (count && points.size() < size_t(count - 1) * stride + 12) { std::fprintf(stderr, "scan_on_host: %s is too short\n", argv[4]); return 1; }
        if (svo_type == VX_SVO_CSVO) vxb::scan_points<vxb::kCsvo>(w, points.data(), stride, count, direction, reach, out.data(), trips.data());
        else vxb::scan_points<vxb::kEsvo>(w, points.data(), stride, count, direction, reach, out.data(), trips.data());
        return write_file(argv[9], out.data(), out.size() * sizeof(vx_scan_hit)) && write_file(argv[10], trips.data(), trips.size() * 4) ? 0 : 1;
    }
    if (!std::strcmp(argv[3], "columns") && argc == 13) {
        int32_t lo[3];
        uint32_t size[3];
        for (int a = 0; a < 3; ++a) {
            lo[a] = int32_t(std::strtol(argv[4 + a], nullptr, 10));
            size[a] = uint32_t(std::strtoul(argv[7 + a], nullptr, 10));
        }
        const int direction = std::atoi(argv[10]);
        if (const char* refused = vxb::check_scan_columns(lo, size, direction)) { std::fprintf(stderr, "scan_on_host: %s\n", refused); return 1; }
        const vxb::Columns p = vxb::plan_columns(lo, size, direction);
        const uint64_t tiles = vxb::column_tiles(p);
        std::vector<vx_scan_hit> out(tiles ? size_t(p.size_u) * p.size_v : 0);
        std::vector<uint32_t> trips(size_t(tiles), 0u);
        std::memset(out.data(), 0x5a, out.size() * sizeof(vx_scan_hit));  // (every column of the footprint has to be written)
        if (svo_type == VX_SVO_CSVO) vxb::scan_columns<vxb::kCsvo>(w, lo, size, direction, out.data(), trips.data());
        else vxb::scan_columns<vxb::kEsvo>(w, lo, size, direction, out.data(), trips.data());
        return write_file(argv[11], out.data(), out.size() * sizeof(vx_scan_hit)) && write_file(argv[12], trips.data(), trips.size() * 4) ? 0 : 1;
    }
    return usage();
}

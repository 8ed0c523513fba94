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
#include "on_host.hpp"
#include "vx_scan.hpp"

using namespace on_host;
const char* const on_host::program = "scan_on_host";

namespace {

int usage() {
    std::fprintf(stderr, "usage: scan_on_host <svo_type> <world.bin> points <points.bin> <stride> <count> <direction> <reach> <out.bin> <trips.bin>\n"
                         "       scan_on_host <svo_type> <world.bin> columns <lox> <loy> <loz> <sx> <sy> <sz> <direction> <out.bin> <trips.bin>\n"
                         "       scan_on_host rules\n");
    return 2;
}

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
    const int svo_type = svo_type_of(argv[1]);
    if (svo_type < 0) return usage();
    std::vector<uint8_t> world;
    if (!load(argv[2], world)) return 1;
    const HostWorld w = {world.data(), world.size()};

    if (!std::strcmp(argv[3], "points") && argc == 11) {
        std::vector<uint8_t> points;
        if (!load(argv[4], points)) return 1;
        const uint32_t stride = u32_of(argv[5]), count = u32_of(argv[6]), reach = u32_of(argv[8]);
        const int direction = std::atoi(argv[7]);
        Output<vx_scan_hit> out(true, count);  // (every record has to be written, its padding too)
        std::vector<uint32_t> trips(count);
        if (const char* refused = vxb::check_scan_points(points.data(), stride, count, direction, reach, out.data())) return refuse(refused);
        if (too_short(points, count, stride, argv[4])) return 1;
        with_format(svo_type, [&](auto format) { vxb::scan_points<decltype(format)::value>(w, points.data(), stride, count, direction, reach, out.data(), trips.data()); });
        return out.write(argv[9]) && write_file(argv[10], trips.data(), trips.size() * 4) ? 0 : 1;
    }
    if (!std::strcmp(argv[3], "columns") && argc == 13) {
        int32_t lo[3];
        uint32_t size[3];
        for (int a = 0; a < 3; ++a) lo[a] = i32_of(argv[4 + a]), size[a] = u32_of(argv[7 + a]);
        const int direction = std::atoi(argv[10]);
        if (const char* refused = vxb::check_scan_columns(lo, size, direction)) return refuse(refused);
        const vxb::Columns p = vxb::plan_columns(lo, size, direction);
        const uint64_t tiles = vxb::column_tiles(p);
        Output<vx_scan_hit> out(true, tiles ? size_t(p.size_u) * p.size_v : 0);  // (every column of the footprint has to be written)
        std::vector<uint32_t> trips(size_t(tiles), 0u);
        with_format(svo_type, [&](auto format) { vxb::scan_columns<decltype(format)::value>(w, lo, size, direction, out.data(), trips.data()); });
        return out.write(argv[11]) && write_file(argv[12], trips.data(), trips.size() * 4) ? 0 : 1;
    }
    return usage();
}

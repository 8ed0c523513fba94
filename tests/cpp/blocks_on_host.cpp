// TEST HARNESS ONLY: the block lookup of vx_block_points and vx_read_region (voxel-rs_amd/csrc/blocks/vx_blocks.hpp) compiled for the host, as a
// stand-alone program -- the descent a kernel's lane makes and the brick-by-brick region routine, over a world frame read from a file into a heap
// block of exactly its size (every read range-checked, as the device's buffer resource checks it; a sanitizer build of this program sees any
// that is not). tests/test_blocks_on_host.py runs it; tests/test_blocks.py holds the GPU's records against its output. Never linked into the
// product libraries; the product has no CPU path.
//
//   blocks_on_host <svo_type> <world.bin> points <points.bin> <stride> <count> <out.bin>     `count` float[3] at `stride` bytes -> vx_block_cell records
//   blocks_on_host <svo_type> <world.bin> region <lox> <loy> <loz> <sx> <sy> <sz> <out.bin>  -> sx * sy * sz uint32, x fastest
//   blocks_on_host rules                                                                       prints what check_points / check_region refuse
#include "on_host.hpp"
#include "vx_blocks.hpp"

using namespace on_host;
const char* const on_host::program = "blocks_on_host";

namespace {

int usage() {
    std::fprintf(stderr, "usage: blocks_on_host <svo_type> <world.bin> points <points.bin> <stride> <count> <out.bin>\n"
                         "       blocks_on_host <svo_type> <world.bin> region <lox> <loy> <loz> <sx> <sy> <sz> <out.bin>\n"
                         "       blocks_on_host rules\n");
    return 2;
}

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
    const int svo_type = svo_type_of(argv[1]);
    if (svo_type < 0) return usage();
    std::vector<uint8_t> world;
    if (!load(argv[2], world)) return 1;
    const HostWorld w = {world.data(), world.size()};

    if (!std::strcmp(argv[3], "points") && argc == 8) {
        std::vector<uint8_t> points;
        if (!load(argv[4], points)) return 1;
        const uint32_t stride = u32_of(argv[5]), count = u32_of(argv[6]);
        std::vector<vx_block_cell> out(count);
        if (const char* refused = vxb::check_points(points.data(), stride, count, out.data())) return refuse(refused);
        if (too_short(points, count, stride, argv[4])) return 1;
        for (uint32_t i = 0; i < count; ++i) {
            float p[3];
            std::memcpy(p, points.data() + size_t(i) * stride, 12);
            out[i] = with_format(svo_type, [&](auto format) { return vxb::cell_at_point<decltype(format)::value>(w, p); });
        }
        return write_file(argv[7], out.data(), out.size() * sizeof(vx_block_cell)) ? 0 : 1;
    }
    if (!std::strcmp(argv[3], "region") && argc == 11) {
        int32_t lo[3];
        uint32_t size[3];
        for (int a = 0; a < 3; ++a) lo[a] = i32_of(argv[4 + a]), size[a] = u32_of(argv[7 + a]);
        if (const char* refused = vxb::check_region(lo, size)) return refuse(refused);
        std::vector<uint32_t> out(size_t(size[0]) * size[1] * size[2], 0xdeadbeefu);  // (every voxel of the box has to be written)
        with_format(svo_type, [&](auto format) { vxb::read_region<decltype(format)::value>(w, lo, size, out.data()); });
        return write_file(argv[10], out.data(), out.size() * 4) ? 0 : 1;
    }
    return usage();
}

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
#include "on_host.hpp"
#include "vx_list.hpp"

using namespace on_host;
const char* const on_host::program = "list_on_host";

namespace {

int usage() {
    std::fprintf(stderr, "usage: list_on_host <svo_type> <world.bin> list <lox> <loy> <loz> <sx> <sy> <sz> <flags> <capacity> <out.bin>\n"
                         "       list_on_host rules\n");
    return 2;
}

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
    const int svo_type = svo_type_of(argv[1]);
    if (svo_type < 0) return usage();
    std::vector<uint8_t> world;
    if (!load(argv[2], world)) return 1;
    const HostWorld w = {world.data(), world.size()};
    int32_t lo[3];
    uint32_t size[3];
    for (int a = 0; a < 3; ++a) lo[a] = i32_of(argv[4 + a]), size[a] = u32_of(argv[7 + a]);
    const uint32_t flags = u32_of(argv[10]), capacity = u32_of(argv[11]);
    Output<vx_block_at> out(capacity != 0, capacity);  // (exactly `capacity` records; none: null in the call)
    uint32_t total = 0x5a5a5a5au;
    if (const char* refused = vxb::check_list(lo, size, flags, out.data(), capacity, &total)) return refuse(refused);
    const uint64_t bricks = size[0] && size[1] && size[2] ? vxb::region_bricks(vxb::plan_region(lo, size)) : 0;
    std::vector<uint32_t> counts(size_t(bricks) + 1);  // (exactly the workspace the call is given)
    total = bricks == 0 ? 0u : with_format(svo_type, [&](auto format) { return vxb::list_region<decltype(format)::value>(w, lo, size, flags, out.data(), capacity, counts.data()); });
    const uint32_t head[2] = {total, uint32_t(bricks)};
    std::ofstream f(argv[12], std::ios::binary);
    if (!f || !f.write(reinterpret_cast<const char*>(head), sizeof head)) return 1;
    if (capacity && !f.write(reinterpret_cast<const char*>(out.data()), std::streamsize(out.block.size() * sizeof(vx_block_at)))) return 1;
    return 0;
}

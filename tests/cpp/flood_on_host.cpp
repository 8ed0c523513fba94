// TEST HARNESS ONLY: vx_flood_points' answer (voxel-rs_amd/csrc/blocks/vx_flood.hpp) compiled for the host, as a stand-alone program -- the
// whole call on one thread, query by query: the bricks, rows and steps the kernel's workgroup walks, with loops where the kernel has threads
// -- over a world frame read from a file into a heap block of exactly its size (every read range-checked, as the device's buffer resource
// checks it; a sanitizer build of this program sees any that is not), the positions read through their stride from a heap block of exactly
// the input file's size, into heap blocks of exactly the bytes the call may write. tests/test_flood_on_host.py runs it, plain and built with
// -fsanitize=address,undefined; tests/test_flood.py holds the GPU's bytes against its output. Never linked into the product libraries; the
// product has no CPU path.
//
//   flood_on_host <svo_type> <world.bin> flood <points.bin> <pos_stride> <count> <size.x> <size.y> <size.z> <seed_at.x> <seed_at.y> <seed_at.z>
//                 <max_steps> <pass_value> <flags> <field_stride> <fields.bin | -> <info.bin | ->
//                                  -> fields.bin: count * field_stride bytes (field_stride 0: the voxel count rounded up to 16), what the call
//                                  leaves untouched 0x5a; info.bin: `count` vx_flood_info records; "-": that output is null
//   flood_on_host rules            prints what check_flood refuses
#include "on_host.hpp"
#include "vx_flood.hpp"

using namespace on_host;
const char* const on_host::program = "flood_on_host";

namespace {

int usage() {
    std::fprintf(stderr, "usage: flood_on_host <svo_type> <world.bin> flood <points.bin> <pos_stride> <count> <size x y z> <seed_at x y z> <max_steps> "
                         "<pass_value> <flags> <field_stride> <fields.bin | -> <info.bin | ->\n       flood_on_host rules\n");
    return 2;
}

int rules() {
    alignas(16) static float v[64];
    static uint8_t fields[2 * 32768];
    static vx_flood_info info[2];
    const unsigned char* bytes = reinterpret_cast<const unsigned char*>(v);
    const vx_flood_shape ok = {{17, 17, 17}, {8, 8, 8}, 250, 0, 0};
    say("packed", vxb::check_flood(v, 12, 2, &ok, fields, 0, info));
    say("entities", vxb::check_flood(v, 64, 1, &ok, fields, 0, info));
    say("fields only", vxb::check_flood(v, 12, 2, &ok, fields, 0, nullptr));
    say("info only", vxb::check_flood(v, 12, 2, &ok, nullptr, 0, info));
    say("info only, any stride", vxb::check_flood(v, 12, 1u << 24, &ok, nullptr, 7, info));
    say("count 0", vxb::check_flood(nullptr, 0, 0, nullptr, nullptr, 0, nullptr));
    say("too many", vxb::check_flood(v, 12, (1u << 24) + 1u, &ok, nullptr, 0, info));
    say("null shape", vxb::check_flood(v, 12, 1, nullptr, fields, 0, info));
    say("null pos", vxb::check_flood(nullptr, 12, 1, &ok, fields, 0, info));
    say("no output", vxb::check_flood(v, 12, 1, &ok, nullptr, 0, nullptr));
    for (uint32_t stride : {0u, 4u, 8u, 13u, 14u}) say("pos_stride " + std::to_string(stride), vxb::check_flood(v, stride, 1, &ok, fields, 0, info));
    for (int off : {1, 2, 3}) say("pos + " + std::to_string(off), vxb::check_flood(bytes + off, 12, 1, &ok, fields, 0, info));
    vx_flood_shape s = ok;
    for (int a = 0; a < 3; ++a)
        for (uint32_t side : {0u, 33u, 0xffffffffu}) {
            s = ok, s.size[a] = side, s.seed_at[a] = 0;
            say("size[" + std::to_string(a) + "] " + std::to_string(side), vxb::check_flood(v, 12, 1, &s, fields, 0, info));
        }
    for (int a = 0; a < 3; ++a) {
        s = ok, s.seed_at[a] = 17;
        say("seed_at[" + std::to_string(a) + "] 17", vxb::check_flood(v, 12, 1, &s, fields, 0, info));
    }
    s = ok, s.size[0] = s.size[1] = s.size[2] = 32, s.seed_at[0] = s.seed_at[1] = s.seed_at[2] = 31;
    say("largest box", vxb::check_flood(v, 12, 1, &s, fields, 0, info));
    s = ok, s.size[0] = s.size[1] = s.size[2] = 1, s.seed_at[0] = s.seed_at[1] = s.seed_at[2] = 0, s.max_steps = 0;
    say("smallest box", vxb::check_flood(v, 12, 1, &s, fields, 0, info));
    s = ok, s.max_steps = 251;
    say("max_steps 251", vxb::check_flood(v, 12, 1, &s, fields, 0, info));
    for (uint32_t flags : {1u, 2u, 3u, 0x80000000u}) {
        s = ok, s.flags = flags;
        say("flags " + std::to_string(flags), vxb::check_flood(v, 12, 1, &s, fields, 0, info));
    }
    s = ok, s.pass_value = 0xffffffffu;
    say("any pass_value", vxb::check_flood(v, 12, 1, &s, fields, 0, info));
    for (uint32_t stride : {4913u, 4920u, 4912u, 4928u, 16u, 8192u}) say("field_stride " + std::to_string(stride), vxb::check_flood(v, 12, 1, &ok, fields, stride, info));
    say("field bytes 2^24", vxb::check_flood(v, 12, 2048, &ok, fields, 8192, info));
    say("field bytes 2^24 + 8192", vxb::check_flood(v, 12, 2049, &ok, fields, 8192, info));
    say("field bytes by the default stride", vxb::check_flood(v, 12, 3405, &ok, fields, 0, info));  // (3,405 * 4,928 > 2^24 >= 3,404 * 4,928)
    say("field bytes by the default stride, one fewer", vxb::check_flood(v, 12, 3404, &ok, fields, 0, info));
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc == 2 && !std::strcmp(argv[1], "rules")) return rules();
    if (argc != 19 || std::strcmp(argv[3], "flood")) return usage();
    const int svo_type = svo_type_of(argv[1]);
    if (svo_type < 0) return usage();
    std::vector<uint8_t> world, raw;
    if (!load(argv[2], world) || !load(argv[4], raw)) return 1;
    const HostWorld w = {world.data(), world.size()};
    const auto u32 = [argv](int i) { return u32_of(argv[i]); };
    const uint32_t pos_stride = u32(5), count = u32(6), field_stride = u32(16);
    const vx_flood_shape s = {{u32(7), u32(8), u32(9)}, {u32(10), u32(11), u32(12)}, u32(13), u32(14), u32(15)};
    const bool want_fields = given(argv[17]), want_info = given(argv[18]);
    if (const char* refused = vxb::check_flood(raw.data(), pos_stride, count, &s, stand_in(want_fields), field_stride, stand_in(want_info))) return refuse(refused);
    const size_t packed = vxb::flood_round16(vxb::flood_voxels(s));
    Fields fields(want_fields, count, field_stride ? field_stride : packed, packed);
    Output<vx_flood_info> info(want_info, count);
    if (too_short(raw, count, pos_stride, "points.bin")) return 1;
    with_format(svo_type, [&](auto format) { vxb::flood_points<decltype(format)::value>(w, raw.data(), pos_stride, count, s, fields.data(), field_stride, info.data()); });
    return fields.write(argv[17]) && info.write(argv[18]) ? 0 : 1;
}

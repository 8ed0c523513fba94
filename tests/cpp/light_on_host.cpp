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
#include "on_host.hpp"
#include "vx_light.hpp"

using namespace on_host;
const char* const on_host::program = "light_on_host";

namespace {

int usage() {
    std::fprintf(stderr, "usage: light_on_host <svo_type> <world.bin> light <lo.bin> <lo_stride> <count> <size x y z> <flags> <props.bin | -> <field_stride> "
                         "<fields.bin | -> <info.bin | ->\n       light_on_host rules\n");
    return 2;
}

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
    const int svo_type = svo_type_of(argv[1]);
    if (svo_type < 0) return usage();
    std::vector<uint8_t> world, raw, table;
    const bool has_props = given(argv[11]);
    if (!load(argv[2], world) || !load(argv[4], raw) || (has_props && !load(argv[11], table))) return 1;
    const HostWorld w = {world.data(), world.size()};
    const auto u32 = [argv](int i) { return u32_of(argv[i]); };
    const uint32_t lo_stride = u32(5), count = u32(6), field_stride = u32(12);
    const vx_light_shape s = {{u32(7), u32(8), u32(9)}, u32(10), has_props ? table.data() : nullptr, uint32_t(table.size())};
    const bool want_fields = given(argv[13]), want_info = given(argv[14]);
    if (const char* refused = vxb::check_light(raw.data(), lo_stride, count, &s, stand_in(want_fields), field_stride, stand_in(want_info))) return refuse(refused);
    const size_t packed = vxb::light_round16(vxb::light_voxels(s.size));
    Fields fields(want_fields, count, field_stride ? field_stride : packed, packed);
    Output<vx_light_info> info(want_info, count);
    if (too_short(raw, count, lo_stride, "lo.bin")) return 1;
    with_format(svo_type, [&](auto format) { vxb::light_boxes<decltype(format)::value>(w, raw.data(), lo_stride, count, s, fields.data(), field_stride, info.data()); });
    return fields.write(argv[13]) && info.write(argv[14]) ? 0 : 1;
}

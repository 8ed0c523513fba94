// TEST HARNESS ONLY: vx_move_boxes' answer (voxel-rs_amd/csrc/blocks/vx_move.hpp) compiled for the host, as a stand-alone program -- the
// whole call on one thread, box by box, pass by pass and brick by brick as the kernel runs it, with loops where the kernel ballots and
// shuffles -- over a world frame read from a file into a heap block of exactly its size (every read range-checked, as the device's buffer
// resource checks it; a sanitizer build of this program sees any that is not), the boxes' vectors and the motions read through their strides
// from a heap block of exactly the input file's size, into a heap block of exactly `count` records. tests/test_move_on_host.py runs it,
// plain and built with -fsanitize=address,undefined -fsanitize=float-cast-overflow (the float-to-integer conversions of the slab);
// tests/test_move.py holds the GPU's records against its output. Never linked into the product libraries; the product has no CPU path.
//
//   move_on_host <svo_type> <world.bin> move <raw.bin> <count> <origin_at> <origin_stride> <offset_at> <offset_stride> <extents_at>
//                <extents_stride> <motion_at> <motion_stride> <only_value> <scale_bits> <skin_bits> <order> <out.bin>
//                                  the vectors lie in raw.bin from byte *_at on (offset_at -1: no offset, a null pointer); scale and skin
//                                  are given as the hexadecimal bits of their floats
//                                  -> out.bin: `count` vx_move_hit records
//   move_on_host rules             prints what check_move refuses
#include <cmath>
#include <limits>

#include "on_host.hpp"
#include "vx_move.hpp"

using namespace on_host;
const char* const on_host::program = "move_on_host";

namespace {

float float_of_bits(const char* hex) {
    const uint32_t bits = uint32_t(std::strtoul(hex, nullptr, 16));
    float v;
    std::memcpy(&v, &bits, 4);
    return v;
}

int usage() {
    std::fprintf(stderr, "usage: move_on_host <svo_type> <world.bin> move <raw.bin> <count> <origin_at> <origin_stride> <offset_at> <offset_stride> "
                         "<extents_at> <extents_stride> <motion_at> <motion_stride> <only_value> <scale_bits> <skin_bits> <order> <out.bin>\n"
                         "       move_on_host rules\n");
    return 2;
}

int rules() {
    alignas(16) static float v[64];
    static vx_move_hit out[2];
    const unsigned char* bytes = reinterpret_cast<const unsigned char*>(v);
    const vx_box_batch boxes = {v, v + 3, v + 6, 12, 12, 12, 0};
    const float* motion = v + 9;
    const vx_move_shape ok = {1.0f, 0.0009765625f, VX_MOVE_ORDER_YXZ, 0};
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    say("packed", vxb::check_move(&boxes, motion, 12, 2, &ok, out));
    say("one motion", vxb::check_move(&boxes, motion, 0, 2, &ok, out));
    say("entities", vxb::check_move(&boxes, motion, 64, 1u << 24, &ok, out));
    say("count 0", vxb::check_move(nullptr, nullptr, 0, 0, &ok, nullptr));
    say("count 0, null shape", vxb::check_move(nullptr, nullptr, 0, 0, nullptr, nullptr));
    say("null shape", vxb::check_move(&boxes, motion, 12, 1, nullptr, out));
    say("null motion", vxb::check_move(&boxes, nullptr, 12, 1, &ok, out));
    say("null boxes", vxb::check_move(nullptr, motion, 12, 1, &ok, out));
    say("null out", vxb::check_move(&boxes, motion, 12, 1, &ok, nullptr));
    say("too many", vxb::check_move(&boxes, motion, 12, (1u << 24) + 1u, &ok, out));
    vx_box_batch b = boxes;
    b.origin_stride = 8;
    say("origin_stride 8", vxb::check_move(&b, motion, 12, 1, &ok, out));
    for (uint32_t stride : {4u, 8u, 13u, 18u}) say("motion_stride " + std::to_string(stride), vxb::check_move(&boxes, motion, stride, 1, &ok, out));
    for (uint32_t stride : {12u, 16u, 64u}) say("motion_stride " + std::to_string(stride), vxb::check_move(&boxes, motion, stride, 1, &ok, out));
    for (int off : {1, 2, 3}) say("motion + " + std::to_string(off), vxb::check_move(&boxes, bytes + 36 + off, 12, 1, &ok, out));
    vx_move_shape s = ok;
    const struct { const char* name; float value; } scales[] = {{"scale 0", 0.0f}, {"scale -1", -1.0f}, {"scale 1e30", 1e30f}, {"scale inf", inf}, {"scale -inf", -inf}, {"scale nan", nan}};
    for (const auto& c : scales) {
        s = ok, s.scale = c.value;
        say(c.name, vxb::check_move(&boxes, motion, 12, 1, &s, out));
    }
    const struct { const char* name; float value; } skins[] = {{"skin 0", 0.0f}, {"skin -0", -0.0f}, {"skin 1", 1.0f}, {"skin 0.5", 0.5f}, {"skin -1e-6", -1e-6f},
                                                               {"skin 1.0000001", 1.0000001f}, {"skin inf", inf}, {"skin nan", nan}};
    for (const auto& c : skins) {
        s = ok, s.skin = c.value;
        say(c.name, vxb::check_move(&boxes, motion, 12, 1, &s, out));
    }
    // every value of the six bits, and a bit above them: the six permutations are allowed, nothing else
    for (uint32_t order = 0; order < 64; ++order) {
        s = ok, s.order = order;
        say("order " + std::to_string(order), vxb::check_move(&boxes, motion, 12, 1, &s, out));
    }
    for (uint32_t order : {0x21u | 0x40u, 0x21u | 0x80000000u}) {
        s = ok, s.order = order;
        say("order " + std::to_string(order), vxb::check_move(&boxes, motion, 12, 1, &s, out));
    }
    for (uint32_t flags : {1u, 0x80000000u}) {
        s = ok, s.flags = flags;
        say("flags " + std::to_string(flags), vxb::check_move(&boxes, motion, 12, 1, &s, out));
    }
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc == 2 && !std::strcmp(argv[1], "rules")) return rules();
    if (argc != 19 || std::strcmp(argv[3], "move")) return usage();
    const int svo_type = svo_type_of(argv[1]);
    if (svo_type < 0) return usage();
    std::vector<uint8_t> world, raw;
    if (!load(argv[2], world) || !load(argv[4], raw)) return 1;
    const HostWorld w = {world.data(), world.size()};
    const uint32_t count = u32_of(argv[5]), motion_stride = u32_of(argv[13]);
    const vx_box_batch b = box_batch_of(argv, raw, u32_of(argv[14]));
    const void* motion = raw.data() + std::atoll(argv[12]);
    vx_move_shape shape = {};
    shape.scale = float_of_bits(argv[15]);
    shape.skin = float_of_bits(argv[16]);
    shape.order = u32_of(argv[17]);
    Output<vx_move_hit> out(true, count);  // (exactly `count` records)
    if (const char* refused = vxb::check_move(&b, motion, motion_stride, count, &shape, out.data())) return refuse(refused);
    with_format(svo_type, [&](auto format) { vxb::move_boxes<decltype(format)::value>(w, b, motion, motion_stride, count, shape, out.data()); });
    return out.write(argv[18]) ? 0 : 1;
}

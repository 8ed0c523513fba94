// TEST HARNESS ONLY: vx_overlap_boxes' answer (voxel-rs_amd/csrc/blocks/vx_boxes.hpp) compiled for the host, as a stand-alone program -- the
// whole call on one thread, box by box and brick by brick as the kernel runs it, with a loop where the kernel shuffles -- over a world frame
// read from a file into a heap block of exactly its size (every read range-checked, as the device's buffer resource checks it; a sanitizer
// build of this program sees any that is not), the boxes' vectors read through their strides from a heap block of exactly the input file's
// size, into a heap block of exactly `count` records. tests/test_boxes_on_host.py runs it, plain and built with -fsanitize=address,undefined
// -fsanitize=float-cast-overflow (the float-to-integer conversions of the cover); tests/test_boxes.py holds the GPU's records against its
// output. Never linked into the product libraries; the product has no CPU path.
//
//   boxes_on_host <svo_type> <world.bin> boxes <raw.bin> <count> <origin_at> <origin_stride> <offset_at> <offset_stride> <extents_at>
//                 <extents_stride> <only_value> <out.bin>
//                                  the vectors lie in raw.bin from byte *_at on (offset_at -1: no offset, a null pointer)
//                                  -> out.bin: `count` vx_box_hit records
//   boxes_on_host rules            prints what check_boxes refuses
#include "on_host.hpp"
#include "vx_boxes.hpp"

using namespace on_host;
const char* const on_host::program = "boxes_on_host";

namespace {

int usage() {
    std::fprintf(stderr, "usage: boxes_on_host <svo_type> <world.bin> boxes <raw.bin> <count> <origin_at> <origin_stride> <offset_at> <offset_stride> "
                         "<extents_at> <extents_stride> <only_value> <out.bin>\n       boxes_on_host rules\n");
    return 2;
}

int rules() {
    alignas(16) static float v[64];
    static vx_box_hit out[2];
    const unsigned char* bytes = reinterpret_cast<const unsigned char*>(v);
    const vx_box_batch ok = {v, v + 3, v + 6, 12, 12, 12, 0};
    say("packed", vxb::check_boxes(&ok, 2, out));
    vx_box_batch b = ok;
    b.offset = nullptr, b.offset_stride = 7;  // (a stride nobody steps by)
    say("no offset", vxb::check_boxes(&b, 2, out));
    b = ok, b.offset_stride = b.extents_stride = 0;
    say("one offset, one extents", vxb::check_boxes(&b, 2, out));
    b = ok, b.origin_stride = b.offset_stride = b.extents_stride = 64, b.only_value = 0xffffffffu;
    say("entities", vxb::check_boxes(&b, 1u << 24, out));
    say("count 0", vxb::check_boxes(nullptr, 0, nullptr));
    say("too many", vxb::check_boxes(&ok, (1u << 24) + 1u, out));
    say("null boxes", vxb::check_boxes(nullptr, 1, out));
    say("null out", vxb::check_boxes(&ok, 1, nullptr));
    b = ok, b.origin = nullptr;
    say("null origin", vxb::check_boxes(&b, 1, out));
    b = ok, b.extents = nullptr;
    say("null extents", vxb::check_boxes(&b, 1, out));
    for (uint32_t stride : {0u, 4u, 8u, 13u, 14u}) {
        b = ok, b.origin_stride = stride;
        say(("origin_stride " + std::to_string(stride)).c_str(), vxb::check_boxes(&b, 1, out));
    }
    for (uint32_t stride : {4u, 8u, 13u, 18u}) {
        b = ok, b.offset_stride = stride;
        say(("offset_stride " + std::to_string(stride)).c_str(), vxb::check_boxes(&b, 1, out));
        b = ok, b.extents_stride = stride;
        say(("extents_stride " + std::to_string(stride)).c_str(), vxb::check_boxes(&b, 1, out));
    }
    for (int off : {1, 2, 3}) {
        b = ok, b.origin = bytes + off;
        say(("origin + " + std::to_string(off)).c_str(), vxb::check_boxes(&b, 1, out));
        b = ok, b.offset = bytes + 12 + off;
        say(("offset + " + std::to_string(off)).c_str(), vxb::check_boxes(&b, 1, out));
        b = ok, b.extents = bytes + 24 + off;
        say(("extents + " + std::to_string(off)).c_str(), vxb::check_boxes(&b, 1, out));
    }
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc == 2 && !std::strcmp(argv[1], "rules")) return rules();
    if (argc != 14 || std::strcmp(argv[3], "boxes")) return usage();
    const int svo_type = svo_type_of(argv[1]);
    if (svo_type < 0) return usage();
    std::vector<uint8_t> world, raw;
    if (!load(argv[2], world) || !load(argv[4], raw)) return 1;
    const HostWorld w = {world.data(), world.size()};
    const uint32_t count = u32_of(argv[5]);
    const vx_box_batch b = box_batch_of(argv, raw, u32_of(argv[12]));
    Output<vx_box_hit> out(true, count);  // (exactly `count` records)
    if (const char* refused = vxb::check_boxes(&b, count, out.data())) return refuse(refused);
    with_format(svo_type, [&](auto format) { vxb::overlap_boxes<decltype(format)::value>(w, b, count, out.data()); });
    return out.write(argv[13]) ? 0 : 1;
}

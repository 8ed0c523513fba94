// TEST HARNESS ONLY: vx_distance_boxes' answer (voxel-rs_amd/csrc/blocks/vx_distance.hpp) compiled for the host, as a stand-alone program --
// the whole call on one thread, box by box: the bricks, rows and the two passes the kernel's workgroup runs, with loops where the kernel has
// threads -- over a world frame read from a file into a heap block of exactly its size (every read range-checked, as the device's buffer
// resource checks it; a sanitizer build of this program sees any that is not), the boxes read through their stride from a heap block of
// exactly the input file's size, into heap blocks of exactly the bytes the call may write. tests/test_distance_on_host.py runs it, plain and
// built with -fsanitize=address,undefined; tests/test_distance.py holds the GPU's bytes against its output. Never linked into the product
// libraries; the product has no CPU path.
//
//   distance_on_host <svo_type> <world.bin> distance <lo.bin> <lo_stride> <count> <size.x> <size.y> <size.z> <pass_value> <match_value> <flags>
//                    <field_stride> <fields.bin | -> <info.bin | ->
//                                  -> fields.bin: count * field_stride bytes (field_stride 0: twice the voxel count rounded up to 16), what the
//                                  call leaves untouched 0x5a; info.bin: `count` vx_distance_info records; "-": that output is null
//   distance_on_host rules         prints what check_distance refuses
//   distance_on_host lines         the bit function and the min-plus pass against their definitions, on seeded words and lines
#include "on_host.hpp"
#include "vx_distance.hpp"

using namespace on_host;
const char* const on_host::program = "distance_on_host";

namespace {

int usage() {
    std::fprintf(stderr, "usage: distance_on_host <svo_type> <world.bin> distance <lo.bin> <lo_stride> <count> <size x y z> <pass_value> <match_value> <flags> "
                         "<field_stride> <fields.bin | -> <info.bin | ->\n       distance_on_host rules\n       distance_on_host lines\n");
    return 2;
}

int rules() {
    alignas(16) static int32_t v[64];
    alignas(16) static uint8_t fields[2 * 8192];
    static vx_distance_info info[2];
    const unsigned char* bytes = reinterpret_cast<const unsigned char*>(v);
    const vx_distance_shape ok = {{16, 16, 16}, 0, 0, 0, {0, 0}};  // 4,096 cells: 8,192 bytes a field
    const auto check = [&](const vx_distance_shape& s, uint32_t count = 1, uint32_t field_stride = 0) { return vxb::check_distance(v, 12, count, &s, fields, field_stride, info); };
    say("packed", vxb::check_distance(v, 12, 2, &ok, fields, 0, info));
    say("stride 64", vxb::check_distance(v, 64, 1, &ok, fields, 0, info));
    say("fields only", vxb::check_distance(v, 12, 2, &ok, fields, 0, nullptr));
    say("info only", vxb::check_distance(v, 12, 2, &ok, nullptr, 0, info));
    say("info only, any stride", vxb::check_distance(v, 12, 2, &ok, nullptr, 7, info));
    say("count 0", vxb::check_distance(nullptr, 0, 0, nullptr, nullptr, 0, nullptr));
    {   // (the largest count: its boxes have to exist for the overlap rule, so they come from the heap)
        std::vector<int32_t> many(size_t(3) << 20);
        std::vector<vx_distance_info> records(size_t(1) << 20);
        say("count 2^20", vxb::check_distance(many.data(), 12, 1u << 20, &ok, nullptr, 0, records.data()));
        say("too many", vxb::check_distance(many.data(), 12, (1u << 20) + 1u, &ok, nullptr, 0, records.data()));
    }
    say("null shape", vxb::check_distance(v, 12, 1, nullptr, fields, 0, info));
    say("null lo", vxb::check_distance(nullptr, 12, 1, &ok, fields, 0, info));
    say("no output", vxb::check_distance(v, 12, 1, &ok, nullptr, 0, nullptr));
    for (uint32_t stride : {0u, 4u, 8u, 13u, 14u}) say("lo_stride " + std::to_string(stride), vxb::check_distance(v, stride, 1, &ok, fields, 0, info));
    for (int off : {1, 2, 3}) say("lo + " + std::to_string(off), vxb::check_distance(bytes + off, 12, 1, &ok, fields, 0, info));
    vx_distance_shape s = ok;
    for (int a = 0; a < 3; ++a)
        for (uint32_t side : {0u, 33u, 0xffffffffu}) {
            s = ok, s.size[a] = side;
            say("size[" + std::to_string(a) + "] " + std::to_string(side), check(s));
        }
    s = ok, s.size[0] = s.size[1] = s.size[2] = 32;
    say("largest box", vxb::check_distance(v, 12, 1, &s, nullptr, 0, info));
    s = ok, s.size[0] = s.size[1] = s.size[2] = 1;
    say("smallest box", check(s));
    for (uint32_t flags : {1u, 2u, 3u, 0x80000000u}) {
        s = ok, s.flags = flags;
        say("flags " + std::to_string(flags), check(s));
    }
    s = ok, s.pass_value = 0xffffffffu;
    say("any pass_value", check(s));
    s = ok, s.match_value = 0xffffffffu;
    say("any match_value", check(s));
    s = ok, s.match_value = 3, s.flags = VX_DISTANCE_TO_AIR;
    say("match_value to air", check(s));
    s = ok, s.match_value = 3, s.pass_value = 9;
    say("match_value with pass_value", check(s));
    s = ok, s._pad[0] = s._pad[1] = 0xffffffffu;
    say("any padding", check(s));
    for (uint32_t stride : {8193u, 8200u, 8176u, 8192u, 8208u, 4096u, 16u, 16384u}) say("field_stride " + std::to_string(stride), vxb::check_distance(v, 12, 1, &ok, fields, stride, nullptr));
    {
        std::vector<int32_t> many(size_t(3) * 2100);
        std::vector<uint8_t> big((size_t(1) << 24) + 8192);
        say("field bytes 2^24", vxb::check_distance(many.data(), 12, 2048, &ok, big.data(), 0, nullptr));
        say("field bytes 2^24 + 8192", vxb::check_distance(many.data(), 12, 2049, &ok, big.data(), 0, nullptr));
        say("records only beyond 2^24", vxb::check_distance(many.data(), 12, 2049, &ok, nullptr, 0, big.data()));
    }
    // overlaps: an output on lo, the outputs on one another; side by side is allowed
    alignas(16) static uint8_t block[4096 + 64];
    s = ok, s.size[0] = s.size[1] = 4, s.size[2] = 2;  // a field of 64 bytes, 16 of info
    say("fields on lo", vxb::check_distance(block + 32, 12, 1, &s, block, 0, nullptr));
    say("fields beside lo", vxb::check_distance(block + 64, 12, 1, &s, block, 0, nullptr));
    say("info on lo", vxb::check_distance(block + 12, 12, 1, &s, nullptr, 0, block));
    say("info beside lo", vxb::check_distance(block + 16, 12, 1, &s, nullptr, 0, block));
    say("fields on info", vxb::check_distance(v, 12, 1, &s, block + 8, 0, block));
    say("side by side", vxb::check_distance(v, 12, 1, &s, block, 0, block + 64));
    say("strided fields between", vxb::check_distance(v, 12, 2, &s, block, 128, block + 64));  // (spans, first byte to last: the gap counts)
    return 0;
}

// distance_row_x and distance_pass against their definitions: a loop over the bits, a double loop over the line
int lines() {
    uint64_t state = 0x9e3779b97f4a7c15ull;
    const auto next = [&state]() {
        state ^= state << 13, state ^= state >> 7, state ^= state << 17;
        return uint32_t(state >> 16);
    };
    std::vector<uint32_t> words = {0u, 1u, 0x80000000u, 0xffffffffu, 0x80000001u, 0x00010000u};
    for (int k = 0; k < 2000; ++k) words.push_back(next() & next() & (k % 3 ? 0xffffffffu : next()));
    for (const uint32_t word : words)
        for (uint32_t rx = 0; rx < 32; ++rx) {
            uint32_t best = vxb::kDistanceNone;
            for (uint32_t tx = 0; tx < 32; ++tx)
                if (word >> tx & 1u) {
                    const uint32_t d = tx > rx ? tx - rx : rx - tx;
                    best = d * d < best ? d * d : best;
                }
            if (vxb::distance_row_x(word, rx) != best) {
                std::printf("distance_row_x(%08x, %u) = %u, expected %u\n", word, rx, vxb::distance_row_x(word, rx), best);
                return 1;
            }
        }
    for (int k = 0; k < 4000; ++k) {
        const uint32_t n = 1u + next() % 32u, kind = next() % 4u;
        uint32_t in[32], out[32];
        for (uint32_t j = 0; j < 32; ++j) {
            const uint32_t r = next();
            in[j] = j >= n ? vxb::kDistanceNone : kind == 0 ? vxb::kDistanceNone : (kind == 1 && r % 4u) ? vxb::kDistanceNone : r % 1923u;  // (at most 2 * 31^2)
            out[j] = 0xdeadbeefu;
        }
        vxb::distance_pass(in, out, n);
        for (uint32_t i = 0; i < 32; ++i) {
            uint32_t best = vxb::kDistanceNone;
            for (uint32_t j = 0; j < n; ++j) {
                const uint32_t d = i > j ? i - j : j - i, v = in[j] == vxb::kDistanceNone ? vxb::kDistanceNone : in[j] + d * d;
                best = v < best ? v : best;
            }
            if (out[i] != (i < n ? best : 0xdeadbeefu)) {
                std::printf("distance_pass: line %d of %u entries, out[%u] = %u, expected %u\n", k, n, i, out[i], i < n ? best : 0xdeadbeefu);
                return 1;
            }
        }
    }
    std::printf("ok\n");
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc == 2 && !std::strcmp(argv[1], "rules")) return rules();
    if (argc == 2 && !std::strcmp(argv[1], "lines")) return lines();
    if (argc != 16 || std::strcmp(argv[3], "distance")) return usage();
    const int svo_type = svo_type_of(argv[1]);
    if (svo_type < 0) return usage();
    std::vector<uint8_t> world, raw;
    if (!load(argv[2], world) || !load(argv[4], raw)) return 1;
    const HostWorld w = {world.data(), world.size()};
    const auto u32 = [argv](int i) { return u32_of(argv[i]); };
    const uint32_t lo_stride = u32(5), count = u32(6), field_stride = u32(13);
    const vx_distance_shape s = {{u32(7), u32(8), u32(9)}, u32(10), u32(11), u32(12), {0u, 0u}};
    // (the shape's own rules first, on one box and a record that lies apart: the sizes below come from a shape that has passed them; the
    // whole call's rules again below, on the blocks it writes to)
    alignas(16) static uint8_t apart[16];
    if (const char* refused = vxb::check_distance(raw.data(), 12, (count && raw.size() >= 12) ? 1u : 0u, &s, nullptr, 0, apart)) return refuse(refused);
    if (count > vxb::kDistanceMaxCount) return refuse("count exceeds 1048576 (2^20)");
    if (field_stride % 16u) return refuse("field_stride must be 0, or a multiple of 16");
    const size_t packed = vxb::distance_field_bytes(s);
    Fields fields(given(argv[14]), count, field_stride ? field_stride : packed, packed);
    Output<vx_distance_info> info(given(argv[15]), count);
    if (too_short(raw, count, lo_stride, "lo.bin")) return 1;
    if (const char* refused = vxb::check_distance(raw.data(), lo_stride, count, &s, fields.data(), field_stride, info.data())) return refuse(refused);
    with_format(svo_type, [&](auto format) { vxb::distance_boxes<decltype(format)::value>(w, raw.data(), lo_stride, count, s, fields.data(), field_stride, info.data()); });
    return fields.write(argv[14]) && info.write(argv[15]) ? 0 : 1;
}

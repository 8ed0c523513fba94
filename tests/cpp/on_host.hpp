// TEST HARNESS ONLY: what the stand-alone programs of the block entry points (tests/cpp/{blocks,scan,list,boxes,move,flood,light,walk,label,
// distance}_on_host.cpp) share -- the world's reader, the files, the arguments, the output blocks and the choice of the node format. Each
// program keeps its usage, its argument positions, its shape, its rules() listing and its one call into vxb::.
// What the sanitized builds of these programs rely on is kept here, once:
//   - the world, the inputs and every output lie in heap blocks of EXACTLY their size (read_file, Output): nothing is rounded up, nothing is
//     shared, so an access beyond one lands in the sanitizer's red zone;
//   - a read of the world that does not lie wholly inside it gives 0 (HostWorld), as the device's buffer resource answers it;
//   - an output the caller did not ask for is null in the call (Output::data); where a check wants a non-null stand-in for it, that is the
//     one-byte block `stand_in`, never the real buffer.
#pragma once

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>
#include <type_traits>
#include <vector>

#include "vx_blocks.hpp"

namespace on_host {

extern const char* const program;  // the program's name, as its messages give it: each program defines it

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

inline bool read_file(const char* path, std::vector<uint8_t>& out) {
    std::ifstream f(path, std::ios::binary | std::ios::ate);
    if (!f) return false;
    const std::streamsize n = f.tellg();
    f.seekg(0);
    out.resize(size_t(n));  // (exactly the file's size: the sanitizer's red zone starts at its end)
    return n == 0 || bool(f.read(reinterpret_cast<char*>(out.data()), n));
}

inline bool write_file(const char* path, const void* data, size_t bytes) {
    std::ofstream f(path, std::ios::binary);
    return f && (bytes == 0 || bool(f.write(static_cast<const char*>(data), std::streamsize(bytes))));
}

// a line of a rules() listing
inline void say(const char* what, const char* refused) { std::printf("%s: %s\n", what, refused ? refused : "ok"); }
inline void say(const std::string& what, const char* refused) { say(what.c_str(), refused); }

// "<program>: <what>" on stderr; 1, the exit code of a refusal
inline int refuse(const char* what) {
    std::fprintf(stderr, "%s: %s\n", program, what);
    return 1;
}

// an input file into a block of exactly its size, or a message
inline bool load(const char* path, std::vector<uint8_t>& out) {
    if (read_file(path, out)) return true;
    std::fprintf(stderr, "%s: cannot read %s\n", program, path);
    return false;
}
// `count` vectors of 12 bytes read through `stride` need more bytes than the file `name` gave: a message (and true)
inline bool too_short(const std::vector<uint8_t>& raw, uint32_t count, uint32_t stride, const char* name) {
    if (!count || raw.size() >= size_t(count - 1u) * stride + 12u) return false;
    std::fprintf(stderr, "%s: %s is too short\n", program, name);
    return true;
}

// the node format of a world, or -1
inline int svo_type_of(const char* arg) {
    const int svo_type = std::atoi(arg);
    return svo_type == VX_SVO_ESVO || svo_type == VX_SVO_CSVO ? svo_type : -1;
}
// call(format) with vxb::kEsvo or vxb::kCsvo as a constant: `decltype(format)::value` names the template argument
template <class F>
auto with_format(int svo_type, F&& call) {
    if (svo_type == VX_SVO_CSVO) return call(std::integral_constant<int, vxb::kCsvo>{});
    return call(std::integral_constant<int, vxb::kEsvo>{});
}

inline uint32_t u32_of(const char* arg) { return uint32_t(std::strtoul(arg, nullptr, 10)); }
inline int32_t i32_of(const char* arg) { return int32_t(std::strtol(arg, nullptr, 10)); }
// "-" in the place of a file: that input or output is null
inline bool given(const char* arg) { return std::strcmp(arg, "-") != 0; }

// The boxes of boxes_on_host and move_on_host, argv[6..11]: <origin_at> <origin_stride> <offset_at> <offset_stride> <extents_at> <extents_stride>,
// the vectors lying in `raw` from byte *_at on (offset_at -1: no offset, a null pointer).
inline vx_box_batch box_batch_of(char** argv, const std::vector<uint8_t>& raw, uint32_t only_value) {
    const long long origin_at = std::atoll(argv[6]), offset_at = std::atoll(argv[8]), extents_at = std::atoll(argv[10]);
    return {raw.data() + origin_at, offset_at < 0 ? nullptr : raw.data() + offset_at, raw.data() + extents_at, u32_of(argv[7]), u32_of(argv[9]), u32_of(argv[11]), only_value};
}

// (a one-byte block stands in for an output that has no byte to receive: never written, never null by accident)
inline uint8_t* stand_in(bool wanted) {
    static uint8_t none = 0;
    return wanted ? &none : nullptr;
}

// An output of the call: a heap block of exactly `n` records -- a record written beyond them is a heap overflow --, every byte 0x5a until
// the call writes it; not wanted: no block, and null in the call.
template <class T>
struct Output {
    bool wanted;
    std::vector<T> block;
    Output(bool wanted_, size_t n) : wanted(wanted_), block(wanted_ ? n : 0u) {
        if (!block.empty()) std::memset(static_cast<void*>(block.data()), 0x5a, block.size() * sizeof(T));
    }
    T* data() { return wanted ? block.data() : nullptr; }
    bool write(const char* path) const { return !wanted || write_file(path, block.data(), block.size() * sizeof(T)); }
};

// The fields of a call, `packed` bytes each as written, one every `stride` bytes: the block ends with the last byte the call may write -- the
// last query's field, not its whole stride --, and is written out at the whole stride, the tail of the last query as the sentinel.
struct Fields : Output<uint8_t> {
    size_t whole;
    Fields(bool wanted_, uint32_t count, size_t stride, size_t packed) : Output<uint8_t>(wanted_, count ? size_t(count - 1u) * stride + packed : 0u), whole(size_t(count) * stride) {}
    bool write(const char* path) {
        if (wanted) block.resize(whole, uint8_t(0x5a));
        return Output<uint8_t>::write(path);
    }
};

}  // namespace on_host

// The argument rules the block entry points share (check_points ... check_distance in the vx_*.hpp beside this file): each rule once, as a
// plain host function that gives what is wrong -- a string literal, which the caller may keep -- or null. A rule whose wording names the
// caller's own argument or limit takes the literal from its caller. The standard library only; nothing here is device code.
#pragma once

#include <cstdint>

namespace vxb {

constexpr uint32_t kMaxFieldBytes = 1u << 24;  // of all fields of a call

// three 4-byte components read through a stride: a multiple of 4 and at least 12; 0 (one vector for the whole batch) only where the call allows it
inline bool stride_ok(uint32_t stride, bool may_be_0 = false) { return stride % 4 == 0 && (stride >= 12 || (may_be_0 && stride == 0)); }
inline bool aligned_to_4(const void* p) { return reinterpret_cast<uintptr_t>(p) % 4 == 0; }

// Do the bytes [a, a + an) and [b, b + bn) share one? (an absent part has no bytes)
inline bool spans_meet(const void* a, uint64_t an, const void* b, uint64_t bn) {
    const uint64_t pa = reinterpret_cast<uintptr_t>(a), pb = reinterpret_cast<uintptr_t>(b);
    return a && b && an && bn && pa < pb + bn && pb < pa + an;
}

// A batch of box corners, an int32[3] each at lo + i * lo_stride. no_output: the caller's refusal of a call with no output at all, or null
// where it has one: that rule stands between these.
inline const char* lo_rule(const void* lo, uint32_t lo_stride, const char* no_output) {
    if (!lo) return "null lo";
    if (no_output) return no_output;
    if (!stride_ok(lo_stride)) return "lo_stride must be a multiple of 4 and >= 12";
    if (!aligned_to_4(lo)) return "lo must be aligned to 4 bytes";
    return nullptr;
}
// the bytes of such a batch, first to last
inline uint64_t lo_span(uint32_t count, uint32_t lo_stride) { return uint64_t(count - 1u) * lo_stride + 12u; }

// A box of 1..side cells an axis (`range`: the caller's wording of it), and, where the call has one, a seed cell inside it: axis by axis.
inline const char* size_rule(const uint32_t size[3], uint32_t side, const char* range, const uint32_t* seed_at = nullptr) {
    for (int a = 0; a < 3; ++a) {
        if (size[a] == 0 || size[a] > side) return range;
        if (seed_at && seed_at[a] >= size[a]) return "seed_at: every component must be below size's";
    }
    return nullptr;
}

// The fields of a call, `packed` bytes each as written, one every field_stride bytes (0: packed). least: the bytes of a field before their
// rounding up to 16, the least a stride may be (`at_least`: the caller's wording of it).
inline const char* field_stride_rule(uint32_t count, uint32_t field_stride, uint32_t least, uint32_t packed, const char* at_least) {
    if (field_stride % 16u || (field_stride && field_stride < least)) return at_least;
    if (uint64_t(count) * (field_stride ? field_stride : packed) > kMaxFieldBytes) return "count * field_stride exceeds 16777216 (2^24) bytes";
    return nullptr;
}
// the bytes of such fields, first to last written (count >= 1)
inline uint64_t field_span(uint32_t count, uint32_t field_stride, uint32_t packed) { return uint64_t(count - 1u) * (field_stride ? field_stride : packed) + packed; }

}  // namespace vxb

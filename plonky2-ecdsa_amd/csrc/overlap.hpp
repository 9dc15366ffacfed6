// BUFFER OVERLAP (include/p2e.h): the one rule every fixed-stride per-element entry point applies to its arguments before it
// reads its context.  Host only, no HIP (as knobs.hpp): tests/emu_overlap compiles it with g++ and the sanitizers.
//
// A call hands over its arguments as spans; overlap::check returns the first pair the contract refuses:
//   two outputs that share a byte;
//   an output that shares a byte with an input, unless the two are EXACTLY IN PLACE: same base, same bytes per element, same
//     element count, and the input is not a broadcast one (an input every lane reads, the single parent of a BIP-32 scan:
//     lane 0's store would reach it before the other lanes' loads);
//   a span whose end wraps round the address space (reported as a pair with itself).
// Two inputs may overlap as they like.  A null pointer or a zero count is no span.  Adjacent ranges share no byte.
// All interval arithmetic is in uintptr_t: pointers into different allocations are never compared as pointers.
#pragma once
#include <cstddef>
#include <cstdint>

namespace p2e {
namespace overlap {

struct Span {
    const char* name;           // the argument's name in include/p2e.h (for p2e_last_error)
    const void* ptr;            // null: the argument was not given, nothing to check
    size_t bytes_per_element;
    size_t count;               // elements at ptr (a broadcast input: the elements that exist, not the lanes that read them)
    bool is_output;
    bool broadcast;             // an input that every one of n > 1 lanes reads
};

struct Clash {
    bool bad = false;
    const char* a = nullptr;    // the earlier span of the list
    const char* b = nullptr;    // the later one (a == b: the span's own end wraps)
};

namespace detail {
// [lo, hi) of a span; false where count * bytes_per_element or lo + that does not fit the address space
inline bool range(const Span& s, uintptr_t& lo, uintptr_t& hi) {
    lo = reinterpret_cast<uintptr_t>(s.ptr);
    const uintptr_t bpe = static_cast<uintptr_t>(s.bytes_per_element), cnt = static_cast<uintptr_t>(s.count);
    if (bpe != 0 && cnt > UINTPTR_MAX / bpe) return false;
    const uintptr_t len = bpe * cnt;
    if (len > UINTPTR_MAX - lo) return false;
    hi = lo + len;
    return true;
}
inline bool live(const Span& s) { return s.ptr != nullptr && s.count != 0 && s.bytes_per_element != 0; }
}   // namespace detail

inline Clash check(const Span* spans, size_t num) {
    Clash k;
    for (size_t i = 0; i < num; ++i) {
        const Span& a = spans[i];
        if (!detail::live(a)) continue;
        uintptr_t alo, ahi;
        if (!detail::range(a, alo, ahi)) {
            k.bad = true, k.a = k.b = a.name;
            return k;
        }
        for (size_t j = i + 1; j < num; ++j) {
            const Span& b = spans[j];
            if (!detail::live(b) || !(a.is_output || b.is_output)) continue;
            uintptr_t blo, bhi;
            if (!detail::range(b, blo, bhi)) continue;   // reported when the outer loop reaches b
            if (ahi <= blo || bhi <= alo) continue;      // disjoint or adjacent
            const bool in_place = a.is_output != b.is_output && alo == blo && a.bytes_per_element == b.bytes_per_element &&
                                  a.count == b.count && !a.broadcast && !b.broadcast;
            if (in_place) continue;
            k.bad = true, k.a = a.name, k.b = b.name;
            return k;
        }
    }
    return k;
}

}   // namespace overlap
}   // namespace p2e

// THE BUFFERS OF A PER-ELEMENT CALL, written once.  Every fixed-stride per-element entry point lists its pointer arguments
// as Bufs (name, where the pointer lives, bytes per element, element count, role, required or not) and hands that one list
// to three consumers:
//   missing(list)        a required pointer is null; the "null pointer (...)" text names every argument of the list
//   spans(list)          the overlap::Spans of BUFFER OVERLAP (include/p2e.h), for overlap::check
//   stage(list, stager)  the host-pointer path: every given pointer is replaced by the stager's device copy of it
// The extent overlap reasons about and the extent staging copies are both bytes_per_element * count of the SAME Buf.
// Host only, no HIP (as overlap.hpp): tests/emu_overlap compiles it with g++ and the sanitizers.  A list is a
// std::initializer_list on the caller's stack; nothing here allocates unless an error text is made.
#pragma once
#include <cstddef>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <string>

#include "overlap.hpp"

namespace p2e {
namespace call_args {

enum class Role {
    In,       // lane i reads element i
    Out,      // lane i writes element i (a sum's single result: count 1)
    Shared,   // an input read by lanes that own no element of it: never in place
    Bcast,    // an input of `count` elements for n lanes: a broadcast one where count == 1 < n
    Opaque,   // null test only: its extent is no fixed stride (variable-length data, a handle, a host-side result slot)
};

struct Buf {
    const char* name;            // the argument's name in include/p2e.h
    void** slot;                 // the argument variable itself (of any object pointer type: read and written as bytes)
    size_t bytes_per_element;
    size_t count;
    Role role;
    bool required;
};
using List = std::initializer_list<Buf>;
constexpr size_t kMaxBufs = 16;  // the longest list of the library has 15 (p2e_sp_scan_batch)

// the macros take the variable itself: its name is the header's, its address the slot
#define P2E_ARG(p, bytes, count, role, required) \
    ::p2e::call_args::Buf{#p, (void**)&(p), (size_t)(bytes), (size_t)(count), ::p2e::call_args::Role::role, (required)}
#define ARG_IN(p, bytes, count) P2E_ARG(p, bytes, count, In, true)
#define ARG_OUT(p, bytes, count) P2E_ARG(p, bytes, count, Out, true)
#define ARG_SHARED(p, bytes, count) P2E_ARG(p, bytes, count, Shared, true)
#define ARG_BCAST(p, bytes, count) P2E_ARG(p, bytes, count, Bcast, true)
#define ARG_OPAQUE(p) P2E_ARG(p, 0, 0, Opaque, true)
#define ARG_IN_IF(required, p, bytes, count) P2E_ARG(p, bytes, count, In, required)   // required in some forms of the call only
#define ARG_OUT_IF(required, p, bytes, count) P2E_ARG(p, bytes, count, Out, required)
#define ARG_IN_OPT(p, bytes, count) P2E_ARG(p, bytes, count, In, false)
#define ARG_OUT_OPT(p, bytes, count) P2E_ARG(p, bytes, count, Out, false)

inline void* get(const Buf& b) {
    void* p;
    std::memcpy(&p, b.slot, sizeof p);
    return p;
}
inline void set(const Buf& b, const void* p) { std::memcpy(b.slot, &p, sizeof p); }

namespace detail {
// "a", "a and b", "a, b and c" of the list's required (or optional) arguments; the number of names
inline size_t names(List list, bool required, std::string& out) {
    size_t total = 0, at = 0;
    for (const Buf& b : list) total += b.required == required;
    for (const Buf& b : list) {
        if (b.required != required) continue;
        if (at) out += at + 1 == total ? " and " : ", ";
        out += b.name;
        ++at;
    }
    return total;
}
}   // namespace detail

// true: a required pointer is null, and `text` says which arguments the call needs (`form`: the form of the call whose
// list this is, where the list depends on one)
inline bool missing(List list, std::string& text, const char* form = nullptr) {
    bool any = false;
    for (const Buf& b : list) any = any || (b.required && !get(b));
    if (!any) return false;
    text = "null pointer (";
    const size_t req = detail::names(list, true, text);
    text += req == 1 ? " is required" : " are all required";
    if (form) text += std::string(" with ") + form;
    std::string opt;
    if (detail::names(list, false, opt)) text += "; " + opt + " may be null";
    text += ")";
    return true;
}

// the spans of the list for n lanes, into out[kMaxBufs]; a null pointer or a zero count is no span.  -> their number
inline size_t spans(List list, size_t lanes, overlap::Span* out) {
    if (list.size() > kMaxBufs) std::abort();
    size_t num = 0;
    for (const Buf& b : list) {
        const void* p = get(b);
        if (b.role == Role::Opaque || !p || b.count == 0) continue;
        const bool broadcast = b.role == Role::Shared || (b.role == Role::Bcast && b.count == 1 && lanes > 1);
        out[num++] = overlap::Span{b.name, p, b.bytes_per_element, b.count, b.role == Role::Out, broadcast};
    }
    return num;
}

// every given pointer becomes stager.in(ptr, bytes) / stager.out(ptr, bytes), in list order
template <class Stager>
inline void stage(List list, Stager& stager) {
    for (const Buf& b : list) {
        if (b.role == Role::Opaque) continue;
        const size_t bytes = b.bytes_per_element * b.count;
        if (unsigned char* p = static_cast<unsigned char*>(get(b)))
            set(b, b.role == Role::Out ? stager.out(p, bytes) : stager.in(static_cast<const unsigned char*>(p), bytes));
    }
}

}   // namespace call_args
}   // namespace p2e

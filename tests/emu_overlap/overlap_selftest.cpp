// Stand-alone run of the buffer-overlap rule (csrc/overlap.hpp; include/p2e.h BUFFER OVERLAP) under the address and
// undefined-behaviour sanitizers.  argv[1] is a text file tests/test_overlap_cpu.py writes: one span list per line with the
// classification Python integers give it.  No span is ever dereferenced: the addresses are numbers, the top of the address
// space included.  Every list lives in a heap allocation of exactly its size, so a walk past its end would stop the program.
//   line:  num  { ptr bytes_per_element count is_output broadcast } x num   bad a b
//   all numbers decimal u64; a, b: the positions of the refused pair (a == b: that span's end wraps), -1 -1 where none is
// Exit status 0 = every list was classified as the file says (and the file held at least one list).
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../plonky2-ecdsa_amd/csrc/call_args.hpp"
#include "../../plonky2-ecdsa_amd/csrc/overlap.hpp"

// Second mode, `overlap_selftest --lists FILE`: csrc/call_args.hpp alone.  Every line of FILE describes one call's buffer list;
// the program prints what the list's three consumers make of it, and tests/test_overlap_cpu.py compares that with Python integers.
//   line:  form lanes num { name ptr bytes_per_element count role required } x num
//          form: the word missing() is given for the form of the call, - for none; role: 0 In, 1 Out, 2 Shared, 3 Bcast, 4 Opaque
//   out:   list K / missing TEXT (or "missing -") / span NAME PTR BPE COUNT IS_OUTPUT BROADCAST ... /
//          stage NAME in|out BYTES ... (what the recording stager received, the name looked up by the pointer it was given) /
//          slot NAME VALUE ... (every argument variable afterwards: the stager's k-th answer is 0xD0000000 + 256 k)
// A list is at most 5 buffers long, built as an initializer_list like the library's.
struct Recorder {
    struct Seen {
        const void* ptr;
        bool out;
        size_t bytes;
    };
    std::vector<Seen> seen;
    unsigned char* answer() { return reinterpret_cast<unsigned char*>(static_cast<uintptr_t>(0xD0000000u + 256 * seen.size())); }
    const unsigned char* in(const unsigned char* p, size_t bytes) {
        seen.push_back({p, false, bytes});
        return answer();
    }
    unsigned char* out(unsigned char* p, size_t bytes) {
        seen.push_back({p, true, bytes});
        return answer();
    }
};
static int lists_mode(const char* path) {
    namespace ca = p2e::call_args;
    FILE* f = fopen(path, "r");
    if (!f) {
        fprintf(stderr, "cannot open %s\n", path);
        return 2;
    }
    size_t lists = 0;
    for (;;) {
        uint64_t lanes = 0, num = 0;
        char form[32];
        if (fscanf(f, "%31s %" SCNu64 " %" SCNu64, form, &lanes, &num) != 3) break;
        if (num > 5) return 2;
        char names[5][32];
        void* vars[5] = {};
        const void* given[5] = {};
        ca::Buf b[5] = {};
        for (uint64_t i = 0; i < num; i++) {
            uint64_t ptr, bpe, count, role, required;
            if (fscanf(f, "%31s %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64, names[i], &ptr, &bpe, &count, &role, &required) != 6 ||
                role > 4) {
                fprintf(stderr, "FAIL: list %zu of the file is malformed\n", lists);
                return 2;
            }
            given[i] = vars[i] = reinterpret_cast<void*>(static_cast<uintptr_t>(ptr));
            b[i] = ca::Buf{names[i], &vars[i], (size_t)bpe, (size_t)count, static_cast<ca::Role>(role), required != 0};
        }
        auto consume = [&](ca::List list) {
            printf("list %zu\n", lists++);
            std::string text;
            printf("missing %s\n", ca::missing(list, text, form[0] == '-' ? nullptr : form) ? text.c_str() : "-");
            p2e::overlap::Span spans[ca::kMaxBufs];
            const size_t ns = ca::spans(list, (size_t)lanes, spans);
            for (size_t i = 0; i < ns; i++)
                printf("span %s %" PRIu64 " %zu %zu %d %d\n", spans[i].name, (uint64_t) reinterpret_cast<uintptr_t>(spans[i].ptr),
                       spans[i].bytes_per_element, spans[i].count, spans[i].is_output ? 1 : 0, spans[i].broadcast ? 1 : 0);
            Recorder rec;
            ca::stage(list, rec);
            for (const Recorder::Seen& s : rec.seen) {
                const char* name = "?";
                for (uint64_t i = 0; i < num; i++)
                    if (given[i] == s.ptr) name = names[i];
                printf("stage %s %s %zu\n", name, s.out ? "out" : "in", s.bytes);
            }
            for (uint64_t i = 0; i < num; i++) printf("slot %s %" PRIu64 "\n", names[i], (uint64_t) reinterpret_cast<uintptr_t>(vars[i]));
        };
        switch (num) {
            case 0: consume({}); break;
            case 1: consume({b[0]}); break;
            case 2: consume({b[0], b[1]}); break;
            case 3: consume({b[0], b[1], b[2]}); break;
            case 4: consume({b[0], b[1], b[2], b[3]}); break;
            default: consume({b[0], b[1], b[2], b[3], b[4]}); break;
        }
    }
    fclose(f);
    return lists > 0 ? 0 : 1;
}

int main(int argc, char** argv) {
    static_assert(sizeof(uintptr_t) == 8, "the cases are written for a 64-bit address space");
    if (argc == 3 && std::string(argv[1]) == "--lists") return lists_mode(argv[2]);
    if (argc != 2) {
        fprintf(stderr, "usage: overlap_selftest CASES | overlap_selftest --lists LISTS\n");
        return 2;
    }
    FILE* f = fopen(argv[1], "r");
    if (!f) {
        fprintf(stderr, "cannot open %s\n", argv[1]);
        return 2;
    }
    using p2e::overlap::Span;
    size_t lists = 0, failures = 0;
    for (;;) {
        uint64_t num = 0;
        if (fscanf(f, "%" SCNu64, &num) != 1) break;
        std::vector<std::string> names(num);
        std::vector<Span> spans(num);
        bool read_ok = true;
        for (uint64_t i = 0; i < num; i++) {
            uint64_t ptr, bpe, count, out, bc;
            if (fscanf(f, "%" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64, &ptr, &bpe, &count, &out, &bc) != 5) {
                read_ok = false;
                break;
            }
            names[i] = std::to_string(i);
            spans[i] = Span{nullptr, reinterpret_cast<const void*>(static_cast<uintptr_t>(ptr)), (size_t)bpe, (size_t)count, out != 0, bc != 0};
        }
        for (uint64_t i = 0; i < num; i++) spans[i].name = names[i].c_str();
        int64_t bad = 0, a = 0, b = 0;
        if (!read_ok || fscanf(f, "%" SCNd64 " %" SCNd64 " %" SCNd64, &bad, &a, &b) != 3) {
            fprintf(stderr, "FAIL: list %zu of the file is malformed\n", lists);
            fclose(f);
            return 2;
        }
        const p2e::overlap::Clash k = p2e::overlap::check(spans.data(), spans.size());
        const int64_t ga = k.bad ? atoll(k.a) : -1, gb = k.bad ? atoll(k.b) : -1;
        if ((k.bad ? 1 : 0) != bad || ga != a || gb != b) {
            if (failures++ < 20)
                fprintf(stderr, "FAIL list %zu: got (%d, %" PRId64 ", %" PRId64 "), want (%" PRId64 ", %" PRId64 ", %" PRId64 ")\n", lists,
                        k.bad ? 1 : 0, ga, gb, bad, a, b);
        }
        lists++;
    }
    fclose(f);
    printf("overlap_selftest: %zu lists, %zu failures\n", lists, failures);
    return (lists > 0 && failures == 0) ? 0 : 1;
}

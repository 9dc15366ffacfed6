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

#include "../../plonky2-ecdsa_amd/csrc/overlap.hpp"

int main(int argc, char** argv) {
    static_assert(sizeof(uintptr_t) == 8, "the cases are written for a 64-bit address space");
    if (argc != 2) {
        fprintf(stderr, "usage: overlap_selftest CASES\n");
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

// Stand-alone run of the multi-scalar-multiplication kernel bodies under the address and undefined-behaviour sanitizers
// (and the limb-bound tracker), both curves.  Part 1: the cases of tests/msm_native_inputs.py selftest_cases, compiled in
// through msm_vectors.inc (small batches of every kind: sizes 0, 1, 2, 65, single points with k = 1 .. 17, cancelling
// pairs, neutral points only, equal scalars, every kind of rejected point, the scalar edges), each at its window widths,
// against its compiled-in expectation byte for byte, with the counted per-lane operations inside the plan's bound.
// Part 2: 150 random scalars on random multiples of G per curve and width against the double-and-add multiplication
// (sum k_i d_i) G of host::scalar_mul_cv.  Exit status 0 = all held.
#include <cstdio>
#include <cstring>

#include "p2e_emu_msm.cpp"

namespace {
struct Row {
    int kind;   // 0: case header, 1: point
    int curve, wb;
    size_t n;
    const char *a, *b, *c;   // header: outx, outy, -; point: k, px, py
    int status, bad;
};
#define MSM_CASE(curve, wb, n, outx, outy, status, bad) {0, curve, wb, n, outx, outy, nullptr, status, bad},
#define MSM_POINT(k, px, py) {1, 0, 0, 0, k, px, py, 0, 0},
const Row ROWS[] = {
#include "msm_vectors.inc"
};
void put_hex(uint8_t* dst, const char* hex) {   // 64 big-endian hex digits -> 32 little-endian bytes
    for (int i = 0; i < 32; i++) {
        unsigned b = 0;
        sscanf(hex + 2 * (31 - i), "%2x", &b);
        dst[i] = (uint8_t)b;
    }
}
// one call checked against (wx, wy, status, bad); point_err only for its sum
int check_call(int curve, unsigned wb, const std::vector<uint8_t>& k, const std::vector<uint8_t>& px, const std::vector<uint8_t>& py, size_t n,
               const uint8_t* wx, const uint8_t* wy, int status, long bad, const char* what) {
    uint8_t ox[32], oy[32], st = 0xAA;
    memset(ox, 0xAA, 32), memset(oy, 0xAA, 32);
    std::vector<uint8_t> perr(n + 1, 0xAA);
    uint64_t ops[7], plan[6];
    const long got = emum_point_msm(curve, wb, k.data(), px.data(), py.data(), n, ox, oy, &st, perr.data(), ops);
    int fails = emum_plan(curve, n, wb, plan) != 0;
    long flagged = 0;
    for (size_t i = 0; i < n; i++) flagged += perr[i] == 1, fails += perr[i] > 1;
    fails += perr[n] != 0xAA;
    if (got != bad || flagged != bad || st != status || memcmp(ox, wx, 32) || memcmp(oy, wy, 32)) fails++;
    for (int j = 0; j < 7; j++) fails += ops[j] > plan[5];
    if (fails) fprintf(stderr, "%s: curve %d width %u n %zu: status %d (expected %d), count %ld (expected %ld)\n", what, curve, wb, n, st, status, got, bad);
    return fails;
}
int run_vectors() {
    int fails = 0, cases = 0;
    const size_t rows = sizeof ROWS / sizeof ROWS[0];
    for (size_t at = 0; at < rows;) {
        const Row& h = ROWS[at++];
        if (h.kind != 0 || at + h.n > rows) return 1000;
        std::vector<uint8_t> k(32 * h.n + 32), px(32 * h.n + 32), py(32 * h.n + 32);
        for (size_t i = 0; i < h.n; i++, at++) {
            if (ROWS[at].kind != 1) return 1000;
            put_hex(&k[32 * i], ROWS[at].a), put_hex(&px[32 * i], ROWS[at].b), put_hex(&py[32 * i], ROWS[at].c);
        }
        uint8_t wx[32], wy[32];
        put_hex(wx, h.a), put_hex(wy, h.b);
        const unsigned all[4] = {0, MSM_WINDOW_MIN, 8, MSM_WINDOW_MAX};
        for (int j = 0; j < (h.wb < 0 ? 4 : 1); j++, cases++)
            fails += check_call(h.curve, h.wb < 0 ? all[j] : (unsigned)h.wb, k, px, py, h.n, wx, wy, h.status, h.bad, "vector");
    }
    printf("vectors: %d calls, %d failures\n", cases, fails);
    return fails + (cases < 100);
}
template <class CV>
int run_random(const char* name) {
    typedef typename CV::Fn Fn;
    const size_t n = 150;
    const int curve = CV::kAZero ? 0 : 1;
    const Aff G = host::generator_cv<CV>();
    std::vector<uint8_t> k(32 * n), px(32 * n), py(32 * n);
    host::SplitMix64 rng{0x3A5Du};
    U256 total = u256_zero();
    for (size_t i = 0; i < n; i++) {
        const U256 kk = host::u256_from_u64(rng.next(), rng.next(), rng.next(), rng.next());
        const U256 d = fe_canon<Fn>(host::u256_from_u64(rng.next(), rng.next(), rng.next(), rng.next() | 1));
        const Aff P = host::scalar_mul_cv<CV>(d, G);
        memcpy(&k[32 * i], kk.w, 32), memcpy(&px[32 * i], P.x.w, 32), memcpy(&py[32 * i], P.y.w, 32);
        total = fe_add<Fn>(total, fe_mul<Fn>(fe_canon<Fn>(kk), d));
    }
    const Aff want = host::scalar_mul_cv<CV>(total, G);
    int fails = 0;
    for (unsigned wb : {0u, 4u, 5u, 7u, 8u, 11u, 12u})
        fails += check_call(curve, wb, k, px, py, n, (const uint8_t*)want.x.w, (const uint8_t*)want.y.w, MSM_OK, 0, name);
    printf("%s: %zu random points x 7 widths, %d failures\n", name, n, fails);
    return fails;
}
}  // namespace

int main() {
    int fails = run_vectors();
    fails += run_random<Secp256k1>("secp256k1");
    fails += run_random<P256>("p256");
    return fails ? 1 : 0;
}

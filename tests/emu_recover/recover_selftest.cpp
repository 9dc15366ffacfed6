// Stand-alone run of the recovery body and the recoverable signer under the address and undefined-behaviour sanitizers
// (and the limb-bound tracker), both curves.  Part 1: every element of input set X (tests/recover_inputs.py, compiled in
// through recover_vectors.inc: forced digits of u2, edge values of u1, the doubling and the neutral-element case of the
// final addition, the overflow bit, non-residues, out-of-range r, s and v) against its compiled-in expectation, byte for
// byte, flagged kinds included.  Part 2: 128 random (msg, sk, k) per curve and plan signed recoverably, recovered, and
// compared with the double-and-add multiplication sk G (host::scalar_mul_cv); the same with v ^ 1 must give another
// point of the curve.  Exit status 0 = all held.
#include <cstdio>
#include <cstring>

#include "p2e_emu_recover.cpp"

namespace {
struct Vec {
    int curve;
    const char *msg, *r, *s;
    int v;
    const char *pkx, *pky;
    int err;
};
const Vec VECTORS[] = {
#include "recover_vectors.inc"
};
void put_hex(uint8_t* dst, const char* hex) {   // 64 big-endian hex digits -> 32 little-endian bytes
    for (int i = 0; i < 32; i++) {
        unsigned b = 0;
        sscanf(hex + 2 * (31 - i), "%2x", &b);
        dst[i] = (uint8_t)b;
    }
}
int run_vectors(int curve, const char* name) {
    std::vector<uint8_t> msg, r, s, v, wx, wy, werr;
    for (const Vec& t : VECTORS) {
        if (t.curve != curve) continue;
        const size_t o = v.size();
        for (auto* a : {&msg, &r, &s, &wx, &wy}) a->resize(32 * (o + 1));
        put_hex(&msg[32 * o], t.msg), put_hex(&r[32 * o], t.r), put_hex(&s[32 * o], t.s);
        put_hex(&wx[32 * o], t.pkx), put_hex(&wy[32 * o], t.pky);
        v.push_back((uint8_t)t.v);
        werr.push_back((uint8_t)t.err);
    }
    const size_t n = v.size();
    std::vector<uint8_t> px(32 * n, 0xAA), py(32 * n, 0xAA), err(n, 0xAA);
    const long bad = emur_recover(curve, msg.data(), r.data(), s.data(), v.data(), px.data(), py.data(), n, err.data());
    int fails = 0;
    long want_bad = 0;
    for (size_t i = 0; i < n; i++) {
        want_bad += werr[i] != 0;
        if (err[i] != werr[i] || memcmp(&px[32 * i], &wx[32 * i], 32) || memcmp(&py[32 * i], &wy[32 * i], 32))
            if (fails++ < 10) fprintf(stderr, "%s: vector %zu differs (err %d, expected %d)\n", name, i, err[i], werr[i]);
    }
    if (bad != want_bad) fails++, fprintf(stderr, "%s: count %ld, expected %ld\n", name, bad, want_bad);
    printf("%s: %zu vectors (%ld flagged), %d failures\n", name, n, want_bad, fails);
    return fails + (n < 100);
}
template <class CV>
int run_round_trip(const char* name) {
    const size_t n = 128;
    const int curve = CV::kAZero ? 0 : 1;
    std::vector<uint8_t> sk(32 * n), msg(32 * n), k(32 * n);
    host::SplitMix64 rng{0x7EC0u};
    for (size_t i = 0; i < n; i++)
        for (auto* a : {&sk, &msg, &k}) {
            const U256 x = host::u256_from_u64(rng.next(), rng.next(), rng.next(), rng.next());
            memcpy(a->data() + 32 * i, x.w, 32);
        }
    int fails = 0;
    const Aff G = host::generator_cv<CV>();
    for (int plan = 1; plan <= 2; plan++) {
        std::vector<uint8_t> r(32 * n, 0xAA), s(32 * n, 0xAA), v(n, 0xAA), e(n, 0xAA), px(32 * n, 0xAA), py(32 * n, 0xAA), e2(n, 0xAA);
        if (emur_sign_recoverable(curve, plan, msg.data(), sk.data(), k.data(), r.data(), s.data(), v.data(), n, e.data())) fails++;
        if (emur_recover(curve, msg.data(), r.data(), s.data(), v.data(), px.data(), py.data(), n, e2.data())) fails++;
        std::vector<uint8_t> v1(v), qx(32 * n, 0xAA), qy(32 * n, 0xAA), e3(n, 0xAA);
        for (auto& b : v1) b ^= 1;
        if (emur_recover(curve, msg.data(), r.data(), s.data(), v1.data(), qx.data(), qy.data(), n, e3.data())) fails++;
        for (size_t i = 0; i < n; i++) {
            const Aff w = host::scalar_mul_cv<CV>(sign_scalar<CV>(sk.data(), i), G);
            Aff got, other;
            got.x = load_packed(px.data(), i), got.y = load_packed(py.data(), i);
            other.x = load_packed(qx.data(), i), other.y = load_packed(qy.data(), i);
            if (v[i] > 3 || !u256_eq(w.x, got.x) || !u256_eq(w.y, got.y)) {
                if (fails++ < 10) fprintf(stderr, "%s plan %d: element %zu does not recover sk G\n", name, plan, i);
            }
            if (!host::aff_on_curve_cv<CV>(other) || u256_eq(other.x, got.x))
                if (fails++ < 10) fprintf(stderr, "%s plan %d: element %zu, v ^ 1\n", name, plan, i);
        }
    }
    printf("%s: %zu round trips x 2 plans, %d failures\n", name, n, fails);
    return fails;
}
}  // namespace

int main() {
    int fails = run_vectors(0, "secp256k1") + run_vectors(1, "p256");
    fails += run_round_trip<Secp256k1>("secp256k1");
    fails += run_round_trip<P256>("p256");
    return fails ? 1 : 0;
}

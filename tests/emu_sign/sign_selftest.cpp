// Stand-alone run of the key-derivation and signing bodies under the address and undefined-behaviour sanitizers (and
// the limb-bound tracker): both plans, both curves, 2 048 elements each -- random scalars, every power of sixteen, and
// the values around 0 and n.  Checks on every element: both plans give the same bytes, an unflagged public key is on the
// curve, the flagged elements are exactly those whose scalar is 0 modulo n; on every 32nd element pk and r against the
// double-and-add multiplication (host::scalar_mul_cv) and s against its defining equation.  Exit status 0 = all held.
#include <cstdio>
#include <cstring>

#include "p2e_emu_sign.cpp"

namespace {
template <class CV>
int run(const char* name) {
    typedef typename CV::Fn Fn;
    const size_t n = 2048;
    std::vector<uint8_t> sk(32 * n), msg(32 * n), k(32 * n);
    host::SplitMix64 rng{0x5157u};
    auto put = [](std::vector<uint8_t>& a, size_t i, const U256& v) { memcpy(a.data() + 32 * i, v.w, 32); };
    U256 nn;
    for (int j = 0; j < 8; j++) nn.w[j] = Fn::m(j);
    for (size_t i = 0; i < n; i++) {
        U256 v[3];
        for (auto& x : v) x = host::u256_from_u64(rng.next(), rng.next(), rng.next(), rng.next());
        if (i < 64) {   // 16^i
            v[0] = u256_zero();
            v[0].w[i >> 3] = 1u << (4 * (i & 7));
            v[2] = v[0];
        } else if (i < 72) {   // 0, 1, n - 1, n, n + 1, 2^256 - 1, 2, n - 2
            U256 e = u256_zero();
            const int c = (int)i - 64;
            if (c == 1) e = u256_small(1);
            if (c == 2 || c == 7) { e = nn; e.w[0] -= (c == 2 ? 1u : 2u); }
            if (c == 3) e = nn;
            if (c == 4) { e = nn; e.w[0] += 1u; }
            if (c == 5) for (auto& w : e.w) w = 0xFFFFFFFFu;
            if (c == 6) e = u256_small(2);
            v[0] = v[2] = e;
        } else if (i % 5 == 0) {   // sparse: most nibbles zero
            for (auto& w : v[0].w) w &= rng.next() & rng.next() & 0xFFFFFFFFu;
            for (auto& w : v[2].w) w &= rng.next() & rng.next() & 0xFFFFFFFFu;
        }
        put(sk, i, v[0]);
        put(msg, i, v[1]);
        put(k, i, v[2]);
    }
    std::vector<uint8_t> px[2], py[2], r[2], s[2], e1[2], e2[2];
    const int curve = CV::kAZero ? 0 : 1;
    for (int p = 0; p < 2; p++) {
        for (auto* a : {&px[p], &py[p], &r[p], &s[p]}) a->assign(32 * n, 0xAA);
        e1[p].assign(n, 0xAA);
        e2[p].assign(n, 0xAA);
        emus_public_key(curve, p + 1, sk.data(), px[p].data(), py[p].data(), n, e1[p].data());
        emus_sign(curve, p + 1, msg.data(), sk.data(), k.data(), r[p].data(), s[p].data(), n, e2[p].data());
    }
    int fails = 0;
    auto fail = [&](const char* what, size_t i) {
        if (fails++ < 10) fprintf(stderr, "%s: %s at element %zu\n", name, what, i);
    };
    if (px[0] != px[1] || py[0] != py[1] || r[0] != r[1] || s[0] != s[1] || e1[0] != e1[1] || e2[0] != e2[1]) fail("plans differ", 0);
    const Aff G = host::generator_cv<CV>();
    for (size_t i = 0; i < n; i++) {
        const U256 skv = sign_scalar<CV>(sk.data(), i), kv = sign_scalar<CV>(k.data(), i), mv = sign_scalar<CV>(msg.data(), i);
        if (e1[0][i] != (u256_is_zero(skv) ? ERR_POINT_AT_INFINITY : 0)) fail("public-key flag", i);
        if (e2[0][i] != (u256_is_zero(kv) ? ERR_INVERSE_OF_ZERO : 0)) fail("sign flag", i);
        Aff pk;
        pk.x = load_packed(px[0].data(), i);
        pk.y = load_packed(py[0].data(), i);
        const U256 rv = load_packed(r[0].data(), i), sv = load_packed(s[0].data(), i);
        if (e1[0][i]) {
            if (!u256_is_zero(pk.x) || !u256_is_zero(pk.y)) fail("flagged key not zero", i);
        } else if (!host::aff_on_curve_cv<CV>(pk)) {
            fail("public key off the curve", i);
        }
        if (e2[0][i]) {
            if (!u256_is_zero(rv) || !u256_is_zero(sv)) fail("flagged signature not zero", i);
            continue;
        }
        // s k = msg + r sk (mod n)
        if (!u256_eq(fe_mul<Fn>(sv, kv), fe_add<Fn>(mv, fe_mul<Fn>(rv, skv)))) fail("s k != msg + r sk", i);
        if (i % 32 == 0 || i < 72) {
            if (!e1[0][i]) {
                const Aff w = host::scalar_mul_cv<CV>(skv, G);
                if (!u256_eq(w.x, pk.x) || !u256_eq(w.y, pk.y)) fail("pk != sk G", i);
            }
            const Aff R = host::scalar_mul_cv<CV>(kv, G);
            if (!u256_eq(fe_canon<Fn>(R.x), rv)) fail("r != (k G).x mod n", i);
        }
    }
    printf("%s: %zu elements, %d failures\n", name, n, fails);
    return fails;
}
}  // namespace

int main() {
    int fails = run<Secp256k1>("secp256k1");
    fails += run<P256>("p256");
    return fails ? 1 : 0;
}

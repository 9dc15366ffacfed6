// Stand-alone run of the point-table bodies under the address and undefined-behaviour sanitizers (and the limb-bound
// tracker), both curves.  Part 1: the table of G equals host::fixed_base_table_cv byte for byte.  Part 2: a table of the
// compiled-in keys (tests/table_inputs.py, table_vectors.inc) in an allocation of EXACTLY its size, and three cases of
// every kind of set X per call against their compiled-in expectations -- lanes with idx >= m among them: a lane that read a
// table word for such an index would read past the allocation and stop the program.  Part 3: a rejected point builds
// nothing.  Part 4: 64 random (idx, k, a, b) per curve against host::scalar_mul_cv.
// Exit status 0 = all held.
#include <cstdio>
#include <cstring>

#include "p2e_emu_table.cpp"

namespace {
struct Pnt {
    int curve;
    const char *x, *y;
};
struct Vec {
    int curve, op;
    uint32_t idx;
    const char *a, *b, *s, *outx;
    int outy_odd, err, valid;
};
#define V(...)
#define T(curve, x, y) {curve, x, y},
const Pnt POINTS[] = {
#include "table_vectors.inc"
};
#undef T
#undef V
#define T(...)
#define V(curve, op, idx, a, b, s, outx, outy_odd, err, valid) {curve, op, idx, a, b, s, outx, outy_odd, err, valid},
const Vec VECTORS[] = {
#include "table_vectors.inc"
};
#undef T
#undef V
void put_hex(uint8_t* dst, const char* hex) {   // up to 64 big-endian hex digits -> 32 little-endian bytes
    const int len = (int)strlen(hex);
    memset(dst, 0, 32);
    for (int i = 0; i < len; i++) {
        const char c = hex[len - 1 - i];
        const unsigned d = c <= '9' ? (unsigned)(c - '0') : (unsigned)(c - 'a' + 10);
        dst[i / 2] |= (uint8_t)(d << (4 * (i & 1)));
    }
}
// the compiled-in keys of one curve and their table, in an allocation of exactly emut_table_bytes(m)
struct Keys {
    std::vector<uint8_t> px, py, tab;
    size_t m = 0;
};
Keys build_keys(int curve, int& fails) {
    Keys k;
    for (const Pnt& p : POINTS) {
        if (p.curve != curve) continue;
        k.px.resize(32 * (k.m + 1)), k.py.resize(32 * (k.m + 1));
        put_hex(&k.px[32 * k.m], p.x), put_hex(&k.py[32 * k.m], p.y);
        k.m++;
    }
    k.tab.assign(emut_table_bytes(k.m), 0xAA);
    std::vector<uint8_t> perr(k.m, 0xAA);
    if (emut_build(curve, k.px.data(), k.py.data(), k.m, k.tab.data(), perr.data()) != 0) fails++;
    for (uint8_t e : perr) fails += e != 0;
    return k;
}
int run_generator(int curve, const char* name, const Keys& k) {
    std::vector<uint8_t> want(emut_table_bytes(1));
    emut_generator_table(curve, want.data());
    const int fails = memcmp(want.data(), k.tab.data(), want.size()) != 0;   // key 0 is G
    printf("%s: table of G against fixed_base_table_cv, %d failures\n", name, fails);
    return fails;
}
int run_vectors(int curve, int op, const char* name, const Keys& k) {
    std::vector<uint8_t> a, b, s, wx, wodd, werr, wvalid;
    std::vector<uint32_t> idx;
    for (const Vec& t : VECTORS) {
        if (t.curve != curve || t.op != op) continue;
        const size_t o = werr.size();
        for (auto* v : {&a, &b, &s, &wx}) v->resize(32 * (o + 1));
        put_hex(&a[32 * o], t.a), put_hex(&b[32 * o], t.b), put_hex(&s[32 * o], t.s), put_hex(&wx[32 * o], t.outx);
        idx.push_back(t.idx);
        wodd.push_back((uint8_t)t.outy_odd), werr.push_back((uint8_t)t.err), wvalid.push_back((uint8_t)t.valid);
    }
    const size_t n = werr.size();
    std::vector<uint8_t> ox(32 * n, 0xAA), oy(32 * n, 0xAA), err(n, 0xAA);
    const long bad = emut_call(curve, op, k.tab.data(), idx.data(), (uint32_t)k.m, a.data(), b.data(), s.data(), ox.data(), oy.data(), n, err.data());
    int fails = 0, out_of_range = 0;
    long want_bad = 0;
    for (size_t i = 0; i < n; i++) {
        want_bad += werr[i] != 0;
        out_of_range += idx[i] >= k.m;
        bool ok = err[i] == werr[i];
        if (op == 2) {
            ok = ok && ox[i] == wvalid[i];   // the verdict bytes are the first n of ox
        } else {
            Aff got;
            got.x = load_packed(ox.data(), i), got.y = load_packed(oy.data(), i);
            const bool on = curve ? host::aff_on_curve_cv<P256>(got) : host::aff_on_curve_cv<Secp256k1>(got);
            ok = ok && !memcmp(&ox[32 * i], &wx[32 * i], 32) && (werr[i] ? u256_is_zero(got.y) : (on && (got.y.w[0] & 1u) == wodd[i]));
        }
        if (!ok && fails++ < 10) fprintf(stderr, "%s op %d: vector %zu differs (err %d, expected %d)\n", name, op, i, err[i], werr[i]);
    }
    if (bad != want_bad) fails++, fprintf(stderr, "%s op %d: count %ld, expected %ld\n", name, op, bad, want_bad);
    printf("%s op %d: %zu vectors (%ld flagged, %d with idx >= m), %d failures\n", name, op, n, want_bad, out_of_range, fails);
    return fails + (n < 10) + (out_of_range < 3);
}
int run_rejection(int curve, const char* name, const Keys& k) {
    Keys bad = k;
    bad.py[32] ^= 1;                        // key 1 leaves the curve
    memset(&bad.px[64], 0, 32), memset(&bad.py[64], 0, 32);   // key 2 is the neutral element
    memset(&bad.px[96], 0xFF, 32);          // key 3: x = 2^256 - 1 >= p
    std::vector<uint8_t> perr(k.m, 0xAA), tab(emut_table_bytes(k.m), 0xAA);
    const long rc = emut_build(curve, bad.px.data(), bad.py.data(), k.m, tab.data(), perr.data());
    int fails = rc != 3 || perr[0] != 0 || perr[1] != WIRE_NOT_ON_CURVE || perr[2] != WIRE_INFINITY || perr[3] != WIRE_COORD_RANGE;
    for (uint8_t v : tab) fails += v != 0xAA;   // nothing is built
    fails += emut_build(curve, k.px.data(), k.py.data(), 0, tab.data(), perr.data()) != -1;
    printf("%s: rejected points, %d failures\n", name, fails);
    return fails;
}
template <class CV>
int run_random(const char* name, const Keys& keys) {
    const size_t n = 64;
    const int curve = CV::kAZero ? 0 : 1;
    const Aff G = host::generator_cv<CV>();
    std::vector<uint8_t> a(32 * n), b(32 * n);
    std::vector<uint32_t> idx(n);
    host::SplitMix64 rng{0x7AB1Eu};
    for (size_t i = 0; i < n; i++) {
        for (auto* v : {&a, &b}) {
            const U256 x = host::u256_from_u64(rng.next(), rng.next(), rng.next(), rng.next());
            memcpy(v->data() + 32 * i, x.w, 32);
        }
        idx[i] = (uint32_t)(rng.next() % keys.m);
    }
    int fails = 0;
    for (int op = 0; op < 2; op++) {
        std::vector<uint8_t> ox(32 * n, 0xAA), oy(32 * n, 0xAA), err(n, 0xAA);
        if (emut_call(curve, op, keys.tab.data(), idx.data(), (uint32_t)keys.m, a.data(), b.data(), nullptr, ox.data(), oy.data(), n, err.data()))
            fails++;
        for (size_t i = 0; i < n; i++) {
            Aff P;
            P.x = load_packed(keys.px.data(), idx[i]), P.y = load_packed(keys.py.data(), idx[i]);
            Jac acc = jac_from_aff(host::scalar_mul_cv<CV>(sign_scalar<CV>(b.data(), i), P));
            if (op == 1) acc = jac_add_cv<CV, false, true>(acc, jac_from_aff(host::scalar_mul_cv<CV>(sign_scalar<CV>(a.data(), i), G))).p;
            const Aff w = host::jac_to_aff_cv<CV>(acc);
            if (!u256_eq(w.x, load_packed(ox.data(), i)) || !u256_eq(w.y, load_packed(oy.data(), i)))
                if (fails++ < 10) fprintf(stderr, "%s op %d: random element %zu differs\n", name, op, i);
        }
    }
    printf("%s: %zu random elements x 2 calls, %d failures\n", name, n, fails);
    return fails;
}
}  // namespace

int main() {
    int fails = 0;
    for (int curve = 0; curve < 2; curve++) {
        const char* name = curve ? "p256" : "secp256k1";
        const Keys k = build_keys(curve, fails);
        if (k.m != 4) fails++;
        fails += run_generator(curve, name, k);
        for (int op = 0; op < 3; op++) fails += run_vectors(curve, op, name, k);
        fails += run_rejection(curve, name, k);
        fails += curve ? run_random<P256>(name, k) : run_random<Secp256k1>(name, k);
    }
    return fails ? 1 : 0;
}

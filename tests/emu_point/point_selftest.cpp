// Stand-alone run of the three point-arithmetic bodies under the address and undefined-behaviour sanitizers (and the
// limb-bound tracker, and the 128-bit bound of the GLV halves), both curves, every plan.  Part 1: three cases of every kind of
// input set X (tests/point_arith_inputs.py, compiled in through point_vectors.inc) against its compiled-in expectation -- the
// code, the x of the result and the parity of its y, which must be on the curve -- flagged kinds included.  Part 2: 128
// random (k, a, b, t, u) per curve and plan with P = t G, Q = u G against the double-and-add multiplication of
// host::scalar_mul_cv: k P = (k t) G, a G + b P = (a + b t) G, P + Q = (t + u) G.
// Exit status 0 = all held.
#include <cstdio>
#include <cstring>

#include "p2e_emu_point.cpp"

namespace {
// point_vectors.inc is read twice: its P lines are the distinct operands, its V lines the cases (p, q: indices into the P lines)
struct Pnt {
    int curve;
    const char *x, *y;
};
struct Vec {
    int curve, op;
    const char *a, *b;
    int p, q;
    const char* outx;
    int outy_odd, err;
};
#define V(...)
#define P(curve, x, y) {curve, x, y},
const Pnt POINTS[] = {
#include "point_vectors.inc"
};
#undef P
#undef V
#define P(...)
#define V(curve, op, a, b, p, q, outx, outy_odd, err) {curve, op, a, b, p, q, outx, outy_odd, err},
const Vec VECTORS[] = {
#include "point_vectors.inc"
};
#undef P
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
long call(int curve, int op, int plan, const uint8_t* a, const uint8_t* b, const uint8_t* px, const uint8_t* py, const uint8_t* qx,
          const uint8_t* qy, uint8_t* ox, uint8_t* oy, size_t n, uint8_t* err) {
    if (op == 0) return emup_mul(curve, plan, b, px, py, ox, oy, n, err);
    if (op == 1) return emup_lincomb(curve, plan, a, b, px, py, ox, oy, n, err);
    return emup_add(curve, px, py, qx, qy, ox, oy, n, err);
}
int run_vectors(int curve, int op, int plan, const char* name) {
    std::vector<uint8_t> a, b, px, py, qx, qy, wx, wodd, werr;
    for (const Vec& t : VECTORS) {
        if (t.curve != curve || t.op != op) continue;
        const size_t o = werr.size();
        for (auto* v : {&a, &b, &px, &py, &qx, &qy, &wx}) v->resize(32 * (o + 1));
        put_hex(&a[32 * o], t.a), put_hex(&b[32 * o], t.b), put_hex(&px[32 * o], POINTS[t.p].x), put_hex(&py[32 * o], POINTS[t.p].y);
        put_hex(&qx[32 * o], POINTS[t.q].x), put_hex(&qy[32 * o], POINTS[t.q].y), put_hex(&wx[32 * o], t.outx);
        wodd.push_back((uint8_t)t.outy_odd);
        werr.push_back((uint8_t)t.err);
    }
    const size_t n = werr.size();
    std::vector<uint8_t> ox(32 * n, 0xAA), oy(32 * n, 0xAA), err(n, 0xAA);
    const long bad = call(curve, op, plan, a.data(), b.data(), px.data(), py.data(), qx.data(), qy.data(), ox.data(), oy.data(), n, err.data());
    int fails = 0;
    long want_bad = 0;
    for (size_t i = 0; i < n; i++) {
        want_bad += werr[i] != 0;
        Aff got;
        got.x = load_packed(ox.data(), i), got.y = load_packed(oy.data(), i);
        // the expected point is given by its x and the parity of its y; flagged: zeros in both
        const bool on = curve ? host::aff_on_curve_cv<P256>(got) : host::aff_on_curve_cv<Secp256k1>(got);
        const bool y_ok = werr[i] ? u256_is_zero(got.y) : (on && (got.y.w[0] & 1u) == wodd[i]);
        if (err[i] != werr[i] || memcmp(&ox[32 * i], &wx[32 * i], 32) || !y_ok)
            if (fails++ < 10) fprintf(stderr, "%s op %d plan %d: vector %zu differs (err %d, expected %d)\n", name, op, plan, i, err[i], werr[i]);
    }
    if (bad != want_bad) fails++, fprintf(stderr, "%s op %d plan %d: count %ld, expected %ld\n", name, op, plan, bad, want_bad);
    printf("%s op %d plan %d: %zu vectors (%ld flagged), %d failures\n", name, op, plan, n, want_bad, fails);
    return fails + (n < 20);
}
template <class CV>
int run_random(int plan, const char* name) {
    typedef typename CV::Fn Fn;
    const size_t n = 128;
    const int curve = CV::kAZero ? 0 : 1;
    const Aff G = host::generator_cv<CV>();
    std::vector<uint8_t> k(32 * n), a(32 * n), b(32 * n), px(32 * n), py(32 * n), qx(32 * n), qy(32 * n);
    std::vector<U256> t(n), u(n);
    host::SplitMix64 rng{0x90147u + (unsigned)plan};
    auto draw = [&]() { return host::u256_from_u64(rng.next(), rng.next(), rng.next(), rng.next()); };
    for (size_t i = 0; i < n; i++) {
        for (auto* v : {&k, &a, &b}) {
            const U256 x = draw();
            memcpy(v->data() + 32 * i, x.w, 32);
        }
        t[i] = fe_canon<Fn>(draw()), u[i] = fe_canon<Fn>(draw());
        const Aff P = host::scalar_mul_cv<CV>(t[i], G), Q = host::scalar_mul_cv<CV>(u[i], G);
        memcpy(&px[32 * i], P.x.w, 32), memcpy(&py[32 * i], P.y.w, 32), memcpy(&qx[32 * i], Q.x.w, 32), memcpy(&qy[32 * i], Q.y.w, 32);
    }
    int fails = 0;
    for (int op = 0; op < 3; op++) {
        std::vector<uint8_t> ox(32 * n, 0xAA), oy(32 * n, 0xAA), err(n, 0xAA);
        if (call(curve, op, plan, a.data(), op == 0 ? k.data() : b.data(), px.data(), py.data(), qx.data(), qy.data(), ox.data(), oy.data(), n,
                 err.data()))
            fails++;
        for (size_t i = 0; i < n; i++) {
            const U256 kk = sign_scalar<CV>(k.data(), i), aa = sign_scalar<CV>(a.data(), i), bb = sign_scalar<CV>(b.data(), i);
            const U256 e = op == 0 ? fe_mul<Fn>(kk, t[i]) : op == 1 ? fe_add<Fn>(aa, fe_mul<Fn>(bb, t[i])) : fe_add<Fn>(t[i], u[i]);
            const Aff w = host::scalar_mul_cv<CV>(e, G);
            if (!u256_eq(w.x, load_packed(ox.data(), i)) || !u256_eq(w.y, load_packed(oy.data(), i)))
                if (fails++ < 10) fprintf(stderr, "%s op %d plan %d: random element %zu differs\n", name, op, plan, i);
        }
    }
    printf("%s plan %d: %zu random elements x 3 calls, %d failures\n", name, plan, n, fails);
    return fails;
}
}  // namespace

int main() {
    int fails = 0;
    for (int curve = 0; curve < 2; curve++) {
        const char* name = curve ? "p256" : "secp256k1";
        for (int plan = 0; plan <= (curve ? 1 : 2); plan++) {
            fails += run_vectors(curve, 0, plan, name) + run_vectors(curve, 1, plan, name);
            fails += curve ? run_random<P256>(plan, name) : run_random<Secp256k1>(plan, name);
        }
        fails += run_vectors(curve, 2, 0, name);
    }
    if (emup_mul(1, MUL_PLAN_GLV, nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr) != -1) fails++;   // GLV on P-256 is refused
    return fails ? 1 : 0;
}

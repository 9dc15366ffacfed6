// Stand-alone run of a P + b Q and of the DLEQ bodies under the address and undefined-behaviour sanitizers (and the limb-bound
// tracker), on a fixed set made from nothing but small integers; every buffer is a heap allocation of exactly the bytes the call
// may touch, so a lane that read or wrote beyond its element would stop the program.
//   1. a P + b Q under every plan on both curves equals k P, k Q and P + Q of the existing bodies, for P = p G, Q = q G with Q = P,
//      Q = -P and a zero scalar among them.
//   2. N shares are proven and verified (with and without a message); a flipped bit of e, of s, and A in the place of C are rejected.
// Exit status 0 = all held.
#include <cstdio>
#include <cstring>

#include "p2e_emu_dleq.cpp"

namespace {
typedef std::vector<uint8_t> Bytes;
constexpr size_t N = 9;

void put_u32(Bytes& b, size_t i, uint32_t v) { memcpy(b.data() + 32 * i, &v, 4); }
template <class CV>
const Aff* table_of();
template <>
const Aff* table_of<Secp256k1>() {
    return gen_table();
}
template <>
const Aff* table_of<P256>() {
    static const std::vector<Aff> t = host::fixed_base_table_cv<P256>(host::generator_cv<P256>());
    return t.data();
}
// the public keys of small secret keys, little-endian (x, y)
template <class CV>
void public_keys(const Bytes& sk, Bytes& x, Bytes& y) {
    for (size_t i = 0; i < sk.size() / 32; i++) body_public_key<CV, SIGN_PLAN_LANE>(table_of<CV>(), sk.data(), x.data(), y.data(), i, 0);
}

template <class CV>
int lincomb2_set(int curve) {
    int fails = 0;
    Bytes p(32 * N, 0), q(32 * N, 0), a(32 * N, 0), b(32 * N, 0);
    for (size_t i = 0; i < N; i++) put_u32(p, i, 3 + 2 * (uint32_t)i), put_u32(q, i, 1000 + 7 * (uint32_t)i), put_u32(a, i, 0x9E3779B9u * (uint32_t)(i + 1)),
        put_u32(b, i, 0x85EBCA6Bu * (uint32_t)(i + 2));
    for (size_t i = 0; i < N; i++) memset(a.data() + 32 * i + 4, 0x5A + (int)i, 27), memset(b.data() + 32 * i + 4, 0xC3 - (int)i, 27);   // wide scalars
    put_u32(q, 1, 5);                  // Q = P
    memset(a.data() + 32 * 2, 0, 32);  // a = 0
    Bytes px(32 * N), py(32 * N), qx(32 * N), qy(32 * N);
    public_keys<CV>(p, px, py), public_keys<CV>(q, qx, qy);
    memcpy(a.data() + 32 * 3, b.data() + 32 * 3, 32), memcpy(qx.data() + 32 * 3, px.data() + 32 * 3, 32);   // a = b, Q = -P: the neutral sum
    store_packed(qy.data(), 3, fe_neg<typename CV::Fp>(load_packed(py.data(), 3)));
    Bytes ax(32 * N), ay(32 * N), bx(32 * N), by(32 * N), wx(32 * N), wy(32 * N), werr(N);
    for (size_t i = 0; i < N; i++) {
        body_point_mul<CV, MUL_PLAN_PLAIN>(a.data(), px.data(), py.data(), ax.data(), ay.data(), i);
        body_point_mul<CV, MUL_PLAN_PLAIN>(b.data(), qx.data(), qy.data(), bx.data(), by.data(), i);
        werr[i] = body_point_add<CV>(ax.data(), ay.data(), bx.data(), by.data(), wx.data(), wy.data(), i);
    }
    if (werr[3] != WIRE_INFINITY) fprintf(stderr, "FAIL curve %d: the set's neutral sum is not one\n", curve), fails++;
    for (int plan = MUL_PLAN_AUTO; plan <= MUL_PLAN_GLV; plan++) {
        if (plan == MUL_PLAN_GLV && curve != 0) continue;
        Bytes ox(32 * N, 0xAA), oy(32 * N, 0xAA), err(N, 0xAA);
        emud_lincomb2(curve, plan, a.data(), b.data(), px.data(), py.data(), qx.data(), qy.data(), ox.data(), oy.data(), N, err.data());
        if (ox != wx || oy != wy || err != werr) fprintf(stderr, "FAIL curve %d plan %d: a P + b Q differs from mul, mul, add\n", curve, plan), fails++;
    }
    return fails;
}

int dleq_set(bool with_msg) {
    int fails = 0;
    Bytes a(32 * N, 0), b(32 * N, 0), aux(32 * N), msg(32 * N);
    for (size_t i = 0; i < N; i++) put_u32(a, i, 1 + (uint32_t)i), put_u32(b, i, 77 + 5 * (uint32_t)i), memset(aux.data() + 32 * i, 0x10 + (int)i, 32),
        memset(msg.data() + 32 * i, 0xE0 + (int)i, 32);
    Bytes ax(32 * N), ay(32 * N), bx(32 * N), by(32 * N);
    public_keys<Secp256k1>(a, ax, ay), public_keys<Secp256k1>(b, bx, by);
    const uint8_t* m = with_msg ? msg.data() : nullptr;
    Bytes proof(64 * N, 0xAA), cx(32 * N, 0xAA), cy(32 * N, 0xAA), err(N, 0xAA), valid(N, 0xAA);
    if (emud_prove(a.data(), bx.data(), by.data(), aux.data(), m, proof.data(), cx.data(), cy.data(), N, err.data()) != 0)
        fprintf(stderr, "FAIL prove: a flagged element\n"), fails++;
    Bytes only(64 * N, 0xAA);   // without the share: the same proofs
    emud_prove(a.data(), bx.data(), by.data(), aux.data(), m, only.data(), nullptr, nullptr, N, err.data());
    if (only != proof) fprintf(stderr, "FAIL prove: the proof depends on whether C is asked for\n"), fails++;
    auto verdicts = [&](const Bytes& pf, const Bytes& x, const Bytes& y, const uint8_t* mm, uint8_t want, const char* what) {
        Bytes e2(N, 0xAA), v(N, 0xAA);
        emud_verify(ax.data(), ay.data(), bx.data(), by.data(), x.data(), y.data(), pf.data(), mm, N, e2.data(), v.data());
        for (size_t i = 0; i < N; i++)
            if (e2[i] != 0 || v[i] != want) {
                fprintf(stderr, "FAIL %s: element %zu has code %d, valid %d\n", what, i, e2[i], v[i]);
                return 1;
            }
        return 0;
    };
    fails += verdicts(proof, cx, cy, m, 1, "verify of fresh proofs");
    fails += verdicts(proof, cx, cy, with_msg ? nullptr : msg.data(), 0, "verify under the other message form");
    Bytes bad = proof;
    for (size_t i = 0; i < N; i++) bad[64 * i + 31] ^= 1;
    fails += verdicts(bad, cx, cy, m, 0, "verify with a flipped bit of e");
    bad = proof;
    for (size_t i = 0; i < N; i++) bad[64 * i + 63] ^= 1;   // (s stays below n but for s = n - 1 ^ 1: not in this set)
    fails += verdicts(bad, cx, cy, m, 0, "verify with a flipped bit of s");
    fails += verdicts(proof, ax, ay, m, 0, "verify with A for C");
    return fails;
}
}  // namespace

int main() {
    int fails = lincomb2_set<Secp256k1>(0) + lincomb2_set<P256>(1);
    fails += dleq_set(false) + dleq_set(true);
    if (fails) return 1;
    printf("dleq_selftest: a P + b Q on two curves, %zu proofs with and without a message ok\n", N);
    return 0;
}

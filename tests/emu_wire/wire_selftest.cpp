// Stand-alone run of the key and signature codec bodies under the address and undefined-behaviour sanitizers.
//   1. published bytes: the SEC 2 generators of both curves decode to the library's constants and encode back;
//   2. the read rule: every element of the edge sets below is decoded from a heap block that begins at the aligned word
//      holding its first byte and ends with the aligned word holding its last byte, at every misalignment 0 .. 3 of the
//      first byte -- a read of any word outside those is a heap-buffer-overflow report -- and an element whose length alone
//      decides it (empty, too long, no valid length) is given NO readable byte at all.  Then all elements are decoded as
//      one concatenated buffer from such a block, and each must give what it gave alone;
//   3. the write bounds: every encoder writes into a heap block of exactly n x stride bytes at every misalignment;
//   4. decode(encode(x)) = x over the values of the edge sets.
// Each case carries the code the header's rules give it.  Exit status 0 = all held.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "p2e_emu_wire.cpp"

namespace {
typedef std::vector<uint8_t> Bytes;
int fails = 0;
void fail(const char* what, long a = -1, long b = -1, long c = -1) {
    if (fails++ < 12) fprintf(stderr, "wire_selftest: %s (%ld, %ld, %ld)\n", what, a, b, c);
}
Bytes from_hex(const char* h) {
    Bytes out;
    for (size_t i = 0; h[i] && h[i + 1]; i += 2) {
        unsigned v;
        sscanf(h + i, "%2x", &v);
        out.push_back((uint8_t)v);
    }
    return out;
}
Bytes cat(std::initializer_list<Bytes> parts) {
    Bytes out;
    for (const Bytes& p : parts) out.insert(out.end(), p.begin(), p.end());
    return out;
}
Bytes be32(const U256& v) {
    Bytes out(32);
    wire_store_be256(out.data(), v);
    return out;
}
U256 from_be(const Bytes& b, size_t at) {
    U256 r;
    for (int j = 0; j < 8; j++) {
        const uint8_t* p = b.data() + at + 28 - 4 * j;
        r.w[j] = ((u32)p[0] << 24) | ((u32)p[1] << 16) | ((u32)p[2] << 8) | p[3];
    }
    return r;
}
template <class MOD>
U256 modulus_plus(int d) {   // m + d for a small d of either sign
    U256 m = hash_modulus<MOD>();
    long long c = d;
    for (int j = 0; j < 8; j++) {
        c += m.w[j];
        m.w[j] = (u32)c;
        c >>= 32;
    }
    return m;
}

// A heap block of exactly the aligned words that hold `len` bytes starting at misalignment `mis`; it sits at the END of its
// allocation (the allocator rounds sizes up), so the word behind its last one is not addressable.  len = 0: no readable
// byte -- first() points at the end of a block of its own.
struct Exact {
    uint8_t* raw;
    uint8_t* base;
    Exact(const uint8_t* src, size_t len, unsigned mis) {
        const size_t block = (mis + len + 3) / 4 * 4, total = block ? (block + 15) / 16 * 16 : 16;
        raw = (uint8_t*)aligned_alloc(16, total);
        base = raw + (total - block) + (len ? mis : 0);
        if (len) memcpy(base, src, len);
    }
    ~Exact() { free(raw); }
    Exact(const Exact&) = delete;
};

struct Case {
    Bytes b;
    int code;
    const char* what;
};
struct Out {
    uint8_t e;
    alignas(4) uint8_t a[32], b[32];
    bool operator==(const Out& o) const { return e == o.e && !memcmp(a, o.a, 32) && !memcmp(b, o.b, 32); }
};
// length alone decides: the lane may read nothing
bool key_len_ok(size_t n) { return n == 1 || n == 33 || n == 65; }
bool der_len_ok(size_t n) { return n >= 8 && n <= 72; }

Out decode_alone(bool key, int curve, unsigned flags, const Bytes& b, unsigned mis) {
    const bool readable = key ? key_len_ok(b.size()) : der_len_ok(b.size());
    Exact blk(b.data(), readable ? b.size() : 0, mis);
    const uint64_t off[2] = {0, b.size()};
    Out o;
    memset(&o, 0xAA, sizeof o);
    if (key)
        emuw_point_decode(curve, blk.base, off, o.a, o.b, 1, &o.e);
    else
        emuw_sig_decode(curve, SIG_DER, flags, blk.base, off, o.a, o.b, nullptr, 1, &o.e);
    return o;
}
void run_cases(bool key, int curve, unsigned flags, const std::vector<Case>& cases) {
    std::vector<Out> alone;
    for (size_t i = 0; i < cases.size(); i++) {
        alone.push_back(decode_alone(key, curve, flags, cases[i].b, 0));
        if (alone[i].e != cases[i].code) fail(cases[i].what, curve, alone[i].e, cases[i].code);
        for (unsigned mis = 1; mis < 4; mis++)
            if (!(decode_alone(key, curve, flags, cases[i].b, mis) == alone[i])) fail("result depends on the alignment", curve, (long)i, mis);
        if (alone[i].e)
            for (int j = 0; j < 32; j++)
                if (alone[i].a[j] || alone[i].b[j]) fail("flagged element did not write zeros", curve, (long)i);
    }
    // the same elements as one buffer; a reversed pair of offsets in the middle
    Bytes all;
    std::vector<uint64_t> off(1, 0);
    for (const Case& c : cases) {
        all.insert(all.end(), c.b.begin(), c.b.end());
        off.push_back(all.size());
    }
    const size_t n = cases.size();
    for (unsigned mis = 0; mis < 4; mis++) {
        Exact blk(all.data(), all.size(), mis);
        std::vector<uint8_t> a(32 * n), b(32 * n), e(n);
        const long bad = key ? emuw_point_decode(curve, blk.base, off.data(), a.data(), b.data(), n, e.data())
                             : emuw_sig_decode(curve, SIG_DER, flags, blk.base, off.data(), a.data(), b.data(), nullptr, n, e.data());
        long want_bad = 0;
        for (size_t i = 0; i < n; i++) {
            want_bad += alone[i].e != 0;
            if (e[i] != alone[i].e || memcmp(&a[32 * i], alone[i].a, 32) || memcmp(&b[32 * i], alone[i].b, 32))
                fail("result depends on the position", curve, (long)i, mis);
        }
        if (bad != want_bad) fail("return value", curve, bad, want_bad);
    }
    const uint64_t rev[3] = {40, 7, 7};   // offsets[1] < offsets[0]: empty, nothing read
    alignas(4) uint8_t a[64], b[64];
    uint8_t e[2];
    Exact none(nullptr, 0, 0);
    const long bad = key ? emuw_point_decode(curve, none.base, rev, a, b, 2, e) : emuw_sig_decode(curve, SIG_DER, flags, none.base, rev, a, b, nullptr, 2, e);
    if (bad != 2 || e[0] != WIRE_BAD_LENGTH || e[1] != WIRE_BAD_LENGTH) fail("reversed offsets", curve, bad, e[0]);
}

template <class CV>
void keys(int curve, const char* g_comp, const char* g_unc) {
    typedef typename CV::Fp F;
    const Bytes comp = from_hex(g_comp), unc = from_hex(g_unc);
    const Bytes gx(unc.begin() + 1, unc.begin() + 33), gy(unc.begin() + 33, unc.end());
    const U256 x = from_be(unc, 1), y = from_be(unc, 33);
    // 1. published bytes
    {
        const Out c = decode_alone(true, curve, 0, comp, 1), u = decode_alone(true, curve, 0, unc, 3);
        if (c.e || u.e || !(c == u) || !u256_eq(load_packed(c.a, 0), x) || !u256_eq(load_packed(c.b, 0), y)) fail("published generator", curve);
        Bytes o33(33), o65(65);
        uint8_t e[1];
        alignas(4) uint8_t px[32], py[32];
        store_packed(px, 0, x), store_packed(py, 0, y);
        emuw_point_encode(curve, SEC1_COMPRESSED, px, py, o33.data(), 1, e);
        emuw_point_encode(curve, SEC1_UNCOMPRESSED, px, py, o65.data(), 1, e);
        if (o33 != comp || o65 != unc) fail("generator does not encode to the published bytes", curve);
    }
    // 2. the edge set
    std::vector<Case> cs;
    cs.push_back({comp, WIRE_OK, "G compressed"});
    cs.push_back({unc, WIRE_OK, "G uncompressed"});
    Bytes other = comp;
    other[0] ^= 1;
    cs.push_back({other, WIRE_OK, "-G compressed"});
    const U256 p = hash_modulus<F>();
    cs.push_back({cat({{4}, gx, be32(fe_neg<F>(y))}), WIRE_OK, "-G uncompressed"});
    cs.push_back({cat({{4}, gx, be32(modulus_plus<F>(0))}), WIRE_COORD_RANGE, "y = p"});
    cs.push_back({cat({{4}, be32(p), gy}), WIRE_COORD_RANGE, "x = p uncompressed"});
    cs.push_back({cat({{2}, be32(p)}), WIRE_COORD_RANGE, "x = p compressed"});
    cs.push_back({cat({{3}, Bytes(32, 0xFF)}), WIRE_COORD_RANGE, "x = 2^256 - 1"});
    cs.push_back({cat({{4}, gx, Bytes(32, 0xFF)}), WIRE_COORD_RANGE, "y = 2^256 - 1"});
    U256 y1 = y;
    y1.w[0] ^= 1;
    cs.push_back({cat({{4}, gx, be32(y1)}), WIRE_NOT_ON_CURVE, "y + 1"});
    cs.push_back({cat({{4}, Bytes(32, 0), Bytes(32, 0)}), WIRE_NOT_ON_CURVE, "04 || 0 || 0"});
    {   // an abscissa whose cubic is no square, found by search
        int found = -1;
        for (int v = 1; v < 64 && found < 0; v++) {
            Bytes b(33, 0);
            b[0] = 2, b[32] = (uint8_t)v;
            if (decode_alone(true, curve, 0, b, 0).e == WIRE_NOT_ON_CURVE) found = v;
        }
        if (found < 0) fail("no non-residue abscissa below 64", curve);
        Bytes b(33, 0);
        b[0] = 3, b[32] = (uint8_t)found;
        cs.push_back({b, WIRE_NOT_ON_CURVE, "non-residue abscissa"});
        b[0] = 2;
        cs.push_back({b, WIRE_NOT_ON_CURVE, "non-residue abscissa, even"});
    }
    const uint8_t prefixes[] = {0, 1, 5, 6, 7, 0xFF};
    for (uint8_t pre : prefixes) {
        cs.push_back({cat({{pre}, gx}), WIRE_BAD_PREFIX, "bad prefix at 33"});
        cs.push_back({cat({{pre}, gx, gy}), WIRE_BAD_PREFIX, "bad prefix at 65"});
    }
    cs.push_back({cat({{4}, gx}), WIRE_BAD_PREFIX, "04 at 33"});
    cs.push_back({cat({{2}, gx, gy}), WIRE_BAD_PREFIX, "02 at 65"});
    cs.push_back({cat({{3}, gx, gy}), WIRE_BAD_PREFIX, "03 at 65"});
    cs.push_back({{0}, WIRE_INFINITY, "00"});
    cs.push_back({{2}, WIRE_BAD_PREFIX, "02 alone"});
    cs.push_back({{4}, WIRE_BAD_PREFIX, "04 alone"});
    const size_t lens[] = {0, 2, 32, 34, 64, 66, 1000};
    for (size_t n : lens) cs.push_back({Bytes(n, 2), WIRE_BAD_LENGTH, "length"});
    run_cases(true, curve, 0, cs);
    // 3. write bounds of the encoder, and the round trip through both forms
    const size_t n = 7;
    std::vector<uint8_t> px(32 * n), py(32 * n), e(n);
    for (size_t i = 0; i < n; i++) {
        const Case& c = cs[i < 4 ? i : 0];
        const Out o = decode_alone(true, curve, 0, c.b, 0);
        memcpy(&px[32 * i], o.a, 32), memcpy(&py[32 * i], o.b, 32);
    }
    memset(&px[32 * 4], 0, 32), memset(&py[32 * 4], 0, 32);          // (0, 0): INFINITY
    memset(&px[32 * 5], 0xFF, 32);                                   // COORD_RANGE
    py[32 * 6] ^= 1;                                                 // NOT_ON_CURVE
    const uint8_t want[n] = {0, 0, 0, 0, WIRE_INFINITY, WIRE_COORD_RANGE, WIRE_NOT_ON_CURVE};
    for (int form = 0; form < 2; form++)
        for (unsigned mis = 0; mis < 4; mis++) {
            const size_t stride = form ? 65 : 33;
            std::vector<uint8_t> buf(n * stride + mis, 0xAA);   // (a vector's block ends with its last byte)
            uint8_t* out = buf.data() + mis;
            if (emuw_point_encode(curve, form, px.data(), py.data(), out, n, e.data()) != 3) fail("encoder's return value", curve, form);
            for (size_t i = 0; i < n; i++) {
                if (e[i] != want[i]) fail("encoder's code", curve, (long)i, e[i]);
                if (want[i])
                    for (size_t j = 0; j < stride; j++)
                        if (out[stride * i + j]) fail("flagged key not zero", curve, (long)i);
            }
            std::vector<uint64_t> off;
            for (size_t i = 0; i <= 4; i++) off.push_back(stride * i);
            Exact blk(out, 4 * stride, mis);
            std::vector<uint8_t> bx(32 * 4), by(32 * 4), be(4);
            if (emuw_point_decode(curve, blk.base, off.data(), bx.data(), by.data(), 4, be.data()) != 0) fail("round trip flagged", curve, form);
            if (memcmp(bx.data(), px.data(), 128) || memcmp(by.data(), py.data(), 128)) fail("decode(encode(x)) != x", curve, form, mis);
        }
}

Bytes der_of(const Bytes& r, const Bytes& s) {
    return cat({{0x30, (uint8_t)(r.size() + s.size() + 4), 2, (uint8_t)r.size()}, r, {2, (uint8_t)s.size()}, s});
}
template <class CV>
void sigs(int curve) {
    typedef typename CV::Fn Fn;
    Bytes r32b(32), s32b(32);
    for (int j = 0; j < 32; j++) r32b[j] = (uint8_t)(0x11 + 3 * j), s32b[j] = (uint8_t)(0x25 + 5 * j);   // both below 2^255
    const Bytes ok = der_of(r32b, s32b);
    const Bytes n_be = be32(hash_modulus<Fn>()), n_minus_1 = be32(modulus_plus<Fn>(-1));
    const Bytes hi33 = cat({{0}, n_minus_1});                                   // n - 1 needs its 00
    Bytes neg = r32b, big33 = cat({{1}, Bytes(32, 0)});
    neg[0] |= 0x80;
    auto with = [&](size_t at, uint8_t v) {
        Bytes b = ok;
        b[at] = v;
        return b;
    };
    std::vector<Case> cs;
    cs.push_back({ok, WIRE_OK, "valid"});
    cs.push_back({der_of({1}, {1}), WIRE_OK, "8 bytes"});
    cs.push_back({der_of(hi33, hi33), WIRE_OK, "72 bytes: r = s = n - 1"});
    cs.push_back({der_of({0, 0x80}, {0x7F}), WIRE_OK, "00 80"});
    cs.push_back({der_of(cat({{0}, n_be}), {1}), WIRE_SCALAR_RANGE, "r = n"});
    cs.push_back({der_of({1}, cat({{0}, n_be})), WIRE_SCALAR_RANGE, "s = n"});
    cs.push_back({der_of({0}, {1}), WIRE_SCALAR_RANGE, "r = 0 as 02 01 00"});
    cs.push_back({der_of({1}, {0}), WIRE_SCALAR_RANGE, "s = 0"});
    cs.push_back({der_of(big33, {1}), WIRE_SCALAR_RANGE, "r = 2^256"});
    cs.push_back({der_of({1}, cat({{0}, Bytes(32, 0xFF)})), WIRE_SCALAR_RANGE, "s = 2^256 - 1"});
    cs.push_back({der_of(neg, s32b), WIRE_DER_INTEGER, "negative r"});
    cs.push_back({der_of(r32b, neg), WIRE_DER_INTEGER, "negative s"});
    cs.push_back({der_of({0x80}, {1}), WIRE_DER_INTEGER, "one negative byte"});
    cs.push_back({der_of(cat({{0}, r32b}), s32b), WIRE_DER_INTEGER, "padded r"});
    cs.push_back({der_of(r32b, {0, 0}), WIRE_DER_INTEGER, "00 00"});
    cs.push_back({der_of({0, 0x7F}, {1}), WIRE_DER_INTEGER, "00 7f"});
    cs.push_back({der_of({0}, neg), WIRE_DER_INTEGER, "r = 0 and a negative s"});
    cs.push_back({with(0, 0x31), WIRE_DER_SYNTAX, "tag 31"});
    cs.push_back({with(2, 0x03), WIRE_DER_SYNTAX, "first integer tag 03"});
    cs.push_back({with(4 + 32, 0x03), WIRE_DER_SYNTAX, "second integer tag 03"});
    cs.push_back({with(1, ok[1] + 1), WIRE_DER_SYNTAX, "b[1] + 1"});
    cs.push_back({with(1, ok[1] - 1), WIRE_DER_SYNTAX, "b[1] - 1"});
    cs.push_back({cat({ok, {1}}), WIRE_DER_SYNTAX, "trailing byte"});
    cs.push_back({cat({with(1, ok[1] + 1), {1}}), WIRE_DER_SYNTAX, "trailing byte counted in b[1]"});
    cs.push_back({cat({{0x30, 0x81, ok[1]}, Bytes(ok.begin() + 2, ok.end())}), WIRE_DER_SYNTAX, "long-form length"});
    cs.push_back({with(3, 0), WIRE_DER_SYNTAX, "lr = 0"});
    cs.push_back({with(3, (uint8_t)(ok.size() - 6)), WIRE_DER_SYNTAX, "lr + 7 > L"});
    cs.push_back({with(3, 0xFF), WIRE_DER_SYNTAX, "lr = 255"});
    cs.push_back({der_of(cat({{0, 0}, r32b}), {1}), WIRE_DER_SYNTAX, "34-byte integer"});
    cs.push_back({Bytes{0x30, 6, 2, 33, 1, 2, 1, 1}, WIRE_DER_SYNTAX, "lr = 33 in 8 bytes"});
    cs.push_back({with(5 + 32, 0), WIRE_DER_SYNTAX, "ls = 0"});
    cs.push_back({with(5 + 32, 31), WIRE_DER_SYNTAX, "ls short"});
    const size_t lens[] = {0, 1, 7, 73, 1000};
    for (size_t n : lens) cs.push_back({Bytes(n, 0x30), WIRE_BAD_LENGTH, "length"});
    for (unsigned flags = 0; flags < 3; flags++) {
        std::vector<Case> f = cs;
        if (flags == SIG_REQUIRE_LOW_S) f[2].code = WIRE_HIGH_S;
        run_cases(false, curve, flags, f);
    }
    // the values behind the valid cases, through every form and back; blocks of exactly n x stride bytes
    const size_t n = 6;
    std::vector<uint8_t> r(32 * n, 0), s(32 * n, 0), v = {0, 1, 2, 3, 27, 255}, e(n);
    const U256 rv = from_be(r32b, 0), sv = from_be(s32b, 0), top = modulus_plus<Fn>(-1), one = u256_small(1), zero = u256_zero();
    const U256 rs[n][2] = {{rv, sv}, {one, one}, {top, top}, {sv, top}, {zero, one}, {rv, hash_modulus<Fn>()}};
    for (size_t i = 0; i < n; i++) store_packed(r.data(), i, rs[i][0]), store_packed(s.data(), i, rs[i][1]);
    for (int form = 0; form < 3; form++)
        for (unsigned flags = 0; flags < 3; flags += 2)
            for (unsigned mis = 0; mis < 4; mis++) {
                const size_t stride = form == SIG_DER ? 72 : form == SIG_COMPACT64 ? 64 : 65;
                std::vector<uint8_t> buf(n * stride + mis, 0xAA), len(n, 0xAA);
                uint8_t* out = buf.data() + mis;
                if (emuw_sig_encode(curve, form, flags, r.data(), s.data(), v.data(), out, len.data(), n, e.data()) != 2) fail("sig encoder's return value", curve, form);
                for (size_t i = 0; i < n; i++) {
                    if (e[i] != (i < 4 ? 0 : WIRE_SCALAR_RANGE)) fail("sig encoder's code", curve, form, (long)i);
                    if (form == SIG_DER && i >= 4 && len[i] != 0) fail("out_len of a flagged element", curve, (long)i);
                    if (i >= 4)
                        for (size_t j = 0; j < stride; j++)
                            if (out[stride * i + j]) fail("flagged signature not zero", curve, form, (long)i);
                }
                // back: the four valid ones
                std::vector<uint8_t> br(32 * 4), bs(32 * 4), bv(4, 0xAA), be(4);
                long bad;
                if (form == SIG_DER) {
                    Bytes all;
                    std::vector<uint64_t> off(1, 0);
                    for (size_t i = 0; i < 4; i++) {
                        all.insert(all.end(), out + stride * i, out + stride * i + len[i]);
                        off.push_back(all.size());
                        for (size_t j = len[i]; j < stride; j++)
                            if (out[stride * i + j]) fail("DER not zero-filled", curve, (long)i);
                    }
                    if (len[1] != 8 || (flags == 0 && len[2] != 72)) fail("DER lengths", curve, len[1], len[2]);
                    Exact blk(all.data(), all.size(), mis);
                    bad = emuw_sig_decode(curve, form, 0, blk.base, off.data(), br.data(), bs.data(), nullptr, 4, be.data());
                } else {
                    Exact blk(out, 4 * stride, mis);
                    bad = emuw_sig_decode(curve, form, 0, blk.base, nullptr, br.data(), bs.data(), bv.data(), 4, be.data());
                }
                if (bad) fail("sig round trip flagged", curve, form, bad);
                for (size_t i = 0; i < 4; i++) {
                    U256 twin;
                    const bool high = wire_high_s<CV>(rs[i][1], twin);
                    const U256 want_s = flags && high ? twin : rs[i][1];
                    if (!u256_eq(load_packed(br.data(), i), rs[i][0]) || !u256_eq(load_packed(bs.data(), i), want_s)) fail("decode(encode(x)) != x", curve, form, (long)i);
                    if (form == SIG_COMPACT65 && bv[i] != (uint8_t)(v[i] ^ (flags && high))) fail("v", curve, (long)i, bv[i]);
                    if (form != SIG_COMPACT65 && bv[i] != 0xAA) fail("v written outside COMPACT65", curve, form);
                    if ((i == 2 || i == 3) != high) fail("high-s test", curve, (long)i);
                }
            }
}
}  // namespace

int main() {
    keys<Secp256k1>(0, "0279BE667EF9DCBBAC55A06295CE870B07029BFCDB2DCE28D959F2815B16F81798",
                    "0479BE667EF9DCBBAC55A06295CE870B07029BFCDB2DCE28D959F2815B16F81798483ADA7726A3C4655DA4FBFC0E1108A8FD17B448A68554199C47D08FFB10D4B8");
    keys<P256>(1, "036B17D1F2E12C4247F8BCE6E563A440F277037D812DEB33A0F4A13945D898C296",
               "046B17D1F2E12C4247F8BCE6E563A440F277037D812DEB33A0F4A13945D898C2964FE342E2FE1A7F9B8EE7EB4A7C0F9E162BCE33576B315ECECBB6406837BF51F5");
    sigs<Secp256k1>(0);
    sigs<P256>(1);
    printf("wire_selftest: %d failures\n", fails);
    return fails ? 1 : 0;
}

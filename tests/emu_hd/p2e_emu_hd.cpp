// CPU harness of the BIP-32 / HASH160 layer (test infrastructure only): the bodies of csrc/hd.hpp run per element, compiled
// with g++ against the library's headers and the generator table the library uploads.  Hash functions are reached through
// their compression bodies: the harness (or the test) does the padding.
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../plonky2-ecdsa_amd/csrc/consts.hpp"
#include "../../plonky2-ecdsa_amd/csrc/hd.hpp"

using namespace p2e;

namespace {
const Aff* gen_table() { return host::consts().fbtab.data(); }
U256 le256(const uint8_t* p) {
    U256 r;
    for (int j = 0; j < 8; j++) r.w[j] = (u32)p[4 * j] | ((u32)p[4 * j + 1] << 8) | ((u32)p[4 * j + 2] << 16) | ((u32)p[4 * j + 3] << 24);
    return r;
}
void put256(uint8_t* p, const U256& v) {
    for (int j = 0; j < 32; j++) p[j] = (uint8_t)(v.w[j / 4] >> (8 * (j % 4)));
}
}  // namespace

// state: 8 words in and out; block: 128 bytes
extern "C" void emuhd_sha512_compress(uint64_t* state, const uint8_t* block) {
    Sha512State s;
    Sha512Block b;
    for (int j = 0; j < 8; j++) s.h[j] = state[j];
    for (int j = 0; j < 16; j++) {
        b.w[j] = 0;
        for (int k = 0; k < 8; k++) b.w[j] = (b.w[j] << 8) | block[8 * j + k];
    }
    s = sha512_compress(s, b);
    for (int j = 0; j < 8; j++) state[j] = s.h[j];
}
extern "C" void emuhd_sha512_iv(uint64_t* state) {
    const Sha512State s = sha512_iv();
    for (int j = 0; j < 8; j++) state[j] = s.h[j];
}
// state: 5 words in and out; block: 64 bytes
extern "C" void emuhd_ripemd160_compress(uint32_t* state, const uint8_t* block) {
    Ripemd160State s;
    u32 x[16];
    for (int j = 0; j < 5; j++) s.h[j] = state[j];
    for (int j = 0; j < 16; j++) x[j] = (u32)block[4 * j] | ((u32)block[4 * j + 1] << 8) | ((u32)block[4 * j + 2] << 16) | ((u32)block[4 * j + 3] << 24);
    s = ripemd160_compress(s, x);
    for (int j = 0; j < 5; j++) state[j] = s.h[j];
}
extern "C" void emuhd_ripemd160_iv(uint32_t* state) {
    const Ripemd160State s = ripemd160_iv();
    for (int j = 0; j < 5; j++) state[j] = s.h[j];
}
// inner[8] then outer[8]: the constant states of "Bitcoin seed", and those of a 32-byte key
extern "C" void emuhd_seed_key_states(uint64_t* out16) {
    const HmacKey512 hk = hmac512_seed_key();
    for (int j = 0; j < 8; j++) out16[j] = hk.inner.h[j], out16[8 + j] = hk.outer.h[j];
}
extern "C" void emuhd_key_states(const uint8_t* cc32, uint64_t* out16) {
    const HmacKey512 hk = hmac512_key(hd_load_cc(cc32, 0));
    for (int j = 0; j < 8; j++) out16[j] = hk.inner.h[j], out16[8 + j] = hk.outer.h[j];
}
// I = HMAC-SHA512(cc, b0 || ser256(v) || ser32(index)) as its 64 bytes; v32 little-endian
extern "C" void emuhd_bip32_I(const uint8_t* cc32, unsigned b0, const uint8_t* v32, uint32_t index, uint8_t* out64) {
    const Bip32I I = bip32_I(hd_load_cc(cc32, 0), b0, le256(v32), index);
    for (int j = 0; j < 32; j++) out64[j] = (uint8_t)(I.il.w[7 - j / 4] >> (8 * (3 - j % 4)));
    for (int j = 0; j < 32; j++) out64[32 + j] = (uint8_t)(I.ir.w[j / 4] >> (8 * (3 - j % 4)));
}
// the arithmetic behind the hash with ANY I_L (32-byte little-endian values); outputs are written only where the code is 0
extern "C" int emuhd_finish_priv(const uint8_t* il32, const uint8_t* k32, uint8_t* out32) {
    U256 kc = u256_zero();
    const uint8_t e = bip32_finish_priv(le256(il32), le256(k32), kc);
    if (!e) put256(out32, kc);
    return e;
}
extern "C" int emuhd_finish_pub(const uint8_t* il32, const uint8_t* px32, const uint8_t* py32, uint8_t* outx32, uint8_t* outy32) {
    Aff K, C;
    K.x = le256(px32), K.y = le256(py32);
    C.x = C.y = u256_zero();
    const uint8_t e = bip32_finish_pub(gen_table(), le256(il32), K, C);
    if (!e) put256(outx32, C.x), put256(outy32, C.y);
    return e;
}
extern "C" void emuhd_hash160_of_digest(const uint8_t* digest32, uint8_t* out20) {
    const Hash160 h = hash160_of_digest(hd_load_cc(digest32, 0));
    for (int j = 0; j < 20; j++) out20[j] = (uint8_t)(h.w[j / 4] >> (8 * (j % 4)));
}

extern "C" long emuhd_master(const uint8_t* seed, size_t seed_len, uint8_t* sk32, uint8_t* cc32, size_t n, uint8_t* err) {
    long bad = 0;
#pragma omp parallel for schedule(dynamic, 16) reduction(+ : bad)
    for (long long i = 0; i < (long long)n; i++) {
        err[i] = body_bip32_master(seed, (u32)seed_len, sk32, cc32, (size_t)i);
        bad += err[i] != 0;
    }
    return bad;
}
extern "C" long emuhd_ckd_priv(const uint8_t* par_sk32, const uint8_t* par_cc32, size_t n_parents, const uint32_t* index, uint8_t* sk32,
                               uint8_t* cc32, size_t n, uint8_t* err) {
    const Aff* T = gen_table();
    long bad = 0;
#pragma omp parallel for schedule(dynamic, 16) reduction(+ : bad)
    for (long long i = 0; i < (long long)n; i++) {
        err[i] = body_bip32_ckd_priv(T, par_sk32, par_cc32, n_parents == n ? (size_t)i : 0, index, sk32, cc32, (size_t)i);
        bad += err[i] != 0;
    }
    return bad;
}
extern "C" long emuhd_ckd_pub(const uint8_t* par_pkx32, const uint8_t* par_pky32, const uint8_t* par_cc32, size_t n_parents,
                              const uint32_t* index, uint8_t* pkx32, uint8_t* pky32, uint8_t* cc32, size_t n, uint8_t* err) {
    const Aff* T = gen_table();
    long bad = 0;
#pragma omp parallel for schedule(dynamic, 16) reduction(+ : bad)
    for (long long i = 0; i < (long long)n; i++) {
        err[i] = body_bip32_ckd_pub(T, par_pkx32, par_pky32, par_cc32, n_parents == n ? (size_t)i : 0, index, pkx32, pky32, cc32, (size_t)i);
        bad += err[i] != 0;
    }
    return bad;
}
extern "C" long emuhd_key_hash160(unsigned form, const uint8_t* pkx32, const uint8_t* pky32, const uint8_t* err_in, uint8_t* out20, size_t n) {
#pragma omp parallel for schedule(dynamic, 16)
    for (long long i = 0; i < (long long)n; i++) body_key_hash160((int)form, pkx32, pky32, err_in, out20, (size_t)i);
    return 0;
}
extern "C" long emuhd_hash160(const uint8_t* data, const uint64_t* offsets, uint8_t* out20, size_t n) {
    long bad = 0;
#pragma omp parallel for schedule(dynamic, 16) reduction(+ : bad)
    for (long long i = 0; i < (long long)n; i++) bad += body_hash160(data, offsets, out20, (size_t)i) ? 1 : 0;
    return bad;
}

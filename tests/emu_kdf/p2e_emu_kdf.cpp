// CPU harness of the PBKDF2 / BIP-39 layer (test infrastructure only): the bodies of csrc/kdf.hpp run per element, compiled
// with g++ against the library's headers.  The absorber and the fixed-shape compression are reachable on their own.
#include <cstdint>
#include <cstring>

#include "../../plonky2-ecdsa_amd/csrc/kdf.hpp"

using namespace p2e;

namespace {
void put_state(uint8_t* out64, const Sha512State& s) {
    for (int j = 0; j < 64; j++) out64[j] = (uint8_t)(s.h[j / 8] >> (8 * (7 - j % 8)));
}
u64 be64(const uint8_t* p) {
    u64 v = 0;
    for (int k = 0; k < 8; k++) v = (v << 8) | p[k];
    return v;
}
}  // namespace

// SHA-512(first || prefix || data[lo, hi) || extra) as its 64 bytes.  first: nothing (null) or ONE 128-byte block that is
// compressed from the IV before the absorber continues behind it; prefix: prefix_len = 0 or 8 bytes; extra: nothing
// (indexed = 0) or the four big-endian bytes of `index`.
extern "C" int emukdf_absorb(const uint8_t* first, const uint8_t* prefix, unsigned prefix_len, const uint8_t* data, uint64_t lo, uint64_t hi,
                             int indexed, uint32_t index, uint8_t* out64) {
    Sha512State st = sha512_iv();
    u64 done = 0;
    if (first) {
        Sha512Block b;
        for (int j = 0; j < 16; j++) b.w[j] = be64(first + 8 * j);
        st = sha512_compress(st, b);
        done = 128;
    }
    const uint64_t offsets[2] = {lo, hi};
    bool bad;
    const MsgView m = kdf_view(data, offsets, 0, &bad);
    if (bad) return 1;
    const u64 tail = indexed ? kdf_tail_indexed(index) : KDF_TAIL_END;
    if (prefix_len == 8)
        st = sha512_absorb<8>(st, done, be64(prefix), m, tail, indexed ? 4 : 0);
    else if (prefix_len == 0)
        st = sha512_absorb<0>(st, done, 0, m, tail, indexed ? 4 : 0);
    else
        return 2;
    put_state(out64, st);
    return 0;
}
// state: 8 words in and out; digest: the 8 words of the block's first 64 bytes.  `plain`: hd.hpp's compression of the same block
extern "C" void emukdf_compress_digest(uint64_t* state, const uint64_t* digest, int plain) {
    Sha512State s, d;
    for (int j = 0; j < 8; j++) s.h[j] = state[j], d.h[j] = digest[j];
    if (plain) {
        Sha512Block b;
        for (int j = 0; j < 16; j++) b.w[j] = j < 8 ? d.h[j] : 0;
        b.w[8] = 0x8000000000000000ull;
        b.w[15] = 1536;
        s = sha512_compress(s, b);
    } else {
        s = sha512_compress_digest(s, d);
    }
    for (int j = 0; j < 8; j++) state[j] = s.h[j];
}
// inner[8] then outer[8] of the key data[lo, hi) (a longer key than 128 bytes is hashed first)
extern "C" int emukdf_key_states(const uint8_t* data, uint64_t lo, uint64_t hi, uint64_t* out16) {
    const uint64_t offsets[2] = {lo, hi};
    bool bad;
    const MsgView m = kdf_view(data, offsets, 0, &bad);
    if (bad) return 1;
    const HmacKey512 hk = kdf_key_states(kdf_key_block(m));
    for (int j = 0; j < 8; j++) out16[j] = hk.inner.h[j], out16[8 + j] = hk.outer.h[j];
    return 0;
}
// the two calls of include/p2e.h, element by element: bip39 != 0 puts "mnemonic" in front of the salt; salt_offsets may be
// null with n_salts == 0 (the empty salt)
extern "C" long emukdf_pbkdf2(int bip39, const uint8_t* password, const uint64_t* pw_offsets, size_t n_passwords, const uint8_t* salt,
                              const uint64_t* salt_offsets, size_t n_salts, uint32_t iterations, size_t dk_len, uint8_t* dk, size_t count,
                              uint8_t* err) {
    long bad = 0;
#pragma omp parallel for schedule(dynamic, 4) reduction(+ : bad)
    for (long long k = 0; k < (long long)count; k++) {
        const size_t i = (size_t)k, pi = n_passwords == count ? i : 0, si = n_salts == count ? i : 0;
        err[i] = bip39 ? body_pbkdf2_sha512<8>(password, pw_offsets, pi, salt, salt_offsets, si, BIP39_SALT_PREFIX, iterations, (u32)(dk_len / 4), dk, i)
                       : body_pbkdf2_sha512<0>(password, pw_offsets, pi, salt, salt_offsets, si, 0, iterations, (u32)(dk_len / 4), dk, i);
        bad += err[i] != 0;
    }
    return bad;
}

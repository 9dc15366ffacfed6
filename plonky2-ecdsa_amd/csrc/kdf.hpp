// PBKDF2-HMAC-SHA512 for a batch, and BIP-39's seed derivation on top of it (include/p2e.h p2e_pbkdf2_hmac_sha512_batch,
// p2e_bip39_seed_batch).  The reference has no counterpart: nothing there derives keys.  What is computed here is defined by
//   RFC 8018 5.2      PBKDF2, here with one output block: T = U_1 ^ ... ^ U_c, U_1 = PRF(P, S || INT(1)), U_j = PRF(P, U_{j-1});
//   RFC 2104          HMAC: a key longer than the hash's 128-byte block is replaced by its digest;
//   FIPS 180-4        SHA-512, hd.hpp's compression;
//   BIP-39            seed = PBKDF2(P = the sentence, S = "mnemonic" || passphrase, c = 2048, 64 bytes).
// One lane derives one key.  Three parts:
//   cold   the SHA-512 of a password longer than a block and the inner hash of U_1 run hd.hpp's compression from a streaming
//          absorber (sha512_absorb, hash.hpp's sha256_message in 128-byte blocks); the lanes of a wave hold different block
//          counts and the loops run to the lane's own.  Two more compressions make the key states.
//   hot    c - 1 trips of two compressions of ONE shape: the block is a 64-byte digest, the 0x80 byte, zeros and the length
//          1536 (a 128-byte key block and 64 bytes).  sha512_compress_digest is that shape's own body: all 80 rounds are
//          unrolled, so the eight constant words of the block fold into the round constants of the first pass and into the
//          schedule of the second, no round constant is loaded, and the last pass computes no schedule.  The hot loop holds
//          that body ONCE and runs 2 (c - 1) trips, the chaining value picked by the trip's parity (a wave-uniform select):
//          one unrolled compression is 26.6 KB of code (3 891 VALU instructions), and the select is under 1 % of a trip:
//          a second copy would buy nothing and crowd the instruction cache.
//   store  dk_len / 4 words of T.
// Registers.  Two key states, U (which becomes schedule words 0 .. 7) and T are 64 registers that live across the loop; the
// other eight schedule words and the working variables are 32 more.  Every index is a compile-time constant; nothing lives
// in the private segment, no LDS (profiles/kdf_kernel_resources.txt).  Passwords, key states and every U_j stay in registers.
#pragma once
#include "hd.hpp"

namespace p2e {

constexpr u32 PBKDF2_MAX_ITERATIONS = 1u << 20;         // include/p2e.h P2E_PBKDF2_MAX_ITERATIONS
constexpr u64 BIP39_SALT_PREFIX = 0x6d6e656d6f6e6963ull;   // "mnemonic", the eight bytes in front of the passphrase
constexpr u32 BIP39_ITERATIONS = 2048, BIP39_SEED_WORDS = 16;

// ---------------------------------------------------------------------------------------------------------------------
// SHA-512 over a message of the concatenated buffer
// ---------------------------------------------------------------------------------------------------------------------
// Big-endian 32-bit word k of  m || tail  (bytes 4 k .. 4 k + 3; zero behind the tail), read as hash.hpp reads: `carry` is
// aligned word k of m on entry and word k + 1 on return, so the words must be asked for in order.  `tail` is up to eight
// bytes that follow the message's last byte at once, first byte on top.
P2E_HD u32 kdf_stream_word(const MsgView& m, u32& carry, u64 k, u64 tail) {
    const u32 next = m.word(k + 1);
    u32 v = hash_bswap32(hash_join(carry, next, m.sh));
    carry = next;
    const u64 at = 4 * k;
    if (at + 4 > m.len) {                                   // the message ends inside or before this word
        const u32 keep = at < m.len ? (u32)(m.len - at) : 0u;   // 0 .. 3 of its bytes are message bytes
        v = keep ? (v & ~(0xFFFFFFFFu >> (8 * keep))) : 0u;
        const u64 d = at + 3 - m.len;                       // the word starts d - 3 bytes into the tail
        if (d <= 7) v |= (u32)(tail >> (56 - 8 * d));
    }
    return v;
}
constexpr u64 KDF_TAIL_END = 0x8000000000000000ull;                                       // the 0x80 byte alone
P2E_HD u64 kdf_tail_indexed(u32 index) { return ((u64)index << 32) | 0x80000000ull; }    // INT(index), then the 0x80 byte
// SHA-512 continued from `st`, which has absorbed `done` bytes (a multiple of 128), over
//   the PREFIX (0 or 8) bytes of `prefix` || m || `extra` (0 or 4) more bytes,
// the extra ones being the first four of `tail` (kdf_tail_indexed), which also carries the 0x80 byte behind them.
template <int PREFIX>
P2E_HD Sha512State sha512_absorb(Sha512State st, u64 done, u64 prefix, const MsgView& m, u64 tail, u32 extra) {
    static_assert(PREFIX == 0 || PREFIX == 8, "the prefix is nothing or one 64-bit word");
    const u64 total = PREFIX + m.len + extra;
    const u64 nblocks = (total + 16) / 128 + 1;   // the 0x80 byte and the 128-bit length always fit
    u32 carry = m.word(0);
    for (u64 b = 0; b < nblocks; b++) {
        Sha512Block blk;
        P2E_UNROLL
        for (int j = 0; j < 16; j++) {
            if (PREFIX == 8 && j == 0 && b == 0) {
                blk.w[j] = prefix;
            } else {
                const u64 k = 32 * b + 2 * j - PREFIX / 4;
                const u32 hi = kdf_stream_word(m, carry, k, tail);
                const u32 lo = kdf_stream_word(m, carry, k + 1, tail);
                blk.w[j] = ((u64)hi << 32) | lo;
            }
        }
        if (b + 1 == nblocks) blk.w[15] = 8 * (done + total);   // (word 14, the length's upper half, is zero as it stands)
        st = sha512_compress(st, blk);
    }
    return st;
}

// ---------------------------------------------------------------------------------------------------------------------
// HMAC-SHA512 key states of a key of 0 .. 128 bytes
// ---------------------------------------------------------------------------------------------------------------------
// the key's block, zero-padded: a password of at most 128 bytes as it is, a longer one as its digest
P2E_HD Sha512Block kdf_key_block(const MsgView& pw) {
    Sha512Block kb;
    if (pw.len > 128) {
        const Sha512State d = sha512_absorb<0>(sha512_iv(), 0, 0, pw, KDF_TAIL_END, 0);
        P2E_UNROLL
        for (int j = 0; j < 16; j++) kb.w[j] = j < 8 ? d.h[j & 7] : 0ull;
    } else {
        u32 carry = pw.word(0);
        P2E_UNROLL
        for (int j = 0; j < 16; j++) {
            const u32 hi = kdf_stream_word(pw, carry, 2 * j, 0);
            const u32 lo = kdf_stream_word(pw, carry, 2 * j + 1, 0);
            kb.w[j] = ((u64)hi << 32) | lo;
        }
    }
    return kb;
}
// one compression each from the IV; a rolled loop of two trips, so that the rounds stand here once
P2E_HD HmacKey512 kdf_key_states(const Sha512Block& kb) {
    HmacKey512 hk;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
    for (int trip = 0; trip < 2; trip++) {
        const u64 pad = trip ? HMAC512_OPAD : HMAC512_IPAD;
        Sha512Block b;
        P2E_UNROLL
        for (int j = 0; j < 16; j++) b.w[j] = kb.w[j] ^ pad;
        const Sha512State s = sha512_compress(sha512_iv(), b);
        P2E_UNROLL
        for (int j = 0; j < 8; j++) {
            if (trip) hk.outer.h[j] = s.h[j];
            else hk.inner.h[j] = s.h[j];
        }
    }
    return hk;
}

// ---------------------------------------------------------------------------------------------------------------------
// the compression of a digest block: 64 bytes, the 0x80 byte, zeros, and 1536 = 8 (128 + 64) bits
// ---------------------------------------------------------------------------------------------------------------------
constexpr u64 KDF_DIGEST_BLOCK_BITS = 8 * (128 + 64);
// sha512_compress(cv, {d[0 .. 8), 0x80 << 56, 0, 0, 0, 0, 0, 0, 1536}) with every round written out: T is the round's number
#define P2E_KDF_ROUND(a, b, c, d, e, f, g, h, T)                                                                             \
    {                                                                                                                        \
        const u64 t1 = h + (sha512_rotr<14>(e) ^ sha512_rotr<18>(e) ^ sha512_rotr<41>(e)) + (g ^ (e & (f ^ g))) +            \
                       (sha512_k(T) + w[(T) & 15]);                                                                          \
        const u64 t2 = (sha512_rotr<28>(a) ^ sha512_rotr<34>(a) ^ sha512_rotr<39>(a)) + ((a & b) | (c & (a | b)));           \
        d += t1;                                                                                                             \
        h = t1 + t2;                                                                                                         \
    }
P2E_HD Sha512State sha512_compress_digest(const Sha512State& cv, const Sha512State& dg) {
    u64 w[16];
    P2E_UNROLL
    for (int j = 0; j < 16; j++) w[j] = j < 8 ? dg.h[j & 7] : 0ull;
    w[8] = 0x8000000000000000ull;
    w[15] = KDF_DIGEST_BLOCK_BITS;
    u64 a = cv.h[0], b = cv.h[1], c = cv.h[2], d = cv.h[3], e = cv.h[4], f = cv.h[5], g = cv.h[6], h = cv.h[7];
    P2E_UNROLL
    for (int pass = 0; pass < 80; pass += 16) {
        P2E_KDF_ROUND(a, b, c, d, e, f, g, h, pass + 0)
        P2E_KDF_ROUND(h, a, b, c, d, e, f, g, pass + 1)
        P2E_KDF_ROUND(g, h, a, b, c, d, e, f, pass + 2)
        P2E_KDF_ROUND(f, g, h, a, b, c, d, e, pass + 3)
        P2E_KDF_ROUND(e, f, g, h, a, b, c, d, pass + 4)
        P2E_KDF_ROUND(d, e, f, g, h, a, b, c, pass + 5)
        P2E_KDF_ROUND(c, d, e, f, g, h, a, b, pass + 6)
        P2E_KDF_ROUND(b, c, d, e, f, g, h, a, pass + 7)
        P2E_KDF_ROUND(a, b, c, d, e, f, g, h, pass + 8)
        P2E_KDF_ROUND(h, a, b, c, d, e, f, g, pass + 9)
        P2E_KDF_ROUND(g, h, a, b, c, d, e, f, pass + 10)
        P2E_KDF_ROUND(f, g, h, a, b, c, d, e, pass + 11)
        P2E_KDF_ROUND(e, f, g, h, a, b, c, d, pass + 12)
        P2E_KDF_ROUND(d, e, f, g, h, a, b, c, pass + 13)
        P2E_KDF_ROUND(c, d, e, f, g, h, a, b, pass + 14)
        P2E_KDF_ROUND(b, c, d, e, f, g, h, a, pass + 15)
        if (pass < 64) {   // the next sixteen schedule words, in place and in order (hd.hpp); constants fold in the first pass
            P2E_UNROLL
            for (int j = 0; j < 16; j++) {
                const u64 w15 = w[(j + 1) & 15], w2 = w[(j + 14) & 15];
                w[j] += (sha512_rotr<1>(w15) ^ sha512_rotr<8>(w15) ^ (w15 >> 7)) + w[(j + 9) & 15] +
                        (sha512_rotr<19>(w2) ^ sha512_rotr<61>(w2) ^ (w2 >> 6));
            }
        }
    }
    Sha512State r;
    r.h[0] = cv.h[0] + a, r.h[1] = cv.h[1] + b, r.h[2] = cv.h[2] + c, r.h[3] = cv.h[3] + d;
    r.h[4] = cv.h[4] + e, r.h[5] = cv.h[5] + f, r.h[6] = cv.h[6] + g, r.h[7] = cv.h[7] + h;
    return r;
}
#undef P2E_KDF_ROUND

// ---------------------------------------------------------------------------------------------------------------------
// PBKDF2-HMAC-SHA512, one output block
// ---------------------------------------------------------------------------------------------------------------------
// T = U_1 ^ ... ^ U_c under password `pw` and salt  PREFIX bytes of `prefix` || `salt`;  c = iterations >= 1
template <int PREFIX>
P2E_HD Sha512State pbkdf2_sha512_block(const MsgView& pw, u64 prefix, const MsgView& salt, u32 iterations) {
    const HmacKey512 hk = kdf_key_states(kdf_key_block(pw));
    // U_1: the inner hash continues behind the ipad block over the salt and INT(1); its digest is the outer hash's one block
    Sha512State u = sha512_absorb<PREFIX>(hk.inner, 128, prefix, salt, kdf_tail_indexed(1), 4);
    u = sha512_compress(hk.outer, Sha512Block{{u.h[0], u.h[1], u.h[2], u.h[3], u.h[4], u.h[5], u.h[6], u.h[7], 0x8000000000000000ull, 0, 0, 0, 0,
                                               0, 0, KDF_DIGEST_BLOCK_BITS}});
    Sha512State t = u;
    // U_2 .. U_c: trip 2 j is the inner hash of U_{j + 2}, trip 2 j + 1 the outer one.  The trip count is wave-uniform.
    const u32 trips = 2 * (iterations - 1);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
    for (u32 trip = 0; trip < trips; trip++) {
        const bool outer = (trip & 1u) != 0;
        Sha512State cv;
        P2E_UNROLL
        for (int j = 0; j < 8; j++) cv.h[j] = outer ? hk.outer.h[j] : hk.inner.h[j];
        u = sha512_compress_digest(cv, u);
        if (outer) {
            P2E_UNROLL
            for (int j = 0; j < 8; j++) t.h[j] ^= u.h[j];
        }
    }
    return t;
}

// element i of a concatenated buffer (hash.hpp's msg_view); *bad: offsets reversed or a length of 2^32 or more
P2E_HD MsgView kdf_view(const uint8_t* data, const uint64_t* offsets, size_t i, bool* bad) {
    bool reversed;
    const MsgView m = msg_view(data, offsets, i, &reversed);
    *bad = reversed || m.len >= ((u64)1 << 32);
    return m;
}
P2E_HD MsgView kdf_empty_view() {
    MsgView m;
    m.p = nullptr, m.sh = 0, m.len = 0, m.end = 0;
    return m;
}
// Element i: password pi, salt si (0 where one serves the batch); salt_offsets == nullptr: the empty salt (BIP-39's absent
// passphrase).  dk_words = dk_len / 4 in 1 .. 16.  A flagged element stores zeros and runs no iteration.
template <int PREFIX>
P2E_HD uint8_t body_pbkdf2_sha512(const uint8_t* password, const uint64_t* pw_offsets, size_t pi, const uint8_t* salt,
                                  const uint64_t* salt_offsets, size_t si, u64 prefix, u32 iterations, u32 dk_words, uint8_t* dk, size_t i) {
    bool bad_pw, bad_salt = false;
    const MsgView pw = kdf_view(password, pw_offsets, pi, &bad_pw);
    const MsgView sv = salt_offsets ? kdf_view(salt, salt_offsets, si, &bad_salt) : kdf_empty_view();
    const bool bad = bad_pw || bad_salt;
    Sha512State t;
    P2E_UNROLL
    for (int j = 0; j < 8; j++) t.h[j] = 0;
    if (!bad) t = pbkdf2_sha512_block<PREFIX>(pw, prefix, sv, iterations);
    u32* q = reinterpret_cast<u32*>(dk + 4 * (size_t)dk_words * i);
    P2E_UNROLL
    for (int j = 0; j < 16; j++)
        if ((u32)j < dk_words) q[j] = hash_bswap32((j & 1) ? (u32)t.h[j / 2] : (u32)(t.h[j / 2] >> 32));
    return bad ? WIRE_BAD_LENGTH : WIRE_OK;
}

#if defined(__HIPCC__)
// thread g owns element g; pw_bcast / salt_bcast: every element uses password / salt 0.  PREFIX = 8: BIP-39's "mnemonic"
template <int PREFIX>
__global__ __launch_bounds__(256) void k_pbkdf2_sha512(const uint8_t* password, const uint64_t* pw_offsets, int pw_bcast, const uint8_t* salt,
                                                       const uint64_t* salt_offsets, int salt_bcast, u32 iterations, u32 dk_words,
                                                       uint8_t* dk, size_t count, uint8_t* err, unsigned long long* counter) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    uint8_t e = 0;
    if (i < count) {
        e = body_pbkdf2_sha512<PREFIX>(password, pw_offsets, pw_bcast ? 0 : i, salt, salt_offsets, salt_bcast ? 0 : i, BIP39_SALT_PREFIX,
                                       iterations, dk_words, dk, i);
        err[i] = e;
    }
    sign_count_err(e, counter);
}
#endif

}  // namespace p2e

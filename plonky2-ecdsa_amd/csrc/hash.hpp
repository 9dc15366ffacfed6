// The two hashes at the ends of the signing pipeline, one lane per message, and what is built from them:
//   SHA-256 (FIPS 180-4) and Keccak-256 (Keccak-f[1600], rate 136, the legacy 0x01 padding Ethereum uses -- not SHA3-256)
//     over messages of any length at any byte offset of one concatenated buffer (message i = data[offsets[i], offsets[i+1]));
//   HMAC-SHA256 in the three shapes RFC 6979 needs (32-byte key; 32-, 33- and 97-byte messages);
//   the RFC 6979 nonce generator for a 256-bit group order and a 256-bit hash (rfc6979_nonce);
//   the Ethereum address of a public key (eth_address).
// The nearest reference counterpart is sign_message (curve/ecdsa.rs:25-40), which draws its nonce with rand() (:29-32) and
// takes the message as a field element: the reference neither hashes nor derives nonces.
//
// Registers.  Every index of the SHA-256 schedule (16 words), of the Keccak state (25 lanes as 50 words) and of the rho/pi
// permutation is a compile-time constant: the 64 SHA rounds are unrolled, the Keccak round body is unrolled (rho/pi written
// out lane by lane) and only the 24-round loop stays rolled -- its round constant is a table lookup by a wave-uniform index,
// its body is 2 KB of code, 24 copies would not fit the instruction cache.  Nothing here is addressed at run time, so nothing
// lives in the private segment.  A 64-bit rotation is written on the two 32-bit halves, one funnel shift
// (v_alignbit_b32) each; a rotation by 32 or more swaps the halves first, for free.
// The SHA-256 compression is the one function that is NOT inlined on the device (sha256_compress_call: state and block
// travel in 24 VGPRs, as f29_mul_call_regs's operands do): the nonce generator runs it at 18 places.
//
// Absorption.  A lane reads its message as ALIGNED 32-bit words and joins neighbours by the start address's byte
// misalignment (one funnel shift per word); the word that straddles a block boundary is carried over, not read twice.
// A word is read only if it holds at least one byte of the lane's own message (MsgView::word) -- nothing before
// data + offsets[i] rounded down to 4, nothing at or after data + offsets[i + 1] rounded up to 4, nothing at all for an
// empty message.  Bytes of such a word that lie outside the message are masked before use.  The lanes of a wave hold
// different block counts: the block loop runs to the lane's own count.
#pragma once
#include <stddef.h>

#include "fe.hpp"

namespace p2e {

constexpr int HASH_SHA256 = 0, HASH_SHA256D = 1, HASH_KECCAK256 = 2;   // include/p2e.h P2E_HASH_*
constexpr unsigned DIGEST_BYTES = 0, DIGEST_SCALAR = 1;                // include/p2e.h P2E_DIGEST_*

P2E_HD u32 hash_bswap32(u32 v) { return __builtin_bswap32(v); }
// bits [sh, sh + 32) of hi:lo, sh = 0, 8, 16 or 24: four consecutive bytes out of two aligned words
P2E_HD u32 hash_join(u32 lo, u32 hi, u32 sh) { return (u32)((((u64)hi << 32) | lo) >> sh); }

// ---------------------------------------------------------------------------------------------------------------------
// one message of the concatenated buffer, as aligned words
// ---------------------------------------------------------------------------------------------------------------------
struct MsgView {
    const u32* p;    // the aligned word that holds the first byte
    u32 sh;          // 8 * (address of the first byte mod 4)
    u64 len;
    uintptr_t end;   // address one past the last byte; 0 for an empty message (no word may be read)
    // aligned word k counted from p, or 0 where the word holds no byte of this message
    P2E_HD u32 word(u64 k) const {
        const u32* a = p + k;
        return (uintptr_t)a < end ? *a : 0u;
    }
};
// offsets[i + 1] < offsets[i]: the empty message, *bad set
P2E_HD MsgView msg_view(const uint8_t* data, const uint64_t* offsets, size_t i, bool* bad) {
    const u64 lo = offsets[i], hi = offsets[i + 1];
    *bad = hi < lo;
    MsgView m;
    const uintptr_t a = (uintptr_t)(data + lo);
    m.len = hi < lo ? 0 : hi - lo;
    m.p = reinterpret_cast<const u32*>(a & ~(uintptr_t)3);
    m.sh = 8u * (u32)(a & 3u);
    m.end = m.len ? a + m.len : 0;
    return m;
}

// ---------------------------------------------------------------------------------------------------------------------
// SHA-256
// ---------------------------------------------------------------------------------------------------------------------
struct Sha256State {
    u32 h[8];
};
struct Sha256Block {
    u32 w[16];   // the block's sixteen big-endian words
};
P2E_HD u32 sha_rotr(u32 x, int n) { return (x >> n) | (x << (32 - n)); }
P2E_HD u32 sha256_k(int t) {
    constexpr u32 K[64] = {
        0x428a2f98u, 0x71374491u, 0xb5c0fbcfu, 0xe9b5dba5u, 0x3956c25bu, 0x59f111f1u, 0x923f82a4u, 0xab1c5ed5u, 0xd807aa98u, 0x12835b01u,
        0x243185beu, 0x550c7dc3u, 0x72be5d74u, 0x80deb1feu, 0x9bdc06a7u, 0xc19bf174u, 0xe49b69c1u, 0xefbe4786u, 0x0fc19dc6u, 0x240ca1ccu,
        0x2de92c6fu, 0x4a7484aau, 0x5cb0a9dcu, 0x76f988dau, 0x983e5152u, 0xa831c66du, 0xb00327c8u, 0xbf597fc7u, 0xc6e00bf3u, 0xd5a79147u,
        0x06ca6351u, 0x14292967u, 0x27b70a85u, 0x2e1b2138u, 0x4d2c6dfcu, 0x53380d13u, 0x650a7354u, 0x766a0abbu, 0x81c2c92eu, 0x92722c85u,
        0xa2bfe8a1u, 0xa81a664bu, 0xc24b8b70u, 0xc76c51a3u, 0xd192e819u, 0xd6990624u, 0xf40e3585u, 0x106aa070u, 0x19a4c116u, 0x1e376c08u,
        0x2748774cu, 0x34b0bcb5u, 0x391c0cb3u, 0x4ed8aa4au, 0x5b9cca4fu, 0x682e6ff3u, 0x748f82eeu, 0x78a5636fu, 0x84c87814u, 0x8cc70208u,
        0x90befffau, 0xa4506cebu, 0xbef9a3f7u, 0xc67178f2u};
    return K[t];
}
P2E_HD Sha256State sha256_iv() {
    Sha256State s;
    s.h[0] = 0x6a09e667u, s.h[1] = 0xbb67ae85u, s.h[2] = 0x3c6ef372u, s.h[3] = 0xa54ff53au;
    s.h[4] = 0x510e527fu, s.h[5] = 0x9b05688cu, s.h[6] = 0x1f83d9abu, s.h[7] = 0x5be0cd19u;
    return s;
}
// One round with the working variables rotated BY NAME: the caller permutes the arguments, nothing moves.
// w[t & 15] is replaced by the schedule word of round t + 16 once it has been used.
#define P2E_SHA_ROUND(a, b, c, d, e, f, g, h, t)                                                                   \
    {                                                                                                              \
        if ((t) >= 16) {                                                                                           \
            const u32 w15 = w[((t) + 1) & 15], w2 = w[((t) + 14) & 15];                                             \
            w[(t) & 15] += (sha_rotr(w15, 7) ^ sha_rotr(w15, 18) ^ (w15 >> 3)) + w[((t) + 9) & 15] +               \
                           (sha_rotr(w2, 17) ^ sha_rotr(w2, 19) ^ (w2 >> 10));                                      \
        }                                                                                                          \
        const u32 t1 = h + (sha_rotr(e, 6) ^ sha_rotr(e, 11) ^ sha_rotr(e, 25)) + (g ^ (e & (f ^ g))) + sha256_k(t) + w[(t) & 15]; \
        const u32 t2 = (sha_rotr(a, 2) ^ sha_rotr(a, 13) ^ sha_rotr(a, 22)) + ((a & b) | (c & (a | b)));            \
        d += t1;                                                                                                   \
        h = t1 + t2;                                                                                               \
    }
P2E_HD Sha256State sha256_compress(const Sha256State& s, const Sha256Block& blk) {
    u32 w[16];
    P2E_UNROLL
    for (int j = 0; j < 16; j++) w[j] = blk.w[j];
    u32 a = s.h[0], b = s.h[1], c = s.h[2], d = s.h[3], e = s.h[4], f = s.h[5], g = s.h[6], h = s.h[7];
    P2E_UNROLL
    for (int t = 0; t < 64; t += 8) {
        P2E_SHA_ROUND(a, b, c, d, e, f, g, h, t + 0)
        P2E_SHA_ROUND(h, a, b, c, d, e, f, g, t + 1)
        P2E_SHA_ROUND(g, h, a, b, c, d, e, f, t + 2)
        P2E_SHA_ROUND(f, g, h, a, b, c, d, e, t + 3)
        P2E_SHA_ROUND(e, f, g, h, a, b, c, d, t + 4)
        P2E_SHA_ROUND(d, e, f, g, h, a, b, c, t + 5)
        P2E_SHA_ROUND(c, d, e, f, g, h, a, b, t + 6)
        P2E_SHA_ROUND(b, c, d, e, f, g, h, a, t + 7)
    }
    Sha256State r;
    r.h[0] = s.h[0] + a, r.h[1] = s.h[1] + b, r.h[2] = s.h[2] + c, r.h[3] = s.h[3] + d;
    r.h[4] = s.h[4] + e, r.h[5] = s.h[5] + f, r.h[6] = s.h[6] + g, r.h[7] = s.h[7] + h;
    return r;
}
#undef P2E_SHA_ROUND
// The call form.  Its 24 words travel as 24 scalar arguments: aggregates are passed in registers only while a call's
// arguments need no more than 16 in all (f29_mul_call_regs, fe29.hpp, has the same shape for the same reason); a struct
// beyond that goes through the private segment.  (A template only so that every translation unit may hold the definition.)
template <int = 0>
P2E_HD_NOINLINE Sha256State sha256_compress_call_regs(u32 h0, u32 h1, u32 h2, u32 h3, u32 h4, u32 h5, u32 h6, u32 h7, u32 w0, u32 w1, u32 w2,
                                                      u32 w3, u32 w4, u32 w5, u32 w6, u32 w7, u32 w8, u32 w9, u32 w10, u32 w11, u32 w12,
                                                      u32 w13, u32 w14, u32 w15) {
    Sha256State s;
    Sha256Block b;
    s.h[0] = h0, s.h[1] = h1, s.h[2] = h2, s.h[3] = h3, s.h[4] = h4, s.h[5] = h5, s.h[6] = h6, s.h[7] = h7;
    b.w[0] = w0, b.w[1] = w1, b.w[2] = w2, b.w[3] = w3, b.w[4] = w4, b.w[5] = w5, b.w[6] = w6, b.w[7] = w7;
    b.w[8] = w8, b.w[9] = w9, b.w[10] = w10, b.w[11] = w11, b.w[12] = w12, b.w[13] = w13, b.w[14] = w14, b.w[15] = w15;
    return sha256_compress(s, b);
}
P2E_HD Sha256State sha256_compress_call(const Sha256State& s, const Sha256Block& b) {
    return sha256_compress_call_regs(s.h[0], s.h[1], s.h[2], s.h[3], s.h[4], s.h[5], s.h[6], s.h[7], b.w[0], b.w[1], b.w[2], b.w[3], b.w[4],
                                     b.w[5], b.w[6], b.w[7], b.w[8], b.w[9], b.w[10], b.w[11], b.w[12], b.w[13], b.w[14], b.w[15]);
}
// a block that ends a message of `total_bits`: words [0, used) are the caller's, the 0x80 byte is already in them
P2E_HD void sha256_finish_block(Sha256Block& b, int used, u32 total_bits) {
    P2E_UNROLL
    for (int j = 0; j < 16; j++)
        if (j >= used) b.w[j] = 0;
    b.w[15] = total_bits;
}

// SHA-256 of one message of the buffer
P2E_HD Sha256State sha256_message(const MsgView& m) {
    Sha256State st = sha256_iv();
    const u64 nblocks = (m.len + 8) / 64 + 1;   // the 0x80 byte and the 64-bit length always fit
    u32 carry = m.word(0);
    for (u64 b = 0; b < nblocks; b++) {
        Sha256Block blk;
        const u64 pos = 64 * b;
        P2E_UNROLL
        for (int j = 0; j < 16; j++) {
            const u32 next = m.word(16 * b + j + 1);
            u32 v = hash_bswap32(hash_join(carry, next, m.sh));   // message bytes pos + 4 j .. + 3, first byte on top
            carry = next;
            const u64 at = pos + 4 * j;
            if (at + 4 > m.len) {                                  // the message ends inside or before this word
                const u32 keep = at < m.len ? (u32)(m.len - at) : 0u;   // 0 .. 3 of its bytes are message bytes
                const u32 cut = 0xFFFFFFFFu >> (8 * keep);
                v = at <= m.len ? ((v & ~cut) | (0x80000000u >> (8 * keep))) : 0u;
            }
            blk.w[j] = v;
        }
        if (b + 1 == nblocks) {
            blk.w[14] = (u32)(m.len >> 29);
            blk.w[15] = (u32)(m.len << 3);
        }
        st = sha256_compress_call(st, blk);
    }
    return st;
}
// SHA-256 of a 32-byte digest (the second pass of SHA-256d)
P2E_HD Sha256State sha256_of_digest(const Sha256State& d) {
    Sha256Block b;
    P2E_UNROLL
    for (int j = 0; j < 8; j++) b.w[j] = d.h[j];
    b.w[8] = 0x80000000u;
    sha256_finish_block(b, 9, 256);
    return sha256_compress_call(sha256_iv(), b);
}
// the digest as 8 words to store little-endian at out32 + 32 i.  BYTES: the digest's bytes in order;  SCALAR: the
// digest read as a big-endian integer, i.e. the same bytes reversed -- the msg32 of every other entry point
P2E_HD U256 sha256_output(const Sha256State& s, unsigned form) {
    U256 r;
    P2E_UNROLL
    for (int j = 0; j < 8; j++) r.w[j] = form == DIGEST_SCALAR ? s.h[7 - j] : hash_bswap32(s.h[j]);
    return r;
}

// ---------------------------------------------------------------------------------------------------------------------
// Keccak-f[1600] and Keccak-256
// ---------------------------------------------------------------------------------------------------------------------
struct Keccak {
    u32 lo[25], hi[25];   // lane x + 5 y
};
P2E_HD u64 keccak_rc(int round) {
    static constexpr u64 RC[24] = {0x0000000000000001ull, 0x0000000000008082ull, 0x800000000000808aull, 0x8000000080008000ull,
                                   0x000000000000808bull, 0x0000000080000001ull, 0x8000000080008081ull, 0x8000000000008009ull,
                                   0x000000000000008aull, 0x0000000000000088ull, 0x0000000080008009ull, 0x000000008000000aull,
                                   0x000000008000808bull, 0x800000000000008bull, 0x8000000000008089ull, 0x8000000000008003ull,
                                   0x8000000000008002ull, 0x8000000000000080ull, 0x000000000000800aull, 0x800000008000000aull,
                                   0x8000000080008081ull, 0x8000000000008080ull, 0x0000000080000001ull, 0x8000000080008008ull};
    return RC[round];
}
// rotate the lane (lo, hi) left by the constant R into (rl, rh): two funnel shifts, the halves swapped first for R >= 32
template <int R>
P2E_HD void keccak_rotl(u32 lo, u32 hi, u32& rl, u32& rh) {
    const u32 a = R >= 32 ? hi : lo, b = R >= 32 ? lo : hi;   // the lane rotated by 32 (R >= 32) or as it is
    constexpr int S = R & 31;
    if (S == 0) {
        rl = a, rh = b;
    } else {
        rl = (a << S) | (b >> ((32 - S) & 31));
        rh = (b << S) | (a >> ((32 - S) & 31));
    }
}
P2E_HD void keccak_f1600(Keccak& s) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
    for (int round = 0; round < 24; round++) {
        // theta
        u32 cl[5], ch[5];
        P2E_UNROLL
        for (int x = 0; x < 5; x++) {
            cl[x] = s.lo[x] ^ s.lo[x + 5] ^ s.lo[x + 10] ^ s.lo[x + 15] ^ s.lo[x + 20];
            ch[x] = s.hi[x] ^ s.hi[x + 5] ^ s.hi[x + 10] ^ s.hi[x + 15] ^ s.hi[x + 20];
        }
        P2E_UNROLL
        for (int x = 0; x < 5; x++) {
            u32 rl, rh;
            keccak_rotl<1>(cl[(x + 1) % 5], ch[(x + 1) % 5], rl, rh);
            const u32 dl = cl[(x + 4) % 5] ^ rl, dh = ch[(x + 4) % 5] ^ rh;
            P2E_UNROLL
            for (int y = 0; y < 25; y += 5) s.lo[x + y] ^= dl, s.hi[x + y] ^= dh;
        }
        // rho and pi: the one cycle through the 24 lanes other than lane 0, each lane rotated on its way
        u32 tl = s.lo[1], th = s.hi[1];
#define P2E_KECCAK_RP(J, R)                        \
    {                                              \
        const u32 nl = s.lo[J], nh = s.hi[J];      \
        keccak_rotl<R>(tl, th, s.lo[J], s.hi[J]);  \
        tl = nl, th = nh;                          \
    }
        P2E_KECCAK_RP(10, 1) P2E_KECCAK_RP(7, 3) P2E_KECCAK_RP(11, 6) P2E_KECCAK_RP(17, 10) P2E_KECCAK_RP(18, 15) P2E_KECCAK_RP(3, 21)
        P2E_KECCAK_RP(5, 28) P2E_KECCAK_RP(16, 36) P2E_KECCAK_RP(8, 45) P2E_KECCAK_RP(21, 55) P2E_KECCAK_RP(24, 2) P2E_KECCAK_RP(4, 14)
        P2E_KECCAK_RP(15, 27) P2E_KECCAK_RP(23, 41) P2E_KECCAK_RP(19, 56) P2E_KECCAK_RP(13, 8) P2E_KECCAK_RP(12, 25) P2E_KECCAK_RP(2, 43)
        P2E_KECCAK_RP(20, 62) P2E_KECCAK_RP(14, 18) P2E_KECCAK_RP(22, 39) P2E_KECCAK_RP(9, 61) P2E_KECCAK_RP(6, 20) P2E_KECCAK_RP(1, 44)
#undef P2E_KECCAK_RP
        // chi
        P2E_UNROLL
        for (int y = 0; y < 25; y += 5) {
            u32 bl[5], bh[5];
            P2E_UNROLL
            for (int x = 0; x < 5; x++) bl[x] = s.lo[y + x], bh[x] = s.hi[y + x];
            P2E_UNROLL
            for (int x = 0; x < 5; x++) {
                s.lo[y + x] = bl[x] ^ (~bl[(x + 1) % 5] & bl[(x + 2) % 5]);
                s.hi[y + x] = bh[x] ^ (~bh[(x + 1) % 5] & bh[(x + 2) % 5]);
            }
        }
        // iota
        const u64 rc = keccak_rc(round);
        s.lo[0] ^= (u32)rc;
        s.hi[0] ^= (u32)(rc >> 32);
    }
}
P2E_HD Keccak keccak_zero() {
    Keccak s;
    P2E_UNROLL
    for (int j = 0; j < 25; j++) s.lo[j] = s.hi[j] = 0;
    return s;
}
constexpr int KECCAK_RATE_WORDS = 34;   // 136 bytes

// Keccak-256 of one message of the buffer: the first 8 state words are the digest's bytes in order
P2E_HD Keccak keccak256_message(const MsgView& m) {
    Keccak st = keccak_zero();
    const u64 nblocks = m.len / 136 + 1;   // the padding always adds at least one byte
    u32 carry = m.word(0);
    for (u64 b = 0; b < nblocks; b++) {
        const u64 pos = 136 * b;
        P2E_UNROLL
        for (int j = 0; j < KECCAK_RATE_WORDS; j++) {
            const u32 next = m.word(KECCAK_RATE_WORDS * b + j + 1);
            u32 v = hash_join(carry, next, m.sh);   // message bytes pos + 4 j .. + 3, first byte lowest
            carry = next;
            const u64 at = pos + 4 * j;
            if (at + 4 > m.len) {
                const u32 keep = at < m.len ? (u32)(m.len - at) : 0u;
                v = at <= m.len ? ((v & ~(0xFFFFFFFFu << (8 * keep))) | (1u << (8 * keep))) : 0u;   // the 0x01 of pad10*1
            }
            if (j == KECCAK_RATE_WORDS - 1 && b + 1 == nblocks) v ^= 0x80000000u;                  // and its final bit
            if (j & 1)
                st.hi[j >> 1] ^= v;
            else
                st.lo[j >> 1] ^= v;
        }
        keccak_f1600(st);
    }
    return st;
}
P2E_HD U256 keccak256_output(const Keccak& s, unsigned form) {
    u32 d[8];
    P2E_UNROLL
    for (int j = 0; j < 4; j++) d[2 * j] = s.lo[j], d[2 * j + 1] = s.hi[j];
    U256 r;
    P2E_UNROLL
    for (int j = 0; j < 8; j++) r.w[j] = form == DIGEST_SCALAR ? hash_bswap32(d[7 - j]) : d[j];
    return r;
}

// The Ethereum address of the public key (x, y), both this library's little-endian values:
// keccak256(BE32(x) || BE32(y))[12..32] as five words to store in order.  One permutation: 64 bytes are under the rate.
struct EthAddress {
    u32 w[5];
};
P2E_HD EthAddress eth_address(const U256& x, const U256& y) {
    Keccak st = keccak_zero();
    P2E_UNROLL
    for (int j = 0; j < 8; j++) {   // absorbed word j = the big-endian value's bytes 4 j .. 4 j + 3, first byte lowest
        const u32 vx = hash_bswap32(x.w[7 - j]), vy = hash_bswap32(y.w[7 - j]);
        if (j & 1)
            st.hi[j >> 1] = vx, st.hi[4 + (j >> 1)] = vy;
        else
            st.lo[j >> 1] = vx, st.lo[4 + (j >> 1)] = vy;
    }
    st.lo[8] = 0x01u;            // byte 64
    st.hi[16] = 0x80000000u;     // byte 135
    keccak_f1600(st);
    EthAddress a;
    a.w[0] = st.hi[1], a.w[1] = st.lo[2], a.w[2] = st.hi[2], a.w[3] = st.lo[3], a.w[4] = st.hi[3];   // digest bytes 12 .. 31
    return a;
}

// ---------------------------------------------------------------------------------------------------------------------
// HMAC-SHA256 in RFC 6979's shapes.  Keys, chaining values and digests are 8 big-endian words (word 0 = bytes 0 .. 3).
// ---------------------------------------------------------------------------------------------------------------------
struct Words8 {
    u32 w[8];
};
struct HmacKey {
    Sha256State inner, outer;   // the states after the ipad and the opad block: computed once per key
};
P2E_HD HmacKey hmac_key(const Words8& k) {
    Sha256Block bi, bo;
    P2E_UNROLL
    for (int j = 0; j < 16; j++) {
        const u32 kw = j < 8 ? k.w[j] : 0u;
        bi.w[j] = kw ^ 0x36363636u;
        bo.w[j] = kw ^ 0x5c5c5c5cu;
    }
    HmacKey hk;
    hk.inner = sha256_compress_call(sha256_iv(), bi);
    hk.outer = sha256_compress_call(sha256_iv(), bo);
    return hk;
}
// the outer hash over the inner digest (64 + 32 bytes in all)
P2E_HD Words8 hmac_outer(const HmacKey& hk, const Sha256State& inner) {
    Sha256Block b;
    P2E_UNROLL
    for (int j = 0; j < 8; j++) b.w[j] = inner.h[j];
    b.w[8] = 0x80000000u;
    sha256_finish_block(b, 9, 8 * (64 + 32));
    const Sha256State o = sha256_compress_call(hk.outer, b);
    Words8 r;
    P2E_UNROLL
    for (int j = 0; j < 8; j++) r.w[j] = o.h[j];
    return r;
}
// HMAC_K(V) and HMAC_K(V || tag): 32 or 33 bytes, one inner block
P2E_HD Words8 hmac_v(const HmacKey& hk, const Words8& v, bool with_tag, u32 tag) {
    Sha256Block b;
    P2E_UNROLL
    for (int j = 0; j < 8; j++) b.w[j] = v.w[j];
    b.w[8] = with_tag ? ((tag << 24) | 0x00800000u) : 0x80000000u;
    sha256_finish_block(b, 9, with_tag ? 8 * (64 + 33) : 8 * (64 + 32));
    return hmac_outer(hk, sha256_compress_call(hk.inner, b));
}
// HMAC_K(V || tag || t): 97 bytes, t = 64 bytes (int2octets(x) || bits2octets(h1)); everything behind V sits one byte off
// the word grid, so stream word j = the last byte of t[j - 1] and the first three of t[j]
P2E_HD Words8 hmac_v_tag_xh(const HmacKey& hk, const Words8& v, u32 tag, const u32 (&t)[16]) {
    Sha256Block b;
    P2E_UNROLL
    for (int j = 0; j < 8; j++) b.w[j] = v.w[j];
    b.w[8] = (tag << 24) | (t[0] >> 8);
    P2E_UNROLL
    for (int j = 1; j < 8; j++) b.w[8 + j] = (t[j - 1] << 24) | (t[j] >> 8);
    const Sha256State mid = sha256_compress_call(hk.inner, b);
    P2E_UNROLL
    for (int j = 8; j < 16; j++) b.w[j - 8] = (t[j - 1] << 24) | (t[j] >> 8);
    b.w[8] = (t[15] << 24) | 0x00800000u;
    sha256_finish_block(b, 9, 8 * (64 + 97));
    return hmac_outer(hk, sha256_compress_call(mid, b));
}

// ---------------------------------------------------------------------------------------------------------------------
// RFC 6979 section 3.2 with qlen = hlen = 256 (bits2int is the identity): the nonce for the key x (given reduced, x < q)
// and the message hash z (any 256-bit value), q the group order as a RUN-TIME value with 2^255 < q < 2^256.
//   h = int2octets(z mod q)  (one conditional subtraction: 2 q > 2^256);  V = 01 x 32;  K = 00 x 32
//   K = HMAC_K(V || 00 || x || h), V = HMAC_K(V);   K = HMAC_K(V || 01 || x || h), V = HMAC_K(V)
//   loop: V = HMAC_K(V), k = int(V); accept iff 1 <= k < q; else K = HMAC_K(V || 00), V = HMAC_K(V)
// The loop is per lane.  *rejected = the number of candidates refused (0 on all but about 2^-32 / 2^-128 of the inputs of
// the real curves: tests reach the loop through a synthetic order).  3.2's further retry for r = 0 or s = 0 belongs to the
// signer and is not done (sign.hpp: such a signature is returned as computed).
// ---------------------------------------------------------------------------------------------------------------------
P2E_HD U256 rfc6979_nonce(const U256& q, const U256& x, const U256& z, u32* rejected) {
    U256 h;
    if (sub_n<8>(h.w, z.w, q.w)) h = z;   // borrow: z < q
    u32 t[16];
    P2E_UNROLL
    for (int j = 0; j < 8; j++) t[j] = x.w[7 - j], t[8 + j] = h.w[7 - j];
    Words8 V, K;
    P2E_UNROLL
    for (int j = 0; j < 8; j++) V.w[j] = 0x01010101u, K.w[j] = 0;
    HmacKey hk = hmac_key(K);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
    for (u32 tag = 0; tag < 2; tag++) {
        K = hmac_v_tag_xh(hk, V, tag, t);
        hk = hmac_key(K);
        V = hmac_v(hk, V, false, 0);
    }
    u32 refused = 0;
    U256 k;
    for (;;) {
        V = hmac_v(hk, V, false, 0);
        P2E_UNROLL
        for (int j = 0; j < 8; j++) k.w[j] = V.w[7 - j];
        U256 d;
        if (!u256_is_zero(k) && sub_n<8>(d.w, k.w, q.w)) break;   // 1 <= k < q
        refused++;
        K = hmac_v(hk, V, true, 0);
        hk = hmac_key(K);
        V = hmac_v(hk, V, false, 0);
    }
    if (rejected) *rejected = refused;
    return k;
}
P2E_HD U256 rfc6979_nonce(const U256& q, const U256& x, const U256& z) { return rfc6979_nonce(q, x, z, nullptr); }

template <class MOD>
P2E_HD U256 hash_modulus() {
    U256 q;
    P2E_UNROLL
    for (int j = 0; j < 8; j++) q.w[j] = MOD::m(j);
    return q;
}
// 32-byte little-endian values at base + 32 i (4-byte aligned, as every packed array of this library)
P2E_HD U256 hash_load_packed(const uint8_t* base, size_t i) {
    const u32* p = reinterpret_cast<const u32*>(base + 32 * i);
    U256 r;
    P2E_UNROLL
    for (int k = 0; k < 8; k++) r.w[k] = p[k];
    return r;
}
P2E_HD void hash_store_packed(uint8_t* base, size_t i, const U256& v) {
    u32* p = reinterpret_cast<u32*>(base + 32 * i);
    P2E_UNROLL
    for (int k = 0; k < 8; k++) p[k] = v.w[k];
}

// ---------------------------------------------------------------------------------------------------------------------
// bodies of the four kernels: element i
// ---------------------------------------------------------------------------------------------------------------------
// returns true where offsets[i + 1] < offsets[i] (hashed as the empty message)
template <int ALG>
P2E_HD bool body_hash(const uint8_t* data, const uint64_t* offsets, uint8_t* out32, size_t i, unsigned form) {
    bool bad;
    const MsgView m = msg_view(data, offsets, i, &bad);
    U256 out;
    if (ALG == HASH_KECCAK256) {
        out = keccak256_output(keccak256_message(m), form);
    } else {
        Sha256State s = sha256_message(m);
        if (ALG == HASH_SHA256D) s = sha256_of_digest(s);
        out = sha256_output(s, form);
    }
    hash_store_packed(out32, i, out);
    return bad;
}
// msg32 and sk32 taken modulo the order FN::m exactly as the signer takes them (sign.hpp sign_scalar); the order itself
// travels to the generator as a value
// (include/p2e.h BUFFER OVERLAP relies on this body reading every input of element i before its first store)
template <class FN>
P2E_HD void body_nonce(const uint8_t* msg32, const uint8_t* sk32, uint8_t* k32, size_t i) {
    const U256 x = fe_canon<FN>(hash_load_packed(sk32, i));
    const U256 z = hash_load_packed(msg32, i);   // (rfc6979_nonce reduces it)
    hash_store_packed(k32, i, rfc6979_nonce(hash_modulus<FN>(), x, z));
}
// err nullable; err[i] != 0: twenty zero bytes
P2E_HD void body_eth_address(const uint8_t* pkx32, const uint8_t* pky32, const uint8_t* err, uint8_t* addr20, size_t i) {
    EthAddress a = eth_address(hash_load_packed(pkx32, i), hash_load_packed(pky32, i));
    const bool flagged = err && err[i] != 0;
    u32* p = reinterpret_cast<u32*>(addr20 + 20 * i);
    P2E_UNROLL
    for (int k = 0; k < 5; k++) p[k] = flagged ? 0u : a.w[k];
}

#if defined(__HIPCC__)
// thread g owns element g
template <int ALG>
__global__ __launch_bounds__(256) void k_hash(const uint8_t* data, const uint64_t* offsets, uint8_t* out32, size_t n, unsigned form,
                                              unsigned long long* counter) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    bool bad = false;
    if (i < n) bad = body_hash<ALG>(data, offsets, out32, i, form);
    const unsigned long long m = __ballot(bad);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(counter, (unsigned long long)__popcll(m));
}
template <class FN>
__global__ __launch_bounds__(256) void k_nonce_rfc6979(const uint8_t* msg32, const uint8_t* sk32, uint8_t* k32, size_t n) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) body_nonce<FN>(msg32, sk32, k32, i);
}
// WITH_ERR = false: err is not looked at
template <bool WITH_ERR>
__global__ __launch_bounds__(256) void k_eth_address(const uint8_t* pkx32, const uint8_t* pky32, const uint8_t* err, uint8_t* addr20,
                                                     size_t n) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) body_eth_address(pkx32, pky32, WITH_ERR ? err : nullptr, addr20, i);
}
#endif

}  // namespace p2e

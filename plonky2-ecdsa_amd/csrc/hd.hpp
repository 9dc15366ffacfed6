// Hierarchical-deterministic keys and Bitcoin key hashes on secp256k1, for a batch (include/p2e.h p2e_bip32_master_batch,
// p2e_bip32_ckd_priv_batch, p2e_bip32_ckd_pub_batch, p2e_key_hash160_batch, p2e_hash160_batch).  The reference has no
// counterpart: curve/ecdsa.rs holds field elements and nothing derives keys.  What is computed here is defined by
//   BIP-32            master key generation, CKDpriv, CKDpub (the public derivation of a non-hardened child);
//   FIPS 180-4        SHA-512 (section 6.4) -- and SHA-256, which is hash.hpp's;
//   RFC 2104          HMAC, here HMAC-SHA512 in the two shapes BIP-32 needs;
//   RIPEMD-160        Dobbertin, Bosselaers, Preneel, "RIPEMD-160: a strengthened version of RIPEMD" (1996);
//   HASH160           RIPEMD-160(SHA-256(.)), Bitcoin's key hash (P2PKH / P2WPKH payload, the BIP-32 fingerprint's source).
// Nothing here is new arithmetic: I_L G is sign.hpp's one-lane fixed-base walk, the one addition with the parent is
// pmsm.hpp's complete msm_add (it doubles where I_L G = K_par and yields the neutral element where I_L G = -K_par), the
// inversion is sign_to_affine's, the curve test is pmsm.hpp's msm_on_curve.
//
// Bytes.  Keys and coordinates are the library's 32-byte little-endian values (they chain into every other call); chain
// codes are 32 bytes in the standard's order; an index is a uint32; hashes are in the order their standard defines.
//
// Codes.  err[i] is a WIRE_* code (wire.hpp), the first failing check in the order include/p2e.h gives; a flagged element
// writes zeros to ALL its outputs, the chain code included.
//
// Registers.  SHA-512 works on 64-bit words held as register pairs.  Every index of the schedule (16 words) and of the
// state is a compile-time constant; a rotation is written on the two 32-bit halves, one funnel shift (v_alignbit_b32)
// each, the halves swapped first for a rotation by 32 or more (hash.hpp's keccak_rotl, turned right); the additions are
// plain 64-bit C++.  The 80 rounds are unrolled BY 16 -- one pass over the schedule, so its indices stay constant -- and the
// five passes stay a rolled loop whose round constants come from a table indexed by a wave-uniform counter: 80 unrolled
// 64-bit rounds are tens of KB of code, and a derivation runs four compressions.  RIPEMD-160's two lines of 80 rounds are
// unrolled: every message word and shift is selected at compile time.  Nothing lives in the private segment, no LDS.
//
// One copy of the rounds, and no call.  HMAC-SHA512 under a 32-byte chain code is four compressions: the ipad block and the
// message block, the opad block and the digest block.  hash.hpp keeps its code small by NOT inlining the SHA-256
// compression; the same shape does not carry over to SHA-512 on this target, for two reasons the compiler's resource
// report shows (profiles/hd_kernel_resources.txt):
//   - a call passes at most 32 VGPRs of arguments in registers, the rest through the private segment.  A chaining value
//     and a digest block are 16 + 16 words already, so the compression alone cannot be the callee without scratch; the
//     smallest callee that fits is "key block, then one message block" (26 words);
//   - a callee may only use caller-saved registers without saving them (to scratch), and those are every other group of
//     eight above v39.  The ~130 registers the rounds need then reach v225: all three derivation kernels drop to 226
//     VGPRs and 2 waves per SIMD, the master-key kernel included, which has no curve arithmetic at all.
// So the four compressions are ONE rolled loop (hmac512_one_block) with the compression inlined in its body: each kernel
// holds the rounds once, exactly as with a call, and its registers are allocated with the kernel's.  Every derivation runs
// that loop once (CKDpriv merges its hardened and its ordinary data before it).  A master key is the same loop under the
// constant "Bitcoin seed" key states (hmac512_seed_key), whose two key trips compress nothing.
//
// Secrets (k_par, I_L, k_child) live in registers only; what is stored is the child key and its chain code.
#pragma once
#include "hash.hpp"
#include "point_arith.hpp"
#include "point_table.hpp"

namespace p2e {

typedef Secp256k1 HdCV;
constexpr u32 BIP32_HARDENED = 0x80000000u;

// ---------------------------------------------------------------------------------------------------------------------
// SHA-512
// ---------------------------------------------------------------------------------------------------------------------
struct Sha512State {
    u64 h[8];
};
struct Sha512Block {
    u64 w[16];   // the block's sixteen big-endian words
};
P2E_HD u64 sha512_k(int t) {
    static constexpr u64 K[80] = {
        0x428a2f98d728ae22ull, 0x7137449123ef65cdull, 0xb5c0fbcfec4d3b2full, 0xe9b5dba58189dbbcull, 0x3956c25bf348b538ull, 0x59f111f1b605d019ull,
        0x923f82a4af194f9bull, 0xab1c5ed5da6d8118ull, 0xd807aa98a3030242ull, 0x12835b0145706fbeull, 0x243185be4ee4b28cull, 0x550c7dc3d5ffb4e2ull,
        0x72be5d74f27b896full, 0x80deb1fe3b1696b1ull, 0x9bdc06a725c71235ull, 0xc19bf174cf692694ull, 0xe49b69c19ef14ad2ull, 0xefbe4786384f25e3ull,
        0x0fc19dc68b8cd5b5ull, 0x240ca1cc77ac9c65ull, 0x2de92c6f592b0275ull, 0x4a7484aa6ea6e483ull, 0x5cb0a9dcbd41fbd4ull, 0x76f988da831153b5ull,
        0x983e5152ee66dfabull, 0xa831c66d2db43210ull, 0xb00327c898fb213full, 0xbf597fc7beef0ee4ull, 0xc6e00bf33da88fc2ull, 0xd5a79147930aa725ull,
        0x06ca6351e003826full, 0x142929670a0e6e70ull, 0x27b70a8546d22ffcull, 0x2e1b21385c26c926ull, 0x4d2c6dfc5ac42aedull, 0x53380d139d95b3dfull,
        0x650a73548baf63deull, 0x766a0abb3c77b2a8ull, 0x81c2c92e47edaee6ull, 0x92722c851482353bull, 0xa2bfe8a14cf10364ull, 0xa81a664bbc423001ull,
        0xc24b8b70d0f89791ull, 0xc76c51a30654be30ull, 0xd192e819d6ef5218ull, 0xd69906245565a910ull, 0xf40e35855771202aull, 0x106aa07032bbd1b8ull,
        0x19a4c116b8d2d0c8ull, 0x1e376c085141ab53ull, 0x2748774cdf8eeb99ull, 0x34b0bcb5e19b48a8ull, 0x391c0cb3c5c95a63ull, 0x4ed8aa4ae3418acbull,
        0x5b9cca4f7763e373ull, 0x682e6ff3d6b2b8a3ull, 0x748f82ee5defb2fcull, 0x78a5636f43172f60ull, 0x84c87814a1f0ab72ull, 0x8cc702081a6439ecull,
        0x90befffa23631e28ull, 0xa4506cebde82bde9ull, 0xbef9a3f7b2c67915ull, 0xc67178f2e372532bull, 0xca273eceea26619cull, 0xd186b8c721c0c207ull,
        0xeada7dd6cde0eb1eull, 0xf57d4f7fee6ed178ull, 0x06f067aa72176fbaull, 0x0a637dc5a2c898a6ull, 0x113f9804bef90daeull, 0x1b710b35131c471bull,
        0x28db77f523047d84ull, 0x32caab7b40c72493ull, 0x3c9ebe0a15c9bebcull, 0x431d67c49c100d4cull, 0x4cc5d4becb3e42b6ull, 0x597f299cfc657e2aull,
        0x5fcb6fab3ad6faecull, 0x6c44198c4a475817ull};
    return K[t];
}
P2E_HD Sha512State sha512_iv() {
    Sha512State s;
    s.h[0] = 0x6a09e667f3bcc908ull, s.h[1] = 0xbb67ae8584caa73bull, s.h[2] = 0x3c6ef372fe94f82bull, s.h[3] = 0xa54ff53a5f1d36f1ull;
    s.h[4] = 0x510e527fade682d1ull, s.h[5] = 0x9b05688c2b3e6c1full, s.h[6] = 0x1f83d9abfb41bd6bull, s.h[7] = 0x5be0cd19137e2179ull;
    return s;
}
// rotate right by the constant R: two funnel shifts on the halves, which are swapped first for R >= 32
template <int R>
P2E_HD u64 sha512_rotr(u64 v) {
    constexpr int S = R & 31;
    static_assert(R > 0 && R < 64 && S != 0, "no rotation of SHA-512 is a multiple of 32");
    const u32 lo = (u32)v, hi = (u32)(v >> 32);
    const u32 a = R >= 32 ? hi : lo, b = R >= 32 ? lo : hi;   // b:a = v rotated by 32 (R >= 32) or as it is
    const u32 rl = (a >> S) | (b << (32 - S)), rh = (b >> S) | (a << (32 - S));
    return ((u64)rh << 32) | rl;
}
// One round with the working variables rotated BY NAME (hash.hpp's P2E_SHA_ROUND); j = the round's place in its pass of 16
#define P2E_SHA512_ROUND(a, b, c, d, e, f, g, h, j)                                                                          \
    {                                                                                                                        \
        const u64 t1 = h + (sha512_rotr<14>(e) ^ sha512_rotr<18>(e) ^ sha512_rotr<41>(e)) + (g ^ (e & (f ^ g))) +            \
                       sha512_k(pass + (j)) + w[j];                                                                          \
        const u64 t2 = (sha512_rotr<28>(a) ^ sha512_rotr<34>(a) ^ sha512_rotr<39>(a)) + ((a & b) | (c & (a | b)));           \
        d += t1;                                                                                                             \
        h = t1 + t2;                                                                                                         \
    }
P2E_HD Sha512State sha512_compress(const Sha512State& s, const Sha512Block& blk) {
    u64 w[16];
    P2E_UNROLL
    for (int j = 0; j < 16; j++) w[j] = blk.w[j];
    u64 a = s.h[0], b = s.h[1], c = s.h[2], d = s.h[3], e = s.h[4], f = s.h[5], g = s.h[6], h = s.h[7];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
    for (int pass = 0; pass < 80; pass += 16) {
        P2E_SHA512_ROUND(a, b, c, d, e, f, g, h, 0)
        P2E_SHA512_ROUND(h, a, b, c, d, e, f, g, 1)
        P2E_SHA512_ROUND(g, h, a, b, c, d, e, f, 2)
        P2E_SHA512_ROUND(f, g, h, a, b, c, d, e, 3)
        P2E_SHA512_ROUND(e, f, g, h, a, b, c, d, 4)
        P2E_SHA512_ROUND(d, e, f, g, h, a, b, c, 5)
        P2E_SHA512_ROUND(c, d, e, f, g, h, a, b, 6)
        P2E_SHA512_ROUND(b, c, d, e, f, g, h, a, 7)
        P2E_SHA512_ROUND(a, b, c, d, e, f, g, h, 8)
        P2E_SHA512_ROUND(h, a, b, c, d, e, f, g, 9)
        P2E_SHA512_ROUND(g, h, a, b, c, d, e, f, 10)
        P2E_SHA512_ROUND(f, g, h, a, b, c, d, e, 11)
        P2E_SHA512_ROUND(e, f, g, h, a, b, c, d, 12)
        P2E_SHA512_ROUND(d, e, f, g, h, a, b, c, 13)
        P2E_SHA512_ROUND(c, d, e, f, g, h, a, b, 14)
        P2E_SHA512_ROUND(b, c, d, e, f, g, h, a, 15)
        if (pass < 64) {   // the next sixteen schedule words, in place and in order (word j + 16 needs j + 1, j + 9, j + 14)
            P2E_UNROLL
            for (int j = 0; j < 16; j++) {
                const u64 w15 = w[(j + 1) & 15], w2 = w[(j + 14) & 15];
                w[j] += (sha512_rotr<1>(w15) ^ sha512_rotr<8>(w15) ^ (w15 >> 7)) + w[(j + 9) & 15] +
                        (sha512_rotr<19>(w2) ^ sha512_rotr<61>(w2) ^ (w2 >> 6));
            }
        }
    }
    Sha512State r;
    r.h[0] = s.h[0] + a, r.h[1] = s.h[1] + b, r.h[2] = s.h[2] + c, r.h[3] = s.h[3] + d;
    r.h[4] = s.h[4] + e, r.h[5] = s.h[5] + f, r.h[6] = s.h[6] + g, r.h[7] = s.h[7] + h;
    return r;
}
#undef P2E_SHA512_ROUND

// ---------------------------------------------------------------------------------------------------------------------
// HMAC-SHA512 in BIP-32's shapes.  A 32-byte key is 8 big-endian 32-bit words (hash.hpp's Words8: word 0 = bytes 0 .. 3).
// ---------------------------------------------------------------------------------------------------------------------
struct HmacKey512 {
    Sha512State inner, outer;   // the states after the ipad and the opad block
};
constexpr u64 HMAC512_IPAD = 0x3636363636363636ull, HMAC512_OPAD = 0x5c5c5c5c5c5c5c5cull;
P2E_HD Sha512Block hmac512_key_block(const Words8& k, u64 pad) {
    Sha512Block b;
    P2E_UNROLL
    for (int j = 0; j < 16; j++) b.w[j] = (j < 4 ? (((u64)k.w[2 * (j & 3)] << 32) | k.w[2 * (j & 3) + 1]) : 0ull) ^ pad;
    return b;
}
// both key states of a 32-byte key, each one compression from the IV (the CPU harness and the documentation of the call below)
P2E_HD HmacKey512 hmac512_key(const Words8& k) {
    HmacKey512 hk;
    hk.inner = sha512_compress(sha512_iv(), hmac512_key_block(k, HMAC512_IPAD));
    hk.outer = sha512_compress(sha512_iv(), hmac512_key_block(k, HMAC512_OPAD));
    return hk;
}
// the key states of the 12 bytes "Bitcoin seed": constants (tests/test_hd_cpu.py recomputes them)
P2E_HD HmacKey512 hmac512_seed_key() {
    HmacKey512 hk;
    hk.inner.h[0] = 0x2e2af459060c1873ull, hk.inner.h[1] = 0x7894b868dc88433aull, hk.inner.h[2] = 0xdd1a797ef1a1933aull;
    hk.inner.h[3] = 0xe6486d04fcb412a7ull, hk.inner.h[4] = 0xfbcc67b9a396caa0ull, hk.inner.h[5] = 0xa2970b146f49b65eull;
    hk.inner.h[6] = 0xfdf1daabc66f6248ull, hk.inner.h[7] = 0x2ff99c812ada6dc3ull;
    hk.outer.h[0] = 0xbbd27bac212e9dbdull, hk.outer.h[1] = 0xdd0bc55e7e4037c1ull, hk.outer.h[2] = 0xdfdd3d6890bd6424ull;
    hk.outer.h[3] = 0x2902de663032b34cull, hk.outer.h[4] = 0xa30f8aa6f67899fcull, hk.outer.h[5] = 0x69a566c30f88378full;
    hk.outer.h[6] = 0x0500247985ecb694ull, hk.outer.h[7] = 0xf6d70307c6b2d337ull;
    return hk;
}
// HMAC-SHA512 of ONE message block under a 32-byte key, or under the seed key (`seeded`: `key` is not looked at).
// The message block is m[0 .. 8) (its first 64 bytes, the 0x80 byte included where it falls there), then the byte 0x80 at
// offset 64 where `tail` has bit 31, zeros, and the length tail & 0x7FFFFFFF in bits in its last word.
// The whole HMAC is one rolled loop with the compression inside it ONCE (see the header):
//   trip 0  IV, key ^ ipad           trip 1  the message block (its digest replaces m)
//   trip 2  IV, key ^ opad           trip 3  the digest block: 64 bytes, 0x80, 8 (128 + 64) bits
// Under the seed key trips 0 and 2 load a constant and compress nothing.
constexpr u32 HMAC512_TAIL_MARK = 0x80000000u;
P2E_HD Sha512State hmac512_one_block(bool seeded, u32 tail, const Words8& key, const u64 (&msg)[8]) {
    const HmacKey512 sk = hmac512_seed_key();
    const Sha512State iv = sha512_iv();
    u64 m[8];
    P2E_UNROLL
    for (int j = 0; j < 8; j++) m[j] = msg[j];
    Sha512State st = iv;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
    for (u32 trip = 0; trip < 4u; trip++) {
        const bool outer = trip >= 2u, keyed = (trip & 1u) == 0;
        Sha512Block b;
        if (keyed) {
            P2E_UNROLL
            for (int j = 0; j < 8; j++) st.h[j] = seeded ? (outer ? sk.outer.h[j] : sk.inner.h[j]) : iv.h[j];
            if (seeded) continue;
            b = hmac512_key_block(key, outer ? HMAC512_OPAD : HMAC512_IPAD);
        } else {
            const u32 t = outer ? (HMAC512_TAIL_MARK | (8u * (128u + 64u))) : tail;
            P2E_UNROLL
            for (int j = 0; j < 8; j++) b.w[j] = m[j];
            b.w[8] = (t & HMAC512_TAIL_MARK) ? 0x8000000000000000ull : 0ull;
            P2E_UNROLL
            for (int j = 9; j < 15; j++) b.w[j] = 0ull;
            b.w[15] = (u64)(t & ~HMAC512_TAIL_MARK);
        }
        st = sha512_compress(st, b);
        if (!keyed) {
            P2E_UNROLL
            for (int j = 0; j < 8; j++) m[j] = st.h[j];
        }
    }
    return st;
}

// I = I_L || I_R: I_L as the integer parse256 gives, I_R as the child's chain code (8 big-endian words = its bytes in order)
struct Bip32I {
    U256 il;
    Words8 ir;
};
P2E_HD Bip32I bip32_split(const Sha512State& s) {
    Bip32I r;
    P2E_UNROLL
    for (int j = 0; j < 4; j++) {
        r.il.w[7 - 2 * j] = (u32)(s.h[j] >> 32), r.il.w[6 - 2 * j] = (u32)s.h[j];
        r.ir.w[2 * j] = (u32)(s.h[4 + j] >> 32), r.ir.w[2 * j + 1] = (u32)s.h[4 + j];
    }
    return r;
}
// I = HMAC-SHA512(key = cc, data = b0 || ser256(v) || ser32(index)): the 37 bytes of CKDpriv and CKDpub.
// b0 = 00 and v = k_par for a hardened child, b0 = 02 | 03 and v = x(K_par) otherwise.  Four compressions.
P2E_HD Bip32I bip32_I(const Words8& cc, u32 b0, const U256& v, u32 index) {
    u32 d[10];   // the data as big-endian words: everything behind b0 sits one byte off the word grid
    d[0] = (b0 << 24) | (v.w[7] >> 8);
    P2E_UNROLL
    for (int j = 1; j < 8; j++) d[j] = (v.w[8 - j] << 24) | (v.w[7 - j] >> 8);
    d[8] = (v.w[0] << 24) | (index >> 8);
    d[9] = (index << 24) | 0x00800000u;   // and the 0x80 that ends the message
    u64 m[8];
    P2E_UNROLL
    for (int j = 0; j < 8; j++) m[j] = j < 5 ? (((u64)d[2 * (j % 5)] << 32) | d[2 * (j % 5) + 1]) : 0ull;
    return bip32_split(hmac512_one_block(false, 8u * (128u + 37u), cc, m));
}
// I = HMAC-SHA512(key = "Bitcoin seed", data = the message `seed` of 16 .. 64 bytes): two compressions behind the constants
P2E_HD Bip32I bip32_master_I(const MsgView& seed) {
    u32 d[16];   // the first 64 bytes as big-endian words (hash.hpp's absorption), the 0x80 byte where the seed ends before byte 64
    u32 carry = seed.word(0);
    P2E_UNROLL
    for (int j = 0; j < 16; j++) {
        const u32 next = seed.word((u64)j + 1);
        u32 v = hash_bswap32(hash_join(carry, next, seed.sh));
        carry = next;
        const u64 at = 4 * (u64)j;
        if (at + 4 > seed.len) {
            const u32 keep = at < seed.len ? (u32)(seed.len - at) : 0u;
            const u32 cut = 0xFFFFFFFFu >> (8 * keep);
            v = at <= seed.len ? ((v & ~cut) | (0x80000000u >> (8 * keep))) : 0u;
        }
        d[j] = v;
    }
    u64 m[8];
    P2E_UNROLL
    for (int j = 0; j < 8; j++) m[j] = ((u64)d[2 * j] << 32) | d[2 * j + 1];
    Words8 none;
    P2E_UNROLL
    for (int j = 0; j < 8; j++) none.w[j] = 0;
    const u32 tail = (seed.len == 64 ? HMAC512_TAIL_MARK : 0u) | (8u * (128u + (u32)seed.len));
    return bip32_split(hmac512_one_block(true, tail, none, m));
}

// ---------------------------------------------------------------------------------------------------------------------
// RIPEMD-160 and HASH160
// ---------------------------------------------------------------------------------------------------------------------
struct Ripemd160State {
    u32 h[5];
};
P2E_HD Ripemd160State ripemd160_iv() {
    Ripemd160State s;
    s.h[0] = 0x67452301u, s.h[1] = 0xEFCDAB89u, s.h[2] = 0x98BADCFEu, s.h[3] = 0x10325476u, s.h[4] = 0xC3D2E1F0u;
    return s;
}
// the paper's f_1 .. f_5 (F = 0 .. 4) and added constants; the right line runs them backwards
template <int F>
P2E_HD u32 ripemd160_f(u32 x, u32 y, u32 z) {
    return F == 0 ? (x ^ y ^ z) : F == 1 ? ((x & y) | (~x & z)) : F == 2 ? ((x | ~y) ^ z) : F == 3 ? ((x & z) | (y & ~z)) : (x ^ (y | ~z));
}
// one step of either line on working variables rotated BY NAME: message word and shift are the caller's constants
template <int F, int S>
P2E_HD void ripemd160_step(u32& a, u32 b, u32& c, u32 d, u32 e, u32 x, u32 k) {
    const u32 t = a + ripemd160_f<F>(b, c, d) + x + k;
    a = ((t << S) | (t >> (32 - S))) + e;
    c = (c << 10) | (c >> 22);
}
// sixteen steps of one line: function F, constant K, message words R0 .. R15 with shifts S0 .. S15.  Sixteen is one more
// than a multiple of five: the names (a, b, c, d, e) leave a group rotated by one place, which the next group's caller undoes.
#define P2E_RMD_5(F, K, a, b, c, d, e, r0, s0, r1, s1, r2, s2, r3, s3, r4, s4) \
    ripemd160_step<F, s0>(a, b, c, d, e, x[r0], K);                            \
    ripemd160_step<F, s1>(e, a, b, c, d, x[r1], K);                            \
    ripemd160_step<F, s2>(d, e, a, b, c, x[r2], K);                            \
    ripemd160_step<F, s3>(c, d, e, a, b, x[r3], K);                            \
    ripemd160_step<F, s4>(b, c, d, e, a, x[r4], K);
#define P2E_RMD_16(F, K, a, b, c, d, e, r0, s0, r1, s1, r2, s2, r3, s3, r4, s4, r5, s5, r6, s6, r7, s7, r8, s8, r9, s9, r10, s10, r11, s11, r12, \
                   s12, r13, s13, r14, s14, r15, s15)                                                                                           \
    P2E_RMD_5(F, K, a, b, c, d, e, r0, s0, r1, s1, r2, s2, r3, s3, r4, s4)                                                                      \
    P2E_RMD_5(F, K, a, b, c, d, e, r5, s5, r6, s6, r7, s7, r8, s8, r9, s9)                                                                      \
    P2E_RMD_5(F, K, a, b, c, d, e, r10, s10, r11, s11, r12, s12, r13, s13, r14, s14)                                                            \
    ripemd160_step<F, s15>(a, b, c, d, e, x[r15], K);
P2E_HD Ripemd160State ripemd160_compress(const Ripemd160State& s, const u32 (&x)[16]) {   // x: the block's little-endian words
    u32 al = s.h[0], bl = s.h[1], cl = s.h[2], dl = s.h[3], el = s.h[4];
    u32 ar = s.h[0], br = s.h[1], cr = s.h[2], dr = s.h[3], er = s.h[4];
    // the left line
    P2E_RMD_16(0, 0x00000000u, al, bl, cl, dl, el, 0, 11, 1, 14, 2, 15, 3, 12, 4, 5, 5, 8, 6, 7, 7, 9, 8, 11, 9, 13, 10, 14, 11, 15, 12, 6, 13, 7,
               14, 9, 15, 8)
    P2E_RMD_16(1, 0x5A827999u, el, al, bl, cl, dl, 7, 7, 4, 6, 13, 8, 1, 13, 10, 11, 6, 9, 15, 7, 3, 15, 12, 7, 0, 12, 9, 15, 5, 9, 2, 11, 14, 7,
               11, 13, 8, 12)
    P2E_RMD_16(2, 0x6ED9EBA1u, dl, el, al, bl, cl, 3, 11, 10, 13, 14, 6, 4, 7, 9, 14, 15, 9, 8, 13, 1, 15, 2, 14, 7, 8, 0, 13, 6, 6, 13, 5, 11, 12,
               5, 7, 12, 5)
    P2E_RMD_16(3, 0x8F1BBCDCu, cl, dl, el, al, bl, 1, 11, 9, 12, 11, 14, 10, 15, 0, 14, 8, 15, 12, 9, 4, 8, 13, 9, 3, 14, 7, 5, 15, 6, 14, 8, 5, 6,
               6, 5, 2, 12)
    P2E_RMD_16(4, 0xA953FD4Eu, bl, cl, dl, el, al, 4, 9, 0, 15, 5, 5, 9, 11, 7, 6, 12, 8, 2, 13, 10, 12, 14, 5, 1, 12, 3, 13, 8, 14, 11, 11, 6, 8,
               15, 5, 13, 6)
    // the right line
    P2E_RMD_16(4, 0x50A28BE6u, ar, br, cr, dr, er, 5, 8, 14, 9, 7, 9, 0, 11, 9, 13, 2, 15, 11, 15, 4, 5, 13, 7, 6, 7, 15, 8, 8, 11, 1, 14, 10, 14,
               3, 12, 12, 6)
    P2E_RMD_16(3, 0x5C4DD124u, er, ar, br, cr, dr, 6, 9, 11, 13, 3, 15, 7, 7, 0, 12, 13, 8, 5, 9, 10, 11, 14, 7, 15, 7, 8, 12, 12, 7, 4, 6, 9, 15,
               1, 13, 2, 11)
    P2E_RMD_16(2, 0x6D703EF3u, dr, er, ar, br, cr, 15, 9, 5, 7, 1, 15, 3, 11, 7, 8, 14, 6, 6, 6, 9, 14, 11, 12, 8, 13, 12, 5, 2, 14, 10, 13, 0, 13,
               4, 7, 13, 5)
    P2E_RMD_16(1, 0x7A6D76E9u, cr, dr, er, ar, br, 8, 15, 6, 5, 4, 8, 1, 11, 3, 14, 11, 14, 15, 6, 0, 14, 5, 6, 12, 9, 2, 12, 13, 9, 9, 12, 7, 5,
               10, 15, 14, 8)
    P2E_RMD_16(0, 0x00000000u, br, cr, dr, er, ar, 12, 8, 15, 5, 10, 12, 4, 9, 1, 12, 5, 5, 8, 14, 7, 6, 6, 8, 2, 13, 13, 6, 14, 5, 0, 15, 3, 13,
               9, 11, 11, 11)
    Ripemd160State r;
    r.h[0] = s.h[1] + cl + dr, r.h[1] = s.h[2] + dl + er, r.h[2] = s.h[3] + el + ar, r.h[3] = s.h[4] + al + br, r.h[4] = s.h[0] + bl + cr;
    return r;
}
#undef P2E_RMD_16
#undef P2E_RMD_5
// the digest as five words to store in order (little-endian words are the digest's bytes)
struct Hash160 {
    u32 w[5];
};
// RIPEMD-160 of a SHA-256 digest (8 big-endian words): 32 bytes, one block from the IV
P2E_HD Hash160 hash160_of_digest(const Words8& d) {
    u32 x[16];
    P2E_UNROLL
    for (int j = 0; j < 16; j++) x[j] = j < 8 ? hash_bswap32(d.w[j & 7]) : 0u;
    x[8] = 0x80u;
    x[14] = 256u;
    const Ripemd160State s = ripemd160_compress(ripemd160_iv(), x);
    Hash160 r;
    P2E_UNROLL
    for (int j = 0; j < 5; j++) r.w[j] = s.h[j];
    return r;
}
P2E_HD Words8 hd_digest_words(const Sha256State& s) {
    Words8 r;
    P2E_UNROLL
    for (int j = 0; j < 8; j++) r.w[j] = s.h[j];
    return r;
}
// HASH160 of the SEC1 string of (x, y), both this library's little-endian values: 02 | 03 || x (one SHA-256 block) or
// 04 || x || y (two).  Nothing is checked: like the Ethereum address, the hash of any coordinate pair is defined.
P2E_HD Hash160 key_hash160(const U256& x, const U256& y, int form) {
    Sha256Block b;
    Sha256State st;
    const u32 b0 = form == SEC1_COMPRESSED ? (2u | (y.w[0] & 1u)) : 4u;
    b.w[0] = (b0 << 24) | (x.w[7] >> 8);
    P2E_UNROLL
    for (int j = 1; j < 8; j++) b.w[j] = (x.w[8 - j] << 24) | (x.w[7 - j] >> 8);
    if (form == SEC1_COMPRESSED) {
        b.w[8] = (x.w[0] << 24) | 0x00800000u;
        sha256_finish_block(b, 9, 8 * 33);
        st = sha256_compress_call(sha256_iv(), b);
    } else {
        b.w[8] = (x.w[0] << 24) | (y.w[7] >> 8);
        P2E_UNROLL
        for (int j = 1; j < 8; j++) b.w[8 + j] = (y.w[8 - j] << 24) | (y.w[7 - j] >> 8);
        st = sha256_compress_call(sha256_iv(), b);
        b.w[0] = (y.w[0] << 24) | 0x00800000u;
        sha256_finish_block(b, 1, 8 * 65);
        st = sha256_compress_call(st, b);
    }
    return hash160_of_digest(hd_digest_words(st));
}

// ---------------------------------------------------------------------------------------------------------------------
// the derivations, split at the hash: what follows I_L is arithmetic that a test can drive with any I_L
// ---------------------------------------------------------------------------------------------------------------------
// k_child = I_L + k_par mod n.  I_L >= n: WIRE_SCALAR_RANGE; k_child = 0: WIRE_INFINITY.  I_L = 0 is valid (child = parent).
P2E_HD uint8_t bip32_finish_priv(const U256& il, const U256& k_par, U256& k_child) {
    typedef HdCV::Fn Fn;
    if (geq_mod<Fn>(il.w)) return WIRE_SCALAR_RANGE;
    k_child = fe_add<Fn>(il, k_par);
    return u256_is_zero(k_child) ? WIRE_INFINITY : WIRE_OK;
}
// K_child = I_L G + K_par for a parent that is on the curve.  I_L >= n: WIRE_SCALAR_RANGE; the neutral element:
// WIRE_INFINITY.  I_L = 0 (an empty walk: child = parent) and I_L G = K_par (the doubling) are computed.
P2E_HD uint8_t bip32_finish_pub(const Aff* T, const U256& il, const Aff& K_par, Aff& K_child) {
    if (geq_mod<HdCV::Fn>(il.w)) return WIRE_SCALAR_RANGE;
    const SignSum<HdCV> A_ = sign_base_mul<HdCV, SIGN_PLAN_LANE>(T, il, 0);
    SignSum<HdCV> B;
    B.p = SignArith<HdCV>::from_aff(K_par);
    B.have = true;
    const SignSum<HdCV> s = msm_add<HdCV, true>(A_, B);
    if (!s.have || !sign_to_affine<HdCV, true>(s, K_child.x, K_child.y)) return WIRE_INFINITY;   // (a zero Z under `have` cannot occur)
    return WIRE_OK;
}

// 32 bytes in their standard's order at base + 32 i (4-byte aligned) <-> 8 big-endian words
P2E_HD Words8 hd_load_cc(const uint8_t* base, size_t i) {
    const u32* q = reinterpret_cast<const u32*>(base + 32 * i);
    Words8 r;
    P2E_UNROLL
    for (int j = 0; j < 8; j++) r.w[j] = hash_bswap32(q[j]);
    return r;
}
P2E_HD void hd_store_cc(uint8_t* base, size_t i, const Words8& v, bool zero) {
    u32* q = reinterpret_cast<u32*>(base + 32 * i);
    P2E_UNROLL
    for (int j = 0; j < 8; j++) q[j] = zero ? 0u : hash_bswap32(v.w[j]);
}
P2E_HD void hd_store_key(uint8_t* base, size_t i, const U256& v, bool zero) {
    u32* q = reinterpret_cast<u32*>(base + 32 * i);
    P2E_UNROLL
    for (int j = 0; j < 8; j++) q[j] = zero ? 0u : v.w[j];
}

// ---- call 1: the master key of seed i = seed[seed_len i, seed_len (i + 1)), 16 <= seed_len <= 64 ------------------------------
P2E_HD uint8_t body_bip32_master(const uint8_t* seed, u32 seed_len, uint8_t* sk32, uint8_t* cc32, size_t i) {
    MsgView m;
    const uintptr_t a = (uintptr_t)(seed + (size_t)seed_len * i);
    m.len = seed_len;
    m.p = reinterpret_cast<const u32*>(a & ~(uintptr_t)3);
    m.sh = 8u * (u32)(a & 3u);
    m.end = a + seed_len;
    const Bip32I I = bip32_master_I(m);
    const uint8_t e = (u256_is_zero(I.il) || geq_mod<HdCV::Fn>(I.il.w)) ? WIRE_SCALAR_RANGE : WIRE_OK;
    hd_store_key(sk32, i, I.il, e != 0);
    hd_store_cc(cc32, i, I.ir, e != 0);
    return e;
}

// ---- call 2: CKDpriv.  Element i derives from parent `p` (i, or 0 where one parent serves the batch) ----------------------------
// (include/p2e.h BUFFER OVERLAP relies on this body reading every input of element i before its first store)
P2E_HD uint8_t body_bip32_ckd_priv(const Aff* T, const uint8_t* par_sk32, const uint8_t* par_cc32, size_t p, const uint32_t* index,
                                   uint8_t* sk32, uint8_t* cc32, size_t i) {
    const U256 k = load_packed(par_sk32, p);
    const u32 idx = index[i];
    uint8_t e = WIRE_OK;
    U256 kc = u256_zero();
    Words8 ir;
    P2E_UNROLL
    for (int j = 0; j < 8; j++) ir.w[j] = 0;
    if (u256_is_zero(k) || geq_mod<HdCV::Fn>(k.w)) {   // (not reduced: BIP-32 keys lie in [1, n - 1])
        e = WIRE_SCALAR_RANGE;
    } else {
        u32 b0 = 0;
        U256 v = k;
        if (idx < BIP32_HARDENED) {   // serP(k G): the generator's table, the cost of a public key
            U256 x = u256_zero(), y = u256_zero();
            const SignSum<HdCV> s = sign_base_mul<HdCV, SIGN_PLAN_LANE>(T, k, 0);
            if (!s.have || !sign_to_affine<HdCV, true>(s, x, y)) e = WIRE_INFINITY;   // (it cannot: 0 < k < n)
            b0 = 2u | (y.w[0] & 1u);
            v = x;
        }
        if (!e) {
            const Bip32I I = bip32_I(hd_load_cc(par_cc32, p), b0, v, idx);
            e = bip32_finish_priv(I.il, k, kc);
            ir = I.ir;
        }
    }
    hd_store_key(sk32, i, kc, e != 0);
    hd_store_cc(cc32, i, ir, e != 0);
    return e;
}

// ---- call 3: CKDpub -------------------------------------------------------------------------------------------------------------
// (include/p2e.h BUFFER OVERLAP relies on this body reading every input of element i before its first store)
P2E_HD uint8_t body_bip32_ckd_pub(const Aff* T, const uint8_t* par_pkx32, const uint8_t* par_pky32, const uint8_t* par_cc32, size_t p,
                                  const uint32_t* index, uint8_t* pkx32, uint8_t* pky32, uint8_t* cc32, size_t i) {
    Aff K, C;
    K.x = load_packed(par_pkx32, p), K.y = load_packed(par_pky32, p);
    C.x = C.y = u256_zero();
    const u32 idx = index[i];
    uint8_t e = WIRE_OK;
    Words8 ir;
    P2E_UNROLL
    for (int j = 0; j < 8; j++) ir.w[j] = 0;
    if (idx >= BIP32_HARDENED)   // a public parent has no hardened child
        e = WIRE_BAD_INDEX;
    else if (u256_is_zero(K.x) && u256_is_zero(K.y))
        e = WIRE_INFINITY;
    else if (geq_mod<HdCV::Fp>(K.x.w) || geq_mod<HdCV::Fp>(K.y.w))
        e = WIRE_COORD_RANGE;
    else if (!msm_on_curve<HdCV>(K.x, K.y))
        e = WIRE_NOT_ON_CURVE;
    if (!e) {
        const Bip32I I = bip32_I(hd_load_cc(par_cc32, p), 2u | (K.y.w[0] & 1u), K.x, idx);
        e = bip32_finish_pub(T, I.il, K, C);
        ir = I.ir;
    }
    hd_store_key(pkx32, i, C.x, e != 0);
    hd_store_key(pky32, i, C.y, e != 0);
    hd_store_cc(cc32, i, ir, e != 0);
    return e;
}

// ---- calls 4 and 5: HASH160 of a key, of a message ----------------------------------------------------------------------------
P2E_HD void hd_store_hash160(uint8_t* out20, size_t i, const Hash160& h, bool zero) {
    u32* p = reinterpret_cast<u32*>(out20 + 20 * i);
    P2E_UNROLL
    for (int k = 0; k < 5; k++) p[k] = zero ? 0u : h.w[k];
}
// err nullable; err[i] != 0: twenty zero bytes
P2E_HD void body_key_hash160(int form, const uint8_t* pkx32, const uint8_t* pky32, const uint8_t* err, uint8_t* out20, size_t i) {
    const Hash160 h = key_hash160(load_packed(pkx32, i), load_packed(pky32, i), form);
    hd_store_hash160(out20, i, h, err && err[i] != 0);
}
// returns true where offsets[i + 1] < offsets[i] (hashed as the empty message), as body_hash does
P2E_HD bool body_hash160(const uint8_t* data, const uint64_t* offsets, uint8_t* out20, size_t i) {
    bool bad;
    const MsgView m = msg_view(data, offsets, i, &bad);
    hd_store_hash160(out20, i, hash160_of_digest(hd_digest_words(sha256_message(m))), false);
    return bad;
}

#if defined(__HIPCC__)
// thread g owns element g; `broadcast`: every element derives from parent 0 (the scan of one extended key)
template <int UNUSED = 0>   // (templates so that every translation unit that includes this file may hold the definitions)
__global__ __launch_bounds__(256) void k_bip32_master(const uint8_t* seed, u32 seed_len, uint8_t* sk32, uint8_t* cc32, size_t n, uint8_t* err,
                                                      unsigned long long* counter) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    uint8_t e = 0;
    if (i < n) {
        e = body_bip32_master(seed, seed_len, sk32, cc32, i);
        err[i] = e;
    }
    sign_count_err(e, counter);
}
template <int UNUSED = 0>
__global__ __launch_bounds__(256) void k_bip32_ckd_priv(const Aff* T, const uint8_t* par_sk32, const uint8_t* par_cc32, int broadcast,
                                                        const uint32_t* index, uint8_t* sk32, uint8_t* cc32, size_t n, uint8_t* err,
                                                        unsigned long long* counter) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    uint8_t e = 0;
    if (i < n) {
        e = body_bip32_ckd_priv(T, par_sk32, par_cc32, broadcast ? 0 : i, index, sk32, cc32, i);
        err[i] = e;
    }
    sign_count_err(e, counter);
}
template <int UNUSED = 0>
__global__ __launch_bounds__(256) void k_bip32_ckd_pub(const Aff* T, const uint8_t* par_pkx32, const uint8_t* par_pky32,
                                                       const uint8_t* par_cc32, int broadcast, const uint32_t* index, uint8_t* pkx32,
                                                       uint8_t* pky32, uint8_t* cc32, size_t n, uint8_t* err, unsigned long long* counter) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    uint8_t e = 0;
    if (i < n) {
        e = body_bip32_ckd_pub(T, par_pkx32, par_pky32, par_cc32, broadcast ? 0 : i, index, pkx32, pky32, cc32, i);
        err[i] = e;
    }
    sign_count_err(e, counter);
}
// WITH_ERR = false: err is not looked at
template <int FORM, bool WITH_ERR>
__global__ __launch_bounds__(256) void k_key_hash160(const uint8_t* pkx32, const uint8_t* pky32, const uint8_t* err, uint8_t* out20, size_t n) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) body_key_hash160(FORM, pkx32, pky32, WITH_ERR ? err : nullptr, out20, i);
}
template <int UNUSED = 0>
__global__ __launch_bounds__(256) void k_hash160(const uint8_t* data, const uint64_t* offsets, uint8_t* out20, size_t n,
                                                 unsigned long long* counter) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    bool bad = false;
    if (i < n) bad = body_hash160(data, offsets, out20, i);
    const unsigned long long m = __ballot(bad);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(counter, (unsigned long long)__popcll(m));
}
#endif

}  // namespace p2e

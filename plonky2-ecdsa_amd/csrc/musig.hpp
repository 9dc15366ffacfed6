// MuSig2 (BIP-327) on secp256k1, for a batch (include/p2e.h p2e_musig_key_agg_batch, p2e_musig_apply_tweak_batch,
// p2e_musig_nonce_agg_batch, p2e_musig_session_batch, p2e_musig_partial_sign_batch, p2e_musig_partial_verify_batch,
// p2e_musig_sig_agg_batch): the multi-party form of a BIP-340 signature, from the key list to the final signature.  The
// reference has no counterpart: its only protocol is ECDSA (curve/ecdsa.rs).  Nothing here is new arithmetic: a_i P_i and
// b R_2 are point_arith.hpp's GLV walk, d' G, t G and s G sign.hpp's one-lane fixed-base walk, every sum pmsm.hpp's complete
// msm_add, the Taproot tweak taproot.hpp's taproot_tweak, SHA-256 hash.hpp's compression call.
//
// Bytes.  Points and the secret scalars of the key layer (pkx32 / pky32, sk32, secnonce64, pubnonce128, aggnonce128, the
// point of a keyagg192 record) are the library's 32-byte little-endian values (hd.hpp, sp.hpp).  What BIP-327 defines as a byte
// string or a hash (tweak32, msg32, psig32, agg_pk32, sig64, and tacc, L, pk2, b, e, x(R) inside the records) is the standard's
// big-endian string (schnorr.hpp).  The records are laid out in include/p2e.h; MusigKeyAgg and MusigSession are their
// register forms.
//
// Tagged hashes.  Each of "KeyAgg list", "KeyAgg coefficient", "MuSig/noncecoef" is a CONSTANT chaining value
// (musig_midstate; tests/test_musig_cpu.py recomputes them); the challenge is schnorr.hpp's, the Taproot tweak taproot.hpp's.
// The key list is a byte stream of 33-byte pieces, so its words do not sit on the block's word grid: MusigStream joins each
// big-endian word with the bytes held back from the word before it (hash.hpp's hash_join, as sha256_message does for a
// message at any alignment) and places it with register selects -- no indexed array, nothing in the private segment.  The
// coefficient hash (65 bytes) has a fixed layout: two compressions.  The nonce coefficient (130 bytes) goes through the stream.
//
// Codes.  err[i] is a WIRE_* code (wire.hpp), the first failing check in the order include/p2e.h gives; a flagged element
// writes zeros to all its outputs.  A zeroed record is refused by the next call (its point is (0, 0): WIRE_INFINITY), so a
// flag travels down the chain.
//
// Split at the hash (as sp.hpp): what produces a coefficient is musig_key_list / musig_coef / musig_nonce_coef; what follows
// it is musig_term / musig_key_agg_finish / musig_finish_tweak / musig_session_finish, which a test drives with
// coefficients no hash will ever produce.
//
// Registers.  The GLV walk of k_point_mul takes 231 VGPRs by itself, and two waves per SIMD end at 256.  What a body must keep
// ACROSS a walk -- the running sum and the list hash of the key aggregation, R_1, x(Q) and msg of the session, s, R_s1, P, the
// key factor and then -Re of the verification -- would push these kernels beyond that and halve their occupancy.  Such values
// are PARKED for the walk: canonical 8-word values written to a per-lane column of LDS before it and read back behind it
// (MusigParkLds; the CPU build parks in a plain array, MusigParkHost, and runs the same text).  Nothing secret is parked: the
// signer has no general-point walk.
//
// One lane per element.  The signer's secrets (k_1, k_2, d', d, the products) live in registers only; the one thing stored
// that derives from them is the partial signature.  Every body reads all inputs of element i before its first store.
#pragma once
#include "taproot.hpp"
#include "sp.hpp"
#include "point_arith.hpp"

namespace p2e {

typedef Secp256k1 MusigCV;
constexpr int MUSIG_TAG_LIST = 0, MUSIG_TAG_COEF = 1, MUSIG_TAG_NONCECOEF = 2;
constexpr size_t MUSIG_MAX_SIGNERS = 1024;                                           // include/p2e.h P2E_MUSIG_MAX_SIGNERS
constexpr int MUSIG_TWEAK_PLAIN = 0, MUSIG_TWEAK_XONLY = 1, MUSIG_TWEAK_TAPROOT = 2;   // include/p2e.h P2E_MUSIG_TWEAK_*
constexpr u32 MUSIG_KA_GACC_NEG = 1u, MUSIG_KA_HAVE_PK2 = 2u, MUSIG_KA_PK2_ODD = 4u;   // the flags of keyagg192
constexpr u32 MUSIG_SES_R_ODD = 1u;                                                    // the flags of session128
constexpr size_t MUSIG_KEYAGG_BYTES = 192, MUSIG_SESSION_BYTES = 128, MUSIG_NONCE_BYTES = 128;

// the chaining value after the block SHA256(tag) || SHA256(tag), tag = "KeyAgg list", "KeyAgg coefficient", "MuSig/noncecoef"
P2E_HD Sha256State musig_midstate(int tag) {
    Sha256State s;
    if (tag == MUSIG_TAG_LIST) {
        s.h[0] = 0xb399d5e0u, s.h[1] = 0xc8fff302u, s.h[2] = 0x6badac71u, s.h[3] = 0x07c5b7f1u;
        s.h[4] = 0x9701e2efu, s.h[5] = 0x2a72ecf8u, s.h[6] = 0x201a4c7bu, s.h[7] = 0xab148a38u;
    } else if (tag == MUSIG_TAG_COEF) {
        s.h[0] = 0x6ef02c5au, s.h[1] = 0x06a480deu, s.h[2] = 0x1f298665u, s.h[3] = 0x1d1134f2u;
        s.h[4] = 0x56a0b063u, s.h[5] = 0x52da4147u, s.h[6] = 0xf280d9d4u, s.h[7] = 0x4484be15u;
    } else {
        s.h[0] = 0x2c7d5a45u, s.h[1] = 0x06bf7e53u, s.h[2] = 0x89be68a6u, s.h[3] = 0x971254c0u;
        s.h[4] = 0x60ac12d2u, s.h[5] = 0x72846dcdu, s.h[6] = 0x6c81212fu, s.h[7] = 0xde7a2500u;
    }
    return s;
}

// ---------------------------------------------------------------------------------------------------------------------
// a SHA-256 byte stream behind a midstate, fed in pieces that are no multiple of four bytes
// ---------------------------------------------------------------------------------------------------------------------
struct MusigStream {
    Sha256State st;
    Sha256Block blk;
    u32 acc;    // the `fill` bytes held back, on top of the word, zeros below
    u32 fill;   // 0 .. 3
    u32 wi;     // the block's next word, 0 .. 15
};
P2E_HD MusigStream musig_stream(const Sha256State& start) {
    MusigStream s;
    s.st = start;
    P2E_UNROLL
    for (int j = 0; j < 16; j++) s.blk.w[j] = 0;
    s.acc = s.fill = s.wi = 0;
    return s;
}
// one whole word of the stream; the block is compressed when it is full
P2E_HD void musig_emit(MusigStream& s, u32 word) {
    P2E_UNROLL
    for (int j = 0; j < 16; j++) s.blk.w[j] = (u32)j == s.wi ? word : s.blk.w[j];   // (a register select: no indexed store)
    if (++s.wi == 16) {
        s.st = sha256_compress_call(s.st, s.blk);
        s.wi = 0;
    }
}
// `nb` (1 or 4) bytes, on top of w with zeros below
P2E_HD void musig_push(MusigStream& s, u32 w, u32 nb) {
    const u32 sh = 8 * s.fill;
    const u32 joined = s.acc | hash_join(w, 0, sh);   // w moved down behind the bytes held back
    if (s.fill + nb >= 4) {
        musig_emit(s, joined);
        s.acc = hash_join(0, w, sh);                  // the bytes of w that did not fit, moved to the top
        s.fill = s.fill + nb - 4;
    } else {
        s.acc = joined;
        s.fill += nb;
    }
}
// cbytes(P) = (02 | odd) || bytes(x); cbytes_ext of the point at infinity is 33 zero bytes
P2E_HD void musig_push_point(MusigStream& s, const U256& x, u32 odd, bool neutral) {
    P2E_UNROLL
    for (int j = 0; j < 9; j++) musig_push(s, neutral ? 0u : sp_serp_word(x, odd, j), j == 8 ? 1u : 4u);
}
P2E_HD void musig_push_be(MusigStream& s, const U256& v) {
    P2E_UNROLL
    for (int j = 0; j < 8; j++) musig_push(s, v.w[7 - j], 4);
}
// the padding and the length of a stream of `len` bytes behind the 64-byte tag block
P2E_HD Sha256State musig_finish(MusigStream& s, u64 len) {
    musig_push(s, 0x80000000u, 1);
    if (s.fill) musig_emit(s, s.acc);
    while (s.wi != 14) musig_emit(s, 0u);   // (at most 17 words)
    const u64 bits = 8 * (64 + len);
    musig_emit(s, (u32)(bits >> 32));
    musig_emit(s, (u32)bits);               // fills the block: compressed
    return s.st;
}

// ---------------------------------------------------------------------------------------------------------------------
// the records (include/p2e.h) in registers
// ---------------------------------------------------------------------------------------------------------------------
struct MusigKeyAgg {
    Aff Q;
    U256 tacc;    // < n
    Words8 L;     // the hash of the key list
    U256 pk2x;    // x of the second key (0 where there is none)
    u32 flags;    // MUSIG_KA_*
};
struct MusigSession {
    U256 b, e, rx;
    u32 flags;    // MUSIG_SES_*
};
P2E_HD MusigKeyAgg musig_load_keyagg(const uint8_t* keyagg192, size_t i) {
    const uint8_t* p = keyagg192 + MUSIG_KEYAGG_BYTES * i;
    MusigKeyAgg r;
    r.Q.x = load_packed(p, 0), r.Q.y = load_packed(p, 1);
    r.tacc = schnorr_load_be(p + 64);
    r.L = hd_load_cc(p, 3);
    r.pk2x = schnorr_load_be(p + 128);
    r.flags = *reinterpret_cast<const u32*>(p + 160);
    return r;
}
// the point (WIRE_INFINITY for (0, 0): a zeroed record), then tacc >= n: WIRE_SCALAR_RANGE, x(pk2) >= p: WIRE_COORD_RANGE,
// an unknown flag bit: WIRE_BAD_PREFIX
P2E_HD uint8_t musig_check_keyagg(const MusigKeyAgg& r) {
    uint8_t e = sp_point_check(r.Q);
    if (!e && geq_mod<MusigCV::Fn>(r.tacc.w)) e = WIRE_SCALAR_RANGE;
    if (!e && geq_mod<MusigCV::Fp>(r.pk2x.w)) e = WIRE_COORD_RANGE;
    if (!e && (r.flags & ~7u)) e = WIRE_BAD_PREFIX;
    return e;
}
P2E_HD void musig_store_keyagg(uint8_t* keyagg192, size_t i, const MusigKeyAgg& r, bool zero) {
    uint8_t* p = keyagg192 + MUSIG_KEYAGG_BYTES * i;
    hd_store_key(p, 0, r.Q.x, zero);
    hd_store_key(p, 1, r.Q.y, zero);
    schnorr_store_be(p + 64, zero ? u256_zero() : r.tacc);
    hd_store_cc(p, 3, r.L, zero);
    schnorr_store_be(p + 128, zero ? u256_zero() : r.pk2x);
    u32* q = reinterpret_cast<u32*>(p + 160);
    q[0] = zero ? 0u : r.flags;
    P2E_UNROLL
    for (int j = 1; j < 8; j++) q[j] = 0u;
}
P2E_HD MusigSession musig_load_session(const uint8_t* session128, size_t i) {
    const uint8_t* p = session128 + MUSIG_SESSION_BYTES * i;
    MusigSession r;
    r.b = schnorr_load_be(p), r.e = schnorr_load_be(p + 32), r.rx = schnorr_load_be(p + 64);
    r.flags = *reinterpret_cast<const u32*>(p + 96);
    return r;
}
// b or e >= n: WIRE_SCALAR_RANGE; x(R) = 0 (a zeroed record; no point has it): WIRE_INFINITY; x(R) >= p: WIRE_COORD_RANGE; an
// unknown flag bit: WIRE_BAD_PREFIX
P2E_HD uint8_t musig_check_session(const MusigSession& r) {
    if (geq_mod<MusigCV::Fn>(r.b.w) || geq_mod<MusigCV::Fn>(r.e.w)) return WIRE_SCALAR_RANGE;
    if (u256_is_zero(r.rx)) return WIRE_INFINITY;
    if (geq_mod<MusigCV::Fp>(r.rx.w)) return WIRE_COORD_RANGE;
    return (r.flags & ~1u) ? WIRE_BAD_PREFIX : WIRE_OK;
}
P2E_HD void musig_store_session(uint8_t* session128, size_t i, const MusigSession& r, bool zero) {
    uint8_t* p = session128 + MUSIG_SESSION_BYTES * i;
    schnorr_store_be(p, zero ? u256_zero() : r.b);
    schnorr_store_be(p + 32, zero ? u256_zero() : r.e);
    schnorr_store_be(p + 64, zero ? u256_zero() : r.rx);
    u32* q = reinterpret_cast<u32*>(p + 96);
    q[0] = zero ? 0u : r.flags;
    P2E_UNROLL
    for (int j = 1; j < 8; j++) q[j] = 0u;
}
P2E_HD Aff musig_load_point(const uint8_t* px32, const uint8_t* py32, size_t j) {
    Aff P;
    P.x = load_packed(px32, j), P.y = load_packed(py32, j);
    return P;
}
// half `h` (0, 1) of nonce j of an array of 128-byte nonces
P2E_HD Aff musig_load_nonce(const uint8_t* nonce128, size_t j, int h) {
    Aff P;
    P.x = load_packed(nonce128, 4 * j + 2 * h), P.y = load_packed(nonce128, 4 * j + 2 * h + 1);
    return P;
}
P2E_HD SignSum<MusigCV> musig_from_aff(const Aff& P, bool have) {
    SignSum<MusigCV> s;
    s.p = SignArith<MusigCV>::from_aff(P);
    s.have = have;
    return s;
}
P2E_HD SignSum<MusigCV> musig_negate(SignSum<MusigCV> s, bool neg) {
    typedef RecField<MusigCV> FA;
    SignSum<MusigCV> m = s;
    m.p.Y = FA::sub(FA::from(u256_zero()), s.p.Y);
    s.p = SignArith<MusigCV>::select(neg, m.p, s.p);
    return s;
}
// g = n - 1 where `neg`: v -> g v mod n
P2E_HD U256 musig_signed(const U256& v, bool neg) { return u256_select(neg, fe_neg<MusigCV::Fn>(v), v); }

// ---------------------------------------------------------------------------------------------------------------------
// parking (see the header): slot k is 8 words; a sum takes three slots (canonical X, Y, Z) and the word MUSIG_PARK_HAVE
// ---------------------------------------------------------------------------------------------------------------------
constexpr int MUSIG_PARK_SLOTS = 6, MUSIG_PARK_HAVE = 8 * MUSIG_PARK_SLOTS, MUSIG_PARK_WORDS = MUSIG_PARK_HAVE + 1;
struct MusigParkHost {
    u32 w[MUSIG_PARK_WORDS];
    P2E_HD u32& at(int k) { return w[k]; }
};
#if defined(__HIPCC__)
struct MusigParkLds {
    u32* col;   // this lane's column of a [MUSIG_PARK_WORDS][256] array: word k of every lane side by side
    __device__ __forceinline__ u32& at(int k) { return col[256 * k]; }
};
#endif
template <class PARK>
P2E_HD void musig_park(PARK& park, int slot, const U256& v) {
    P2E_UNROLL
    for (int j = 0; j < 8; j++) park.at(8 * slot + j) = v.w[j];
}
template <class PARK>
P2E_HD U256 musig_unpark(PARK& park, int slot) {
    U256 v;
    P2E_UNROLL
    for (int j = 0; j < 8; j++) v.w[j] = park.at(8 * slot + j);
    return v;
}
template <class PARK>
P2E_HD void musig_park_words(PARK& park, int slot, const Words8& v) {
    P2E_UNROLL
    for (int j = 0; j < 8; j++) park.at(8 * slot + j) = v.w[j];
}
template <class PARK>
P2E_HD Words8 musig_unpark_words(PARK& park, int slot) {
    Words8 v;
    P2E_UNROLL
    for (int j = 0; j < 8; j++) v.w[j] = park.at(8 * slot + j);
    return v;
}
template <class PARK>
P2E_HD void musig_park_sum(PARK& park, int slot, const SignSum<MusigCV>& s) {
    typedef RecField<MusigCV> FA;
    musig_park(park, slot, FA::canon(s.p.X));
    musig_park(park, slot + 1, FA::canon(s.p.Y));
    musig_park(park, slot + 2, FA::canon(s.p.Z));
    park.at(MUSIG_PARK_HAVE) = s.have ? 1u : 0u;
}
template <class PARK>
P2E_HD SignSum<MusigCV> musig_unpark_sum(PARK& park, int slot) {
    typedef RecField<MusigCV> FA;
    SignSum<MusigCV> s;
    s.p.X = FA::from(musig_unpark(park, slot));
    s.p.Y = FA::from(musig_unpark(park, slot + 1));
    s.p.Z = FA::from(musig_unpark(park, slot + 2));
    s.have = park.at(MUSIG_PARK_HAVE) != 0;
    return s;
}

// ---------------------------------------------------------------------------------------------------------------------
// the hashes
// ---------------------------------------------------------------------------------------------------------------------
// Pass 1 over the keys [lo, lo + u) of a session: every key checked (the first failing one gives the code), L =
// H_list(cbytes(pk_1) || ..), and the second key: the first one whose cbytes differ from pk_1's.
P2E_HD uint8_t musig_key_list(const uint8_t* pkx32, const uint8_t* pky32, u64 lo, u32 u, MusigKeyAgg& r) {
    MusigStream s = musig_stream(musig_midstate(MUSIG_TAG_LIST));
    U256 x1 = u256_zero();
    u32 odd1 = 0;
    r.pk2x = u256_zero();
    r.flags = 0;
    for (u32 j = 0; j < u; j++) {
        const Aff P = musig_load_point(pkx32, pky32, (size_t)(lo + j));
        const uint8_t e = sp_point_check(P);
        if (e) return e;
        const u32 odd = P.y.w[0] & 1u;
        if (j == 0) x1 = P.x, odd1 = odd;
        if (!(r.flags & MUSIG_KA_HAVE_PK2) && (!u256_eq(P.x, x1) || odd != odd1)) {
            r.pk2x = P.x;
            r.flags = MUSIG_KA_HAVE_PK2 | (odd ? MUSIG_KA_PK2_ODD : 0u);
        }
        musig_push_point(s, P.x, odd, false);
    }
    r.L = hd_digest_words(musig_finish(s, 33 * (u64)u));
    return WIRE_OK;
}
// the coefficient of the key (x, parity odd): 1 for the second key, else int(H_coef(L || cbytes(pk))) mod n
P2E_HD U256 musig_coef(const MusigKeyAgg& r, const U256& x, u32 odd) {
    if ((r.flags & MUSIG_KA_HAVE_PK2) && u256_eq(x, r.pk2x) && odd == ((r.flags & MUSIG_KA_PK2_ODD) ? 1u : 0u)) return u256_small(1);
    Sha256Block blk;
    P2E_UNROLL
    for (int j = 0; j < 8; j++) blk.w[j] = r.L.w[j], blk.w[8 + j] = sp_serp_word(x, odd, j);
    const Sha256State s = sha256_compress_call(musig_midstate(MUSIG_TAG_COEF), blk);
    blk.w[0] = sp_serp_word(x, odd, 8) | 0x00800000u;
    sha256_finish_block(blk, 1, 8 * (64 + 65));
    return fe_canon<MusigCV::Fn>(schnorr_digest_int(sha256_compress_call(s, blk)));
}
// b = int(H_noncecoef(cbytes_ext(R_1) || cbytes_ext(R_2) || xbytes(Q) || msg)) mod n: 130 bytes, three compressions
P2E_HD U256 musig_nonce_coef(const Aff& R1, bool n1, const Aff& R2, bool n2, const U256& qx, const U256& msg) {
    MusigStream s = musig_stream(musig_midstate(MUSIG_TAG_NONCECOEF));
    musig_push_point(s, R1.x, R1.y.w[0] & 1u, n1);
    musig_push_point(s, R2.x, R2.y.w[0] & 1u, n2);
    musig_push_be(s, qx);
    musig_push_be(s, msg);
    return fe_canon<MusigCV::Fn>(schnorr_digest_int(musig_finish(s, 130)));
}

// ---------------------------------------------------------------------------------------------------------------------
// behind the hashes: arithmetic that a test can drive with any coefficient
// ---------------------------------------------------------------------------------------------------------------------
// a P for a checked P that is not neutral and a < n (a = 1: no walk; a = 0: the neutral element)
P2E_HD SignSum<MusigCV> musig_term(const Aff& P, const U256& a) {
    SignSum<MusigCV> W = musig_from_aff(P, true);
    if (!u256_eq(a, u256_small(1))) W = point_var_mul<MusigCV, MUL_PLAN_GLV>(P, false, a);
    return W;
}
// Q = the sum: WIRE_INFINITY where it is neutral; gacc = 1, tacc = 0
P2E_HD uint8_t musig_key_agg_finish(const SignSum<MusigCV>& sum, MusigKeyAgg& r) {
    if (!sum.have || !sign_to_affine<MusigCV, true>(sum, r.Q.x, r.Q.y)) return WIRE_INFINITY;   // (a zero Z under `have` cannot occur)
    r.tacc = u256_zero();
    return WIRE_OK;
}
// ApplyTweak behind t.  t >= n: WIRE_SCALAR_RANGE; Q' neutral: WIRE_INFINITY.
P2E_HD uint8_t musig_finish_tweak(const Aff* T, const MusigKeyAgg& in, const U256& t, bool xonly, MusigKeyAgg& out) {
    const bool neg = xonly && (in.Q.y.w[0] & 1u);
    Aff P = in.Q;
    P.y = u256_select(neg, fe_neg<MusigCV::Fp>(in.Q.y), in.Q.y);
    out = in;
    const uint8_t e = bip32_finish_pub(T, t, P, out.Q);   // (the same sum: t G + g Q, with the same codes)
    if (e) return e;
    out.flags = in.flags ^ (neg ? MUSIG_KA_GACC_NEG : 0u);
    out.tacc = fe_add<MusigCV::Fn>(t, musig_signed(in.tacc, neg));
    return WIRE_OK;
}
// the session behind b: R' = R_1 + b R_2, R = G where R' is neutral, e the BIP-340 challenge
template <class PARK>
P2E_HD uint8_t musig_session_finish(PARK& park, const Aff* T, const U256& qx_, const Aff& R1_, bool n1, const Aff& R2, bool n2, const U256& b,
                                    const U256& msg_, MusigSession& r) {
    musig_park(park, 0, R1_.x), musig_park(park, 1, R1_.y), musig_park(park, 2, qx_), musig_park(park, 3, msg_);
    musig_park(park, 4, b);
    const SignSum<MusigCV> bR2 = point_var_mul<MusigCV, MUL_PLAN_GLV>(R2, n2, b);
    Aff R1;
    R1.x = musig_unpark(park, 0), R1.y = musig_unpark(park, 1);
    const U256 qx = musig_unpark(park, 2), msg = musig_unpark(park, 3);
    SignSum<MusigCV> R = msm_add<MusigCV, true>(bR2, musig_from_aff(R1, !n1));
    if (!R.have) R = musig_from_aff(T[1], true);   // (T[1] = 1 * 16^0 G: the first entry of the generator's table)
    U256 ry;
    if (!sign_to_affine<MusigCV, true>(R, r.rx, ry)) return WIRE_INFINITY;   // (a zero Z under `have` cannot occur)
    r.b = musig_unpark(park, 4);
    r.e = schnorr_challenge(r.rx, qx, msg);
    r.flags = (ry.w[0] & 1u) ? MUSIG_SES_R_ODD : 0u;
    return WIRE_OK;
}
// e a g gacc mod n: the factor of the signer's key in a partial signature (g from the parity of y(Q))
P2E_HD U256 musig_key_factor(const MusigKeyAgg& ka, const MusigSession& ses, const U256& a) {
    const bool neg = ((ka.Q.y.w[0] & 1u) != 0) != ((ka.flags & MUSIG_KA_GACC_NEG) != 0);
    return musig_signed(fe_mul<MusigCV::Fn>(ses.e, a), neg);
}
// s G == Re + c P  <=>  s G + (n - c) P - Re is neutral, Re = +-(R_s1 + b R_s2): no inversion
template <class PARK>
P2E_HD bool musig_partial_holds(PARK& park, const Aff* T, const U256& s_, const Aff& Rs1_, const Aff& Rs2, const Aff& P_, const U256& b,
                                bool r_odd, const U256& c_) {
    musig_park(park, 0, Rs1_.x), musig_park(park, 1, Rs1_.y), musig_park(park, 2, P_.x), musig_park(park, 3, P_.y);
    musig_park(park, 4, fe_neg<MusigCV::Fn>(c_)), musig_park(park, 5, s_);
    const SignSum<MusigCV> bR2 = point_var_mul<MusigCV, MUL_PLAN_GLV>(Rs2, false, b);
    Aff Rs1, P;
    Rs1.x = musig_unpark(park, 0), Rs1.y = musig_unpark(park, 1), P.x = musig_unpark(park, 2), P.y = musig_unpark(park, 3);
    const U256 minus_c = musig_unpark(park, 4);
    const SignSum<MusigCV> Re = msm_add<MusigCV, true>(bR2, musig_from_aff(Rs1, true));
    musig_park_sum(park, 0, musig_negate(Re, !r_odd));   // (slots 0 .. 2: R_s1 and x(P) are done with)
    const SignSum<MusigCV> cP = point_var_mul<MusigCV, MUL_PLAN_GLV>(P, false, minus_c);
    const SignSum<MusigCV> rest = msm_add<MusigCV, false>(cP, musig_unpark_sum(park, 0));
    const SignSum<MusigCV> sG = sign_base_mul<MusigCV, SIGN_PLAN_LANE>(T, musig_unpark(park, 5), 0);
    return !msm_add<MusigCV, false>(sG, rest).have;
}

// ---- call 1: KeyAgg of session i's keys ------------------------------------------------------------------------------------------
template <class PARK>
P2E_HD uint8_t body_musig_key_agg(PARK& park, const uint8_t* pkx32, const uint8_t* pky32, const uint64_t* key_offsets, uint8_t* keyagg192,
                                  uint8_t* agg_pk32, size_t i) {
    const u64 lo = key_offsets[i], hi = key_offsets[i + 1];
    MusigKeyAgg r;
    r.Q.x = r.Q.y = r.tacc = r.pk2x = u256_zero();
    r.L = taproot_zero_words();
    r.flags = 0;
    uint8_t e = (hi <= lo || hi - lo > MUSIG_MAX_SIGNERS) ? WIRE_BAD_LENGTH : WIRE_OK;
    const u32 u = e ? 0u : (u32)(hi - lo);
    if (!e) e = musig_key_list(pkx32, pky32, lo, u, r);
    if (!e) {
        musig_park_sum(park, 0, msm_neutral<MusigCV>());
        musig_park_words(park, 3, r.L), musig_park(park, 4, r.pk2x);
        park.at(MUSIG_PARK_HAVE - 1) = r.flags;   // (the last word of slot 5, which this body does not use)
        for (u32 j = 0; j < u; j++) {
            const Aff P = musig_load_point(pkx32, pky32, (size_t)(lo + j));
            MusigKeyAgg h;   // what the coefficient needs of the record; dead before the walk
            h.L = musig_unpark_words(park, 3), h.pk2x = musig_unpark(park, 4), h.flags = park.at(MUSIG_PARK_HAVE - 1);
            const SignSum<MusigCV> W = musig_term(P, musig_coef(h, P.x, P.y.w[0] & 1u));
            musig_park_sum(park, 0, msm_add<MusigCV, false>(musig_unpark_sum(park, 0), W));
        }
        r.L = musig_unpark_words(park, 3), r.pk2x = musig_unpark(park, 4), r.flags = park.at(MUSIG_PARK_HAVE - 1);
        e = musig_key_agg_finish(musig_unpark_sum(park, 0), r);
    }
    musig_store_keyagg(keyagg192, i, r, e != 0);
    schnorr_store_be(agg_pk32 + 32 * i, e ? u256_zero() : r.Q.x);
    return e;
}

// ---- call 2: ApplyTweak (tweak32 nullable in mode 2: no root) ---------------------------------------------------------------------
// (include/p2e.h BUFFER OVERLAP relies on this body reading every input of element i before its first store)
P2E_HD uint8_t body_musig_apply_tweak(const Aff* T, const uint8_t* keyagg192_in, const uint8_t* tweak32, int mode, uint8_t* keyagg192_out,
                                      uint8_t* agg_pk32, size_t i) {
    const MusigKeyAgg in = musig_load_keyagg(keyagg192_in, i);
    const U256 tw = tweak32 ? schnorr_load_be(tweak32 + 32 * i) : u256_zero();
    const Words8 root = tweak32 ? hd_load_cc(tweak32, i) : taproot_zero_words();
    MusigKeyAgg out = in;
    uint8_t e = musig_check_keyagg(in);
    if (!e) {
        const U256 t = mode == MUSIG_TWEAK_TAPROOT ? taproot_tweak(in.Q.x, tweak32 != nullptr, root) : tw;
        e = musig_finish_tweak(T, in, t, mode != MUSIG_TWEAK_PLAIN, out);
    }
    musig_store_keyagg(keyagg192_out, i, out, e != 0);
    schnorr_store_be(agg_pk32 + 32 * i, e ? u256_zero() : out.Q.x);
    return e;
}

// ---- call 3: NonceAgg of session i's public nonces ---------------------------------------------------------------------------------
P2E_HD uint8_t body_musig_nonce_agg(const uint8_t* pubnonce128, const uint64_t* key_offsets, uint8_t* aggnonce128, size_t i) {
    const u64 lo = key_offsets[i], hi = key_offsets[i + 1];
    uint8_t e = (hi <= lo || hi - lo > MUSIG_MAX_SIGNERS) ? WIRE_BAD_LENGTH : WIRE_OK;
    const u32 u = e ? 0u : (u32)(hi - lo);
    SignSum<MusigCV> s1 = msm_neutral<MusigCV>(), s2 = msm_neutral<MusigCV>();
    for (u32 j = 0; j < u && !e; j++) {
        const Aff R1 = musig_load_nonce(pubnonce128, (size_t)(lo + j), 0), R2 = musig_load_nonce(pubnonce128, (size_t)(lo + j), 1);
        e = sp_point_check(R1);
        if (!e) e = sp_point_check(R2);
        if (e) break;
        s1 = msm_add<MusigCV, true>(s1, musig_from_aff(R1, true));
        s2 = msm_add<MusigCV, true>(s2, musig_from_aff(R2, true));
    }
    U256 x1 = u256_zero(), y1 = u256_zero(), x2 = u256_zero(), y2 = u256_zero();
    if (!e && s1.have && !sign_to_affine<MusigCV, true>(s1, x1, y1)) e = WIRE_INFINITY;   // (a zero Z under `have` cannot occur)
    if (!e && s2.have && !sign_to_affine<MusigCV, true>(s2, x2, y2)) e = WIRE_INFINITY;
    hd_store_key(aggnonce128, 4 * i + 0, x1, e != 0);
    hd_store_key(aggnonce128, 4 * i + 1, y1, e != 0);
    hd_store_key(aggnonce128, 4 * i + 2, x2, e != 0);
    hd_store_key(aggnonce128, 4 * i + 3, y2, e != 0);
    return e;
}

// ---- call 4: the session values b, e, R ---------------------------------------------------------------------------------------------
template <class PARK>
P2E_HD uint8_t body_musig_session(PARK& park, const Aff* T, const uint8_t* keyagg192, const uint8_t* aggnonce128, const uint8_t* msg32,
                                  uint8_t* session128, size_t i) {
    const MusigKeyAgg ka = musig_load_keyagg(keyagg192, i);
    const Aff R1 = musig_load_nonce(aggnonce128, i, 0), R2 = musig_load_nonce(aggnonce128, i, 1);
    const U256 msg = schnorr_load_be(msg32 + 32 * i);
    bool n1 = false, n2 = false;
    uint8_t e = musig_check_keyagg(ka);
    if (!e) e = point_check<MusigCV>(R1.x, R1.y, n1);
    if (!e) e = point_check<MusigCV>(R2.x, R2.y, n2);
    MusigSession r;
    r.b = r.e = r.rx = u256_zero();
    r.flags = 0;
    if (!e) e = musig_session_finish(park, T, ka.Q.x, R1, n1, R2, n2, musig_nonce_coef(R1, n1, R2, n2, ka.Q.x, msg), msg, r);
    musig_store_session(session128, i, r, e != 0);
    return e;
}

// ---- call 5: the caller's partial signature in session i --------------------------------------------------------------------------
P2E_HD uint8_t body_musig_partial_sign(const Aff* T, const uint8_t* secnonce64, const uint8_t* sk32, const uint8_t* keyagg192,
                                       const uint8_t* session128, uint8_t* psig32, size_t i) {
    typedef MusigCV::Fn Fn;
    const U256 k1 = load_packed(secnonce64, 2 * i), k2 = load_packed(secnonce64, 2 * i + 1), d0 = load_packed(sk32, i);
    const MusigKeyAgg ka = musig_load_keyagg(keyagg192, i);
    const MusigSession ses = musig_load_session(session128, i);
    uint8_t e = sp_scalar_check(k1);
    if (!e) e = sp_scalar_check(k2);
    if (!e) e = sp_scalar_check(d0);
    if (!e) e = musig_check_keyagg(ka);
    if (!e) e = musig_check_session(ses);
    U256 s = u256_zero(), px, py;
    if (!e && !schnorr_base_mul(T, d0, px, py)) e = WIRE_INFINITY;   // (it cannot: 0 < d' < n)
    if (!e) {
        const bool r_odd = (ses.flags & MUSIG_SES_R_ODD) != 0;
        const U256 c = musig_key_factor(ka, ses, musig_coef(ka, px, py.w[0] & 1u));
        s = fe_add<Fn>(fe_add<Fn>(musig_signed(k1, r_odd), fe_mul<Fn>(ses.b, musig_signed(k2, r_odd))), fe_mul<Fn>(c, d0));
    }
    schnorr_store_be(psig32 + 32 * i, e ? u256_zero() : s);
    return e;
}

// ---- call 6: PartialSigVerify of partial signature i in session session_index[i] (null: i) -----------------------------------------------
// (valid[i] is this body's only store and comes last)
template <class PARK>
P2E_HD uint8_t body_musig_partial_verify(PARK& park, const Aff* T, const uint8_t* psig32, const uint8_t* pubnonce128, const uint8_t* pkx32,
                                         const uint8_t* pky32, const uint32_t* session_index, const uint8_t* keyagg192,
                                         const uint8_t* session128, size_t n_sessions, uint8_t* valid, size_t i) {
    const size_t at = session_index ? (size_t)session_index[i] : i;
    uint8_t e = at >= n_sessions ? WIRE_BAD_INDEX : WIRE_OK;
    bool ok = false;
    if (!e) {
        const U256 s = schnorr_load_be(psig32 + 32 * i);
        const Aff Rs1 = musig_load_nonce(pubnonce128, i, 0), Rs2 = musig_load_nonce(pubnonce128, i, 1);
        const Aff P = musig_load_point(pkx32, pky32, i);
        const MusigKeyAgg ka = musig_load_keyagg(keyagg192, at);
        const MusigSession ses = musig_load_session(session128, at);
        if (geq_mod<MusigCV::Fn>(s.w)) e = WIRE_SCALAR_RANGE;
        if (!e) e = sp_point_check(Rs1);
        if (!e) e = sp_point_check(Rs2);
        if (!e) e = sp_point_check(P);
        if (!e) e = musig_check_keyagg(ka);
        if (!e) e = musig_check_session(ses);
        if (!e)
            ok = musig_partial_holds(park, T, s, Rs1, Rs2, P, ses.b, (ses.flags & MUSIG_SES_R_ODD) != 0,
                                     musig_key_factor(ka, ses, musig_coef(ka, P.x, P.y.w[0] & 1u)));
    }
    valid[i] = ok ? 1 : 0;
    return e;
}

// ---- call 7: PartialSigAgg of session i's partial signatures -------------------------------------------------------------------------
P2E_HD uint8_t body_musig_sig_agg(const uint8_t* psig32, const uint64_t* key_offsets, const uint8_t* keyagg192, const uint8_t* session128,
                                  uint8_t* sig64, size_t i) {
    typedef MusigCV::Fn Fn;
    const u64 lo = key_offsets[i], hi = key_offsets[i + 1];
    const MusigKeyAgg ka = musig_load_keyagg(keyagg192, i);
    const MusigSession ses = musig_load_session(session128, i);
    uint8_t e = (hi <= lo || hi - lo > MUSIG_MAX_SIGNERS) ? WIRE_BAD_LENGTH : WIRE_OK;
    if (!e) e = musig_check_keyagg(ka);
    if (!e) e = musig_check_session(ses);
    const u32 u = e ? 0u : (u32)(hi - lo);
    U256 s = u256_zero();
    for (u32 j = 0; j < u; j++) {
        const U256 v = schnorr_load_be(psig32 + 32 * (size_t)(lo + j));
        if (geq_mod<Fn>(v.w)) {
            e = WIRE_SCALAR_RANGE;
            break;
        }
        s = fe_add<Fn>(s, v);
    }
    if (!e) s = fe_add<Fn>(s, musig_signed(fe_mul<Fn>(ses.e, ka.tacc), (ka.Q.y.w[0] & 1u) != 0));
    schnorr_store_be(sig64 + 64 * i, e ? u256_zero() : ses.rx);
    schnorr_store_be(sig64 + 64 * i + 32, e ? u256_zero() : s);
    return e;
}

#if defined(__HIPCC__)
// thread g owns element g
template <int UNUSED = 0>   // (templates so that every translation unit that includes this file may hold the definitions)
__global__ __launch_bounds__(256) void k_musig_key_agg(const uint8_t* pkx32, const uint8_t* pky32, const uint64_t* key_offsets,
                                                       uint8_t* keyagg192, uint8_t* agg_pk32, size_t count, uint8_t* err,
                                                       unsigned long long* counter) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    uint8_t e = 0;
    __shared__ u32 lds[MUSIG_PARK_WORDS][256];
    MusigParkLds park{&lds[0][threadIdx.x]};
    if (i < count) {
        e = body_musig_key_agg(park, pkx32, pky32, key_offsets, keyagg192, agg_pk32, i);
        err[i] = e;
    }
    sign_count_err(e, counter);
}
template <int UNUSED = 0>
__global__ __launch_bounds__(256) void k_musig_apply_tweak(const Aff* T, const uint8_t* keyagg192_in, const uint8_t* tweak32, int mode,
                                                           uint8_t* keyagg192_out, uint8_t* agg_pk32, size_t count, uint8_t* err,
                                                           unsigned long long* counter) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    uint8_t e = 0;
    if (i < count) {
        e = body_musig_apply_tweak(T, keyagg192_in, tweak32, mode, keyagg192_out, agg_pk32, i);
        err[i] = e;
    }
    sign_count_err(e, counter);
}
template <int UNUSED = 0>
__global__ __launch_bounds__(256) void k_musig_nonce_agg(const uint8_t* pubnonce128, const uint64_t* key_offsets, uint8_t* aggnonce128,
                                                         size_t count, uint8_t* err, unsigned long long* counter) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    uint8_t e = 0;
    if (i < count) {
        e = body_musig_nonce_agg(pubnonce128, key_offsets, aggnonce128, i);
        err[i] = e;
    }
    sign_count_err(e, counter);
}
template <int UNUSED = 0>
__global__ __launch_bounds__(256) void k_musig_session(const Aff* T, const uint8_t* keyagg192, const uint8_t* aggnonce128,
                                                       const uint8_t* msg32, uint8_t* session128, size_t count, uint8_t* err,
                                                       unsigned long long* counter) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    uint8_t e = 0;
    __shared__ u32 lds[MUSIG_PARK_WORDS][256];
    MusigParkLds park{&lds[0][threadIdx.x]};
    if (i < count) {
        e = body_musig_session(park, T, keyagg192, aggnonce128, msg32, session128, i);
        err[i] = e;
    }
    sign_count_err(e, counter);
}
template <int UNUSED = 0>
__global__ __launch_bounds__(256) void k_musig_partial_sign(const Aff* T, const uint8_t* secnonce64, const uint8_t* sk32,
                                                            const uint8_t* keyagg192, const uint8_t* session128, uint8_t* psig32,
                                                            size_t count, uint8_t* err, unsigned long long* counter) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    uint8_t e = 0;
    if (i < count) {
        e = body_musig_partial_sign(T, secnonce64, sk32, keyagg192, session128, psig32, i);
        err[i] = e;
    }
    sign_count_err(e, counter);
}
template <int UNUSED = 0>
__global__ __launch_bounds__(256) void k_musig_partial_verify(const Aff* T, const uint8_t* psig32, const uint8_t* pubnonce128,
                                                              const uint8_t* pkx32, const uint8_t* pky32, const uint32_t* session_index,
                                                              const uint8_t* keyagg192, const uint8_t* session128, size_t n_sessions,
                                                              size_t count, uint8_t* err, uint8_t* valid, unsigned long long* counter) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    uint8_t e = 0;
    __shared__ u32 lds[MUSIG_PARK_WORDS][256];
    MusigParkLds park{&lds[0][threadIdx.x]};
    if (i < count) {
        e = body_musig_partial_verify(park, T, psig32, pubnonce128, pkx32, pky32, session_index, keyagg192, session128, n_sessions, valid, i);
        err[i] = e;
    }
    sign_count_err(e, counter);
}
template <int UNUSED = 0>
__global__ __launch_bounds__(256) void k_musig_sig_agg(const uint8_t* psig32, const uint64_t* key_offsets, const uint8_t* keyagg192,
                                                       const uint8_t* session128, uint8_t* sig64, size_t count, uint8_t* err,
                                                       unsigned long long* counter) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    uint8_t e = 0;
    if (i < count) {
        e = body_musig_sig_agg(psig32, key_offsets, keyagg192, session128, sig64, i);
        err[i] = e;
    }
    sign_count_err(e, counter);
}
#endif

}  // namespace p2e

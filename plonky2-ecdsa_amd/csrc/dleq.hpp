// Discrete-log-equality proofs (BIP-374) on secp256k1, for a batch (include/p2e.h p2e_dleq_prove_batch, p2e_dleq_verify_batch):
// a signer publishes its ECDH share C = a B together with a proof that C uses the a of its public key A = a G; a coordinator
// checks every such proof before it adds the shares (the collaborative form of sp.hpp's sender, PSBTs under BIP-375).  The
// reference has no counterpart: its only protocol is ECDSA (curve/ecdsa.rs).  Nothing here is new arithmetic but the
// verifier's R2 = s B - e C, which is point_arith.hpp's joint walk over two general points; a G, k G and s G are sign.hpp's
// one-lane fixed-base walk, a B and k B point_arith.hpp's point_glv_mul, SHA-256 is hash.hpp's compression call.
//
// The definition is include/p2e.h's; it has NOT been checked against the vectors published with BIP-374.
//
// Bytes.  Points and a_sk32 are the library's 32-byte little-endian values (they chain with the silent-payment, BIP-32 and
// point calls).  aux_rand32 and msg32 are byte strings; proof64 = bytes32(e) || bytes32(s), big-endian as the standard writes it.
// cbytes(X) is the 33-byte compressed point (02 | parity of y) || bytes32(x).
//
// Tagged hashes.  Each of "BIP0374/aux", "BIP0374/nonce", "BIP0374/challenge" is a CONSTANT chaining value (dleq_midstate;
// tests/test_dleq_cpu.py recomputes them).  A message is laid out as big-endian words at compile-time offsets (DleqMsg: every
// index is a constant once the loops are unrolled, so the words are registers), the 33-byte points straddling word boundaries:
//   nonce      t || cbytes(A) || cbytes(C) || m'                                             98 or 130 bytes: 2 or 3 compressions
//   challenge  cbytes(A) || cbytes(B) || cbytes(C) || cbytes(G) || cbytes(R1) || cbytes(R2) || m'   198 or 230 bytes: 4 compressions
// m' is msg32[i], or empty where msg32 is null (for the whole batch).
//
// Codes.  err[i] is a WIRE_* code (wire.hpp), the first failing check in the order include/p2e.h gives; a flagged element
// writes zeros to all its outputs.  The verifier's contract is schnorr.hpp's: a well-formed wrong proof is err = 0, valid = 0.
//
// Split at the hash (as sp.hpp).  Behind k on the prover's side stands dleq_prove_with_nonce, behind e dleq_response and
// dleq_verify_points; a test drives them with values no hash will ever produce (k = 0 among them).
//
// Inversions.  Two affine points share one inversion (dleq_to_affine2): A and C before the nonce hash, R1 and R2 before the
// challenge hash -- two per proof, one per verification.  The prover's two walks over B stand on either side of the nonce hash
// and each builds point_glv_mul's table {B, 2 B, 3 B} (two doublings and one addition of 128: not shared).  The verifier's
// -e A and -e C decompose the one scalar twice (glv_decompose is a few multiplications).
//
// The standard's last step of proving -- verify the fresh proof -- is NOT done, as schnorr.hpp's body_schnorr_sign does not
// verify what it signed: a caller who wants it chains p2e_dleq_verify_batch (examples/dleq_share.c does).
//
// One lane per element.  a, t and k live in registers only.  Every body reads all inputs of element i before its first store.
#pragma once
#include "sp.hpp"

namespace p2e {

typedef Secp256k1 DleqCV;
constexpr int DLEQ_TAG_AUX = 0, DLEQ_TAG_NONCE = 1, DLEQ_TAG_CHALLENGE = 2;

// the chaining value after the block SHA256(tag) || SHA256(tag), tag = "BIP0374/aux", "BIP0374/nonce", "BIP0374/challenge"
P2E_HD Sha256State dleq_midstate(int tag) {
    Sha256State s;
    if (tag == DLEQ_TAG_AUX) {
        s.h[0] = 0x48479343u, s.h[1] = 0xa9eb648cu, s.h[2] = 0x58952fe4u, s.h[3] = 0x4772d3b2u;
        s.h[4] = 0x977ab0a0u, s.h[5] = 0xcb8e2740u, s.h[6] = 0x60bb4b81u, s.h[7] = 0x68a41b66u;
    } else if (tag == DLEQ_TAG_NONCE) {
        s.h[0] = 0xa810fc87u, s.h[1] = 0x3b4a4d2au, s.h[2] = 0xe302cfb4u, s.h[3] = 0x322df1a0u;
        s.h[4] = 0xd2e7fb82u, s.h[5] = 0x7808570du, s.h[6] = 0x9c33e0cdu, s.h[7] = 0x2dfbf7f6u;
    } else {
        s.h[0] = 0x24f1c9c7u, s.h[1] = 0xd1538c75u, s.h[2] = 0xc9874ae8u, s.h[3] = 0x6566de76u;
        s.h[4] = 0x487843c9u, s.h[5] = 0xc13d8026u, s.h[6] = 0x39a2f3efu, s.h[7] = 0x2ad0fcb3u;
    }
    return s;
}

// ---------------------------------------------------------------------------------------------------------------------
// messages: up to four blocks of big-endian words, filled at compile-time byte offsets
// ---------------------------------------------------------------------------------------------------------------------
struct DleqMsg {
    u32 w[64];
};
P2E_HD DleqMsg dleq_msg_empty() {
    DleqMsg m;
    P2E_UNROLL
    for (int j = 0; j < 64; j++) m.w[j] = 0;
    return m;
}
template <int OFF>
P2E_HD void dleq_put_byte(DleqMsg& m, u32 b) {
    m.w[OFF / 4] |= b << (24 - 8 * (OFF % 4));
}
// bytes32(v) at byte OFF
template <int OFF>
P2E_HD void dleq_put32(DleqMsg& m, const U256& v) {
    constexpr int r = OFF % 4;
    P2E_UNROLL
    for (int j = 0; j < 8; j++) {
        const u32 word = v.w[7 - j];
        if constexpr (r == 0) {
            m.w[OFF / 4 + j] |= word;
        } else {
            m.w[OFF / 4 + j] |= word >> (8 * r);
            m.w[OFF / 4 + j + 1] |= word << (32 - 8 * r);
        }
    }
}
// cbytes(X) at byte OFF
template <int OFF>
P2E_HD void dleq_put_point(DleqMsg& m, const Aff& X) {
    dleq_put_byte<OFF>(m, 2u | (X.y.w[0] & 1u));
    dleq_put32<OFF + 1>(m, X.x);
}
// int(H_tag(the first BYTES bytes of m))
template <int BYTES>
P2E_HD U256 dleq_hash(int tag, DleqMsg& m) {
    constexpr int blocks = (BYTES + 9 + 63) / 64;
    static_assert(blocks <= 4, "DleqMsg holds four blocks");
    dleq_put_byte<BYTES>(m, 0x80u);
    m.w[16 * blocks - 1] = 8u * (64 + BYTES);
    Sha256State s = dleq_midstate(tag);
    P2E_UNROLL
    for (int b = 0; b < blocks; b++) {
        Sha256Block blk;
        P2E_UNROLL
        for (int j = 0; j < 16; j++) blk.w[j] = m.w[16 * b + j];
        s = sha256_compress_call(s, blk);
    }
    return schnorr_digest_int(s);
}

// k = int(H_nonce(t || cbytes(A) || cbytes(C) || m')) mod n, t = bytes32(a) xor H_aux(aux_rand)
P2E_HD U256 dleq_nonce(const U256& a, const U256& aux, const Aff& A, const Aff& C, bool has_msg, const U256& msg) {
    DleqMsg m = dleq_msg_empty();
    dleq_put32<0>(m, aux);
    const U256 ha = dleq_hash<32>(DLEQ_TAG_AUX, m);
    U256 t;
    P2E_UNROLL
    for (int j = 0; j < 8; j++) t.w[j] = a.w[j] ^ ha.w[j];
    m = dleq_msg_empty();
    dleq_put32<0>(m, t);
    dleq_put_point<32>(m, A);
    dleq_put_point<65>(m, C);
    U256 h;
    if (has_msg) {
        dleq_put32<98>(m, msg);
        h = dleq_hash<130>(DLEQ_TAG_NONCE, m);
    } else {
        h = dleq_hash<98>(DLEQ_TAG_NONCE, m);
    }
    return fe_canon<DleqCV::Fn>(h);
}
// e = int(H_challenge(cbytes(A) || cbytes(B) || cbytes(C) || cbytes(G) || cbytes(R1) || cbytes(R2) || m')): all 256 bits
P2E_HD U256 dleq_challenge(const Aff& A, const Aff& B, const Aff& C, const Aff& G, const Aff& R1, const Aff& R2, bool has_msg,
                           const U256& msg) {
    DleqMsg m = dleq_msg_empty();
    dleq_put_point<0>(m, A);
    dleq_put_point<33>(m, B);
    dleq_put_point<66>(m, C);
    dleq_put_point<99>(m, G);
    dleq_put_point<132>(m, R1);
    dleq_put_point<165>(m, R2);
    if (has_msg) {
        dleq_put32<198>(m, msg);
        return dleq_hash<230>(DLEQ_TAG_CHALLENGE, m);
    }
    return dleq_hash<198>(DLEQ_TAG_CHALLENGE, m);
}

// ---------------------------------------------------------------------------------------------------------------------
// behind the hashes: arithmetic that a test can drive with any k and any e
// ---------------------------------------------------------------------------------------------------------------------
// two non-empty sums as affine points through ONE inversion, of Z1 Z2; false: a zero Z (it cannot occur: sign.hpp)
P2E_HD bool dleq_to_affine2(const SignSum<DleqCV>& S1, const SignSum<DleqCV>& S2, Aff& P1, Aff& P2) {
    typedef DleqCV::Fp F;
    const Jac j1 = SignArith<DleqCV>::canon(S1.p), j2 = SignArith<DleqCV>::canon(S2.p);
    U256 zi;
    if (!fe_inv_safegcd<F>(fe_mul<F>(j1.Z, j2.Z), zi)) return false;
    const U256 z1 = fe_mul<F>(zi, j2.Z), z2 = fe_mul<F>(zi, j1.Z);   // 1 / Z1, 1 / Z2
    const U256 z1s = fe_sqr<F>(z1), z2s = fe_sqr<F>(z2);
    P1.x = fe_mul<F>(j1.X, z1s), P1.y = fe_mul<F>(j1.Y, fe_mul<F>(z1s, z1));
    P2.x = fe_mul<F>(j2.X, z2s), P2.y = fe_mul<F>(j2.Y, fe_mul<F>(z2s, z2));
    return true;
}
// s = (k + e a) mod n for any 256-bit e
P2E_HD U256 dleq_response(const U256& k, const U256& e, const U256& a) {
    typedef DleqCV::Fn Fn;
    return fe_add<Fn>(k, fe_mul<Fn>(fe_canon<Fn>(e), a));
}
// the proof (e, s) of C = a B under THIS k: R1 = k G, R2 = k B.  k = 0: WIRE_INFINITY.  0 < a < n; A, B, C are checked points.
P2E_HD uint8_t dleq_prove_with_nonce(const Aff* T, const U256& a, const Aff& A, const Aff& B, const Aff& C, const U256& k, bool has_msg,
                                     const U256& msg, U256& e, U256& s) {
    if (u256_is_zero(k)) return WIRE_INFINITY;
    const SignSum<DleqCV> S1 = sign_base_mul<DleqCV, SIGN_PLAN_LANE>(T, k, 0);
    const SignSum<DleqCV> S2 = point_glv_mul<DleqCV>(B, k);
    Aff R1, R2;
    if (!S1.have || !S2.have || !dleq_to_affine2(S1, S2, R1, R2)) return WIRE_INFINITY;   // (it cannot: 0 < k < n)
    e = dleq_challenge(A, B, C, T[1], R1, R2, has_msg, msg);
    s = dleq_response(k, e, a);
    return WIRE_OK;
}
// the verifier's R1 = s G - e A and R2 = s B - e C for any 256-bit e (used modulo n) and s < n; false where either is the
// neutral element.  R2 is point_arith.hpp's joint walk; s G and -e A meet in one complete addition.
P2E_HD bool dleq_verify_points(const Aff* T, const Aff& A, const Aff& B, const Aff& C, const U256& e, const U256& s, Aff& R1, Aff& R2) {
    typedef DleqCV CV;
    const U256 ne = fe_neg<CV::Fn>(fe_canon<CV::Fn>(e));
    const SignSum<CV> X2 = point_joint_mul<CV, MUL_PLAN_GLV>(B, true, s, C, true, ne);
    const SignSum<CV> EA = point_var_mul<CV, MUL_PLAN_GLV>(A, false, ne);
    const SignSum<CV> X1 = msm_add<CV, false>(sign_base_mul<CV, SIGN_PLAN_LANE>(T, s, 0), EA);
    if (!X1.have || !X2.have) return false;
    return dleq_to_affine2(X1, X2, R1, R2);
}

// ---- call 1: the share C = a B and its proof ------------------------------------------------------------------------------------
// (include/p2e.h BUFFER OVERLAP relies on this body reading every input of element i before its first store)
// the verify-what-you-proved step of the standard is NOT done (see the header)
P2E_HD uint8_t body_dleq_prove(const Aff* T, const uint8_t* a_sk32, const uint8_t* bx32, const uint8_t* by32, const uint8_t* aux_rand32,
                               const uint8_t* msg32, uint8_t* proof64, uint8_t* cx32, uint8_t* cy32, size_t i) {
    const U256 a = load_packed(a_sk32, i);
    Aff B;
    B.x = load_packed(bx32, i), B.y = load_packed(by32, i);
    const U256 aux = schnorr_load_be(aux_rand32 + 32 * i);
    const U256 msg = msg32 ? schnorr_load_be(msg32 + 32 * i) : u256_zero();
    uint8_t err = sp_scalar_check(a);
    if (!err) err = sp_point_check(B);
    U256 e = u256_zero(), s = u256_zero();
    Aff A, C;
    C.x = C.y = u256_zero();
    if (!err) {
        const SignSum<DleqCV> SA = sign_base_mul<DleqCV, SIGN_PLAN_LANE>(T, a, 0);
        const SignSum<DleqCV> SC = point_glv_mul<DleqCV>(B, a);
        if (!SA.have || !SC.have || !dleq_to_affine2(SA, SC, A, C)) err = WIRE_INFINITY;   // (it cannot: 0 < a < n)
        if (!err) err = dleq_prove_with_nonce(T, a, A, B, C, dleq_nonce(a, aux, A, C, msg32 != nullptr, msg), msg32 != nullptr, msg, e, s);
    }
    if (err) e = s = C.x = C.y = u256_zero();
    schnorr_store_be(proof64 + 64 * i, e);
    schnorr_store_be(proof64 + 64 * i + 32, s);
    if (cx32) {
        store_packed(cx32, i, C.x);
        store_packed(cy32, i, C.y);
    }
    return err;
}

// ---- call 2: the per-element verdict -----------------------------------------------------------------------------------------------
P2E_HD uint8_t body_dleq_verify(const Aff* T, const uint8_t* ax32, const uint8_t* ay32, const uint8_t* bx32, const uint8_t* by32,
                                const uint8_t* cx32, const uint8_t* cy32, const uint8_t* proof64, const uint8_t* msg32, uint8_t* valid,
                                size_t i) {
    Aff A, B, C;
    A.x = load_packed(ax32, i), A.y = load_packed(ay32, i);
    B.x = load_packed(bx32, i), B.y = load_packed(by32, i);
    C.x = load_packed(cx32, i), C.y = load_packed(cy32, i);
    const U256 e = schnorr_load_be(proof64 + 64 * i), s = schnorr_load_be(proof64 + 64 * i + 32);
    const U256 msg = msg32 ? schnorr_load_be(msg32 + 32 * i) : u256_zero();
    uint8_t err = sp_point_check(A);
    if (!err) err = sp_point_check(B);
    if (!err) err = sp_point_check(C);
    if (!err && geq_mod<DleqCV::Fn>(s.w)) err = WIRE_SCALAR_RANGE;
    bool ok = false;
    if (!err) {
        Aff R1, R2;
        if (dleq_verify_points(T, A, B, C, e, s, R1, R2)) ok = u256_eq(dleq_challenge(A, B, C, T[1], R1, R2, msg32 != nullptr, msg), e);
    }
    valid[i] = ok ? 1 : 0;
    return err;
}

#if defined(__HIPCC__)
// thread g owns element g
template <int UNUSED = 0>   // (templates so that every translation unit that includes this file may hold the definitions)
__global__ __launch_bounds__(256) void k_dleq_prove(const Aff* T, const uint8_t* a_sk32, const uint8_t* bx32, const uint8_t* by32,
                                                    const uint8_t* aux_rand32, const uint8_t* msg32, uint8_t* proof64, uint8_t* cx32,
                                                    uint8_t* cy32, size_t count, uint8_t* err, unsigned long long* counter) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    uint8_t e = 0;
    if (i < count) {
        e = body_dleq_prove(T, a_sk32, bx32, by32, aux_rand32, msg32, proof64, cx32, cy32, i);
        err[i] = e;
    }
    sign_count_err(e, counter);
}
template <int UNUSED = 0>
__global__ __launch_bounds__(256) void k_dleq_verify(const Aff* T, const uint8_t* ax32, const uint8_t* ay32, const uint8_t* bx32,
                                                     const uint8_t* by32, const uint8_t* cx32, const uint8_t* cy32, const uint8_t* proof64,
                                                     const uint8_t* msg32, uint8_t* valid, size_t count, uint8_t* err,
                                                     unsigned long long* counter) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    uint8_t e = 0;
    if (i < count) {
        e = body_dleq_verify(T, ax32, ay32, bx32, by32, cx32, cy32, proof64, msg32, valid, i);
        err[i] = e;
    }
    sign_count_err(e, counter);
}
#endif

}  // namespace p2e

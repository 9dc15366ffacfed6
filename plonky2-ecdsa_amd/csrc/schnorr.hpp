// BIP-340 Schnorr signatures on secp256k1, for a batch (include/p2e.h p2e_schnorr_public_key_batch, p2e_schnorr_sign_batch,
// p2e_schnorr_verify_batch, p2e_xonly_decode_batch, p2e_schnorr_verify_aggregate).  The reference has no counterpart: its
// only signature is ECDSA (curve/ecdsa.rs).  Nothing here is new arithmetic: SHA-256 is hash.hpp's compression, the square
// root is recover.hpp's recover_decompress, k G is sign.hpp's fixed-base walk, the variable half of s G - e P is
// point_arith.hpp's GLV walk (P2E_MUL_PLAN_AUTO's choice on this curve) and the one unrelated addition is pmsm.hpp's msm_add.
//
// Bytes.  Every argument is the standard's byte string, big-endian: sk, msg, aux, the x-only pk, sig = bytes(r) || bytes(s),
// element i at +32 i (sig: +64 i), 4-byte aligned like every packed array of this library.  A value is fetched as eight
// aligned words and byte-swapped (schnorr_load_be), so U256 word 7 - j is big-endian word j of the string -- which is also
// the j-th word of a SHA-256 block that holds it.  msg is 32 opaque bytes: it only ever travels into a block.
//
// Tagged hashes.  SHA256(SHA256(tag) || SHA256(tag) || data): the 64-byte prefix is exactly one block, so each of the three
// tags is a CONSTANT chaining value (schnorr_midstate; tests/test_schnorr_cpu.py recomputes them).  H_aux(32 bytes) is one
// compression from there; H_nonce and H_challenge (96 bytes) are two.
//
// Codes.  err[i] is a WIRE_* code (wire.hpp), the first failing check in the order include/p2e.h gives; a flagged element
// writes zeros to all its outputs.
//
// One lane per element, no LDS but the block reduction of the aggregate's preparation, nothing in the private segment.
// The signer's secrets (d, t, k', k) live in registers only; the one thing derived from them that is stored is the signature.
//
// The aggregate check (BIP-340 "Batch Verification").  With R_i = lift_x(r_i), P_i = lift_x(pk_i) (even y both) the batch
// holds iff   (sum a_i s_i) G - sum a_i R_i - sum (a_i e_i) P_i   is the neutral element, for randomisers a_i the signer
// could not predict.  The preparation kernel lifts r_i and pk_i with the ODD root -- that IS -R_i and -P_i, so no scalar is
// negated and the R scalars stay 128 bits wide -- and writes the 2 n + 1 terms in pmsm.hpp's input layout (32-byte
// little-endian scalars and coordinates):
//     [0]          sum a_i s_i mod n,   G        (the scalar by body_schnorr_agg_finish, from per-block partial sums)
//     [1 + i]      a_i,                 -R_i
//     [1 + n + i]  a_i e_i mod n,       -P_i
// a_i = the first 16 bytes of SHA-256(seed32 || LE64(i)) as a big-endian integer, 0 replaced by 1; no a_i is fixed at 1.
// A flagged element writes scalar 0 and the point (0, 0) twice -- the MSM's neutral operand -- and adds 0 to the sum, so
// the MSM never rejects a point; the verdict kernel refuses the batch on the flag count instead.
#pragma once
#include "hash.hpp"
#include "point_arith.hpp"

namespace p2e {

typedef Secp256k1 SchnorrCV;
constexpr int SCHNORR_TAG_AUX = 0, SCHNORR_TAG_NONCE = 1, SCHNORR_TAG_CHALLENGE = 2;
constexpr u32 SCHNORR_AGG_LANES = 256;   // lanes of the preparation kernel's block and of the finishing kernel

// the chaining value after the block SHA256(tag) || SHA256(tag), tag = "BIP0340/aux", "BIP0340/nonce", "BIP0340/challenge"
P2E_HD Sha256State schnorr_midstate(int tag) {
    Sha256State s;
    if (tag == SCHNORR_TAG_AUX) {
        s.h[0] = 0x24dd3219u, s.h[1] = 0x4eba7e70u, s.h[2] = 0xca0fabb9u, s.h[3] = 0x0fa3166du;
        s.h[4] = 0x3afbe4b1u, s.h[5] = 0x4c44df97u, s.h[6] = 0x4aac2739u, s.h[7] = 0x249e850au;
    } else if (tag == SCHNORR_TAG_NONCE) {
        s.h[0] = 0x46615b35u, s.h[1] = 0xf4bfbff7u, s.h[2] = 0x9f8dc671u, s.h[3] = 0x83627ab3u;
        s.h[4] = 0x60217180u, s.h[5] = 0x57358661u, s.h[6] = 0x21a29e54u, s.h[7] = 0x68b07b4cu;
    } else {
        s.h[0] = 0x9cecba11u, s.h[1] = 0x23925381u, s.h[2] = 0x11679112u, s.h[3] = 0xd1627e0fu;
        s.h[4] = 0x97c87550u, s.h[5] = 0x003cc765u, s.h[6] = 0x90f61164u, s.h[7] = 0x33e9b66au;
    }
    return s;
}

// 32 big-endian bytes at p (4-byte aligned) as an integer, and back
P2E_HD U256 schnorr_load_be(const uint8_t* p) {
    const u32* q = reinterpret_cast<const u32*>(p);
    U256 r;
    P2E_UNROLL
    for (int j = 0; j < 8; j++) r.w[7 - j] = hash_bswap32(q[j]);
    return r;
}
P2E_HD void schnorr_store_be(uint8_t* p, const U256& v) {
    u32* q = reinterpret_cast<u32*>(p);
    P2E_UNROLL
    for (int j = 0; j < 8; j++) q[j] = hash_bswap32(v.w[7 - j]);
}
// the digest read as a big-endian integer
P2E_HD U256 schnorr_digest_int(const Sha256State& s) {
    U256 r;
    P2E_UNROLL
    for (int j = 0; j < 8; j++) r.w[j] = s.h[7 - j];
    return r;
}
// int(H_tag(bytes(a) || bytes(b) || bytes(c))): two compressions behind the midstate
P2E_HD U256 schnorr_hash96(int tag, const U256& a, const U256& b, const U256& c) {
    Sha256Block blk;
    P2E_UNROLL
    for (int j = 0; j < 8; j++) blk.w[j] = a.w[7 - j], blk.w[8 + j] = b.w[7 - j];
    Sha256State s = sha256_compress_call(schnorr_midstate(tag), blk);
    P2E_UNROLL
    for (int j = 0; j < 8; j++) blk.w[j] = c.w[7 - j];
    blk.w[8] = 0x80000000u;
    sha256_finish_block(blk, 9, 8 * (64 + 96));
    return schnorr_digest_int(sha256_compress_call(s, blk));
}
// int(H_tag(bytes(a))): one compression behind the midstate
P2E_HD U256 schnorr_hash32(int tag, const U256& a) {
    Sha256Block blk;
    P2E_UNROLL
    for (int j = 0; j < 8; j++) blk.w[j] = a.w[7 - j];
    blk.w[8] = 0x80000000u;
    sha256_finish_block(blk, 9, 8 * (64 + 32));
    return schnorr_digest_int(sha256_compress_call(schnorr_midstate(tag), blk));
}
// e = int(H_challenge(bytes(r) || bytes(px) || msg)) mod n (one conditional subtraction: 2 n > 2^256)
P2E_HD U256 schnorr_challenge(const U256& r, const U256& px, const U256& msg) {
    return fe_canon<SchnorrCV::Fn>(schnorr_hash96(SCHNORR_TAG_CHALLENGE, r, px, msg));
}

// lift_x with the wanted parity of y: WIRE_COORD_RANGE for x >= p, WIRE_NOT_ON_CURVE where x^3 + 7 is no square
P2E_HD uint8_t schnorr_lift_x(const U256& x, bool odd, Aff& pt) {
    if (geq_mod<SchnorrCV::Fp>(x.w)) return WIRE_COORD_RANGE;
    return recover_decompress<SchnorrCV>(x, odd, pt) ? WIRE_OK : WIRE_NOT_ON_CURVE;
}
// 0 < d < n, as the standard demands of a secret key (it fails here; nothing is reduced)
P2E_HD bool schnorr_key_ok(const U256& d) { return !u256_is_zero(d) && !geq_mod<SchnorrCV::Fn>(d.w); }

// k G in affine coordinates for 0 < k < n; false: the walk ended on a zero Z (it cannot: sign.hpp)
P2E_HD bool schnorr_base_mul(const Aff* T, const U256& k, U256& x, U256& y) {
    const SignSum<SchnorrCV> s = sign_base_mul<SchnorrCV, SIGN_PLAN_LANE>(T, k, 0);
    return s.have && sign_to_affine<SchnorrCV, true>(s, x, y);
}

// ---- call 1: pk = bytes(x(d G)) ------------------------------------------------------------------------------------------------
// (include/p2e.h BUFFER OVERLAP relies on this body reading every input of element i before its first store)
P2E_HD uint8_t body_schnorr_public_key(const Aff* T, const uint8_t* sk32, uint8_t* pk32, size_t i) {
    const U256 d = schnorr_load_be(sk32 + 32 * i);
    uint8_t e = WIRE_OK;
    U256 x = u256_zero(), y;
    if (!schnorr_key_ok(d)) {
        e = WIRE_SCALAR_RANGE;
    } else if (!schnorr_base_mul(T, d, x, y)) {
        e = WIRE_INFINITY;
        x = u256_zero();
    }
    schnorr_store_be(pk32 + 32 * i, x);
    return e;
}

// ---- call 2: BIP-340 default signing ---------------------------------------------------------------------------------------------
// the signature under the adjusted key d (its point has even y and abscissa px) with THIS k': (rx, s).  k' = 0: WIRE_INFINITY.
P2E_HD uint8_t schnorr_sign_with_nonce(const Aff* T, const U256& d, const U256& px, const U256& msg, const U256& k0, U256& rx, U256& s) {
    typedef SchnorrCV::Fn Fn;
    U256 ry;
    if (u256_is_zero(k0) || !schnorr_base_mul(T, k0, rx, ry)) return WIRE_INFINITY;
    const U256 k = u256_select((ry.w[0] & 1u) != 0, fe_neg<Fn>(k0), k0);
    s = fe_add<Fn>(k, fe_mul<Fn>(schnorr_challenge(rx, px, msg), d));
    return WIRE_OK;
}
// the verify-what-you-signed step the standard recommends is NOT done (include/p2e.h says so)
P2E_HD uint8_t body_schnorr_sign(const Aff* T, const uint8_t* msg32, const uint8_t* sk32, const uint8_t* aux32, uint8_t* sig64, size_t i) {
    typedef SchnorrCV::Fn Fn;
    const U256 d0 = schnorr_load_be(sk32 + 32 * i);
    uint8_t e = WIRE_OK;
    U256 rx = u256_zero(), s = u256_zero(), px, py;
    if (!schnorr_key_ok(d0)) {
        e = WIRE_SCALAR_RANGE;
    } else if (!schnorr_base_mul(T, d0, px, py)) {
        e = WIRE_INFINITY;
    } else {
        const U256 msg = schnorr_load_be(msg32 + 32 * i);
        const U256 d = u256_select((py.w[0] & 1u) != 0, fe_neg<Fn>(d0), d0);
        const U256 ha = schnorr_hash32(SCHNORR_TAG_AUX, schnorr_load_be(aux32 + 32 * i));
        U256 t;
        P2E_UNROLL
        for (int j = 0; j < 8; j++) t.w[j] = d.w[j] ^ ha.w[j];
        const U256 k0 = fe_canon<Fn>(schnorr_hash96(SCHNORR_TAG_NONCE, t, px, msg));
        e = schnorr_sign_with_nonce(T, d, px, msg, k0, rx, s);
    }
    if (e) rx = s = u256_zero();
    schnorr_store_be(sig64 + 64 * i, rx);
    schnorr_store_be(sig64 + 64 * i + 32, s);
    return e;
}

// ---- call 3: the per-element verdict -----------------------------------------------------------------------------------------------
// the four checks in the header's order; pt = lift_x(pk) with the wanted parity where the code is 0
P2E_HD uint8_t schnorr_check(const U256& pk, const U256& r, const U256& s, bool odd, Aff& pt) {
    uint8_t e = schnorr_lift_x(pk, odd, pt);
    if (!e && geq_mod<SchnorrCV::Fp>(r.w)) e = WIRE_COORD_RANGE;
    if (!e && geq_mod<SchnorrCV::Fn>(s.w)) e = WIRE_SCALAR_RANGE;
    return e;
}
P2E_HD uint8_t body_schnorr_verify(const Aff* T, const uint8_t* msg32, const uint8_t* pk32, const uint8_t* sig64, uint8_t* valid, size_t i) {
    typedef SchnorrCV CV;
    const U256 pk = schnorr_load_be(pk32 + 32 * i);
    const U256 r = schnorr_load_be(sig64 + 64 * i), s = schnorr_load_be(sig64 + 64 * i + 32);
    Aff P;
    const uint8_t e = schnorr_check(pk, r, s, false, P);
    bool ok = false;
    if (!e) {
        const U256 c = schnorr_challenge(r, pk, schnorr_load_be(msg32 + 32 * i));
        // X = s G + (n - e) P: both halves may be empty (s = 0, e = 0), they may be equal or opposite: one complete addition
        const SignSum<CV> B = point_var_mul<CV, MUL_PLAN_GLV>(P, false, fe_neg<CV::Fn>(c));
        const SignSum<CV> A_ = sign_base_mul<CV, SIGN_PLAN_LANE>(T, s, 0);
        const SignSum<CV> X = msm_add<CV, false>(A_, B);
        U256 x, y;
        ok = X.have && sign_to_affine<CV, true>(X, x, y) && (y.w[0] & 1u) == 0 && u256_eq(x, r);
    }
    valid[i] = ok ? 1 : 0;
    return e;
}

// ---- call 4: x-only key -> the library's little-endian affine point with even y ------------------------------------------------------
// (include/p2e.h BUFFER OVERLAP relies on this body reading every input of element i before its first store)
P2E_HD uint8_t body_xonly_decode(const uint8_t* pk32, uint8_t* px32, uint8_t* py32, size_t i) {
    Aff P;
    const uint8_t e = schnorr_lift_x(schnorr_load_be(pk32 + 32 * i), false, P);
    store_packed(px32, i, e ? u256_zero() : P.x);
    store_packed(py32, i, e ? u256_zero() : P.y);
    return e;
}

// ---- call 5: the aggregate check's preparation ----------------------------------------------------------------------------------------
// a_i (see the header): SHA-256 of the 40 bytes seed32 || LE64(i) is one block
P2E_HD U256 schnorr_randomizer(const uint8_t* seed32, uint64_t i) {
    const u32* q = reinterpret_cast<const u32*>(seed32);
    Sha256Block blk;
    P2E_UNROLL
    for (int j = 0; j < 8; j++) blk.w[j] = hash_bswap32(q[j]);
    blk.w[8] = hash_bswap32((u32)i);
    blk.w[9] = hash_bswap32((u32)(i >> 32));
    blk.w[10] = 0x80000000u;
    sha256_finish_block(blk, 11, 8 * 40);
    const Sha256State h = sha256_compress_call(sha256_iv(), blk);
    U256 a = u256_zero();
    a.w[3] = h.h[0], a.w[2] = h.h[1], a.w[1] = h.h[2], a.w[0] = h.h[3];
    if (u256_is_zero(a)) a.w[0] = 1u;
    return a;
}
// terms 1 + i and 1 + n + i of element i; *as = a_i s_i mod n, 0 where the element is flagged.  Returns the code.
P2E_HD uint8_t body_schnorr_agg_prepare(const uint8_t* msg32, const uint8_t* pk32, const uint8_t* sig64, const uint8_t* seed32, size_t n,
                                        uint8_t* k32, uint8_t* px32, uint8_t* py32, size_t i, U256* as) {
    typedef SchnorrCV::Fn Fn;
    const U256 pk = schnorr_load_be(pk32 + 32 * i);
    const U256 r = schnorr_load_be(sig64 + 64 * i), s = schnorr_load_be(sig64 + 64 * i + 32);
    Aff P, R;
    P.x = P.y = R.x = R.y = u256_zero();
    uint8_t e = schnorr_check(pk, r, s, true, P);
    if (!e) e = schnorr_lift_x(r, true, R);   // (r < p is known: the code can only be WIRE_NOT_ON_CURVE)
    U256 a = u256_zero(), ae = u256_zero();
    *as = u256_zero();
    if (!e) {
        a = schnorr_randomizer(seed32, (uint64_t)i);
        ae = fe_mul<Fn>(a, schnorr_challenge(r, pk, schnorr_load_be(msg32 + 32 * i)));
        *as = fe_mul<Fn>(a, s);
    } else {
        P.x = P.y = R.x = R.y = u256_zero();
    }
    store_packed(k32, 1 + i, a);
    store_packed(px32, 1 + i, R.x);
    store_packed(py32, 1 + i, R.y);
    store_packed(k32, 1 + n + i, ae);
    store_packed(px32, 1 + n + i, P.x);
    store_packed(py32, 1 + n + i, P.y);
    return e;
}
// term 0: the reduced sum and G (T[1] = 1 * 16^0 G: the first entry of the generator's table)
P2E_HD void body_schnorr_agg_finish(const Aff* T, const U256& sum, uint8_t* k32, uint8_t* px32, uint8_t* py32) {
    const Aff g = T[1];
    store_packed(k32, 0, sum);
    store_packed(px32, 0, g.x);
    store_packed(py32, 0, g.y);
}
// the one verdict byte: the MSM found the neutral element and no element was flagged
P2E_HD uint8_t schnorr_agg_verdict(uint8_t msm_status, unsigned long long flagged) {
    return (msm_status == MSM_NEUTRAL && flagged == 0) ? 1 : 0;
}

#if defined(__HIPCC__)
// thread g owns element g
template <int UNUSED = 0>   // (templates so that every translation unit that includes this file may hold the definitions)
__global__ __launch_bounds__(256) void k_schnorr_public_key(const Aff* T, const uint8_t* sk32, uint8_t* pk32, size_t n, uint8_t* err,
                                                            unsigned long long* counter) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    uint8_t e = 0;
    if (i < n) {
        e = body_schnorr_public_key(T, sk32, pk32, i);
        err[i] = e;
    }
    sign_count_err(e, counter);
}
template <int UNUSED = 0>
__global__ __launch_bounds__(256) void k_schnorr_sign(const Aff* T, const uint8_t* msg32, const uint8_t* sk32, const uint8_t* aux32,
                                                      uint8_t* sig64, size_t n, uint8_t* err, unsigned long long* counter) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    uint8_t e = 0;
    if (i < n) {
        e = body_schnorr_sign(T, msg32, sk32, aux32, sig64, i);
        err[i] = e;
    }
    sign_count_err(e, counter);
}
template <int UNUSED = 0>
__global__ __launch_bounds__(256) void k_schnorr_verify(const Aff* T, const uint8_t* msg32, const uint8_t* pk32, const uint8_t* sig64,
                                                        size_t n, uint8_t* err, uint8_t* valid, unsigned long long* counter) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    uint8_t e = 0;
    if (i < n) {
        e = body_schnorr_verify(T, msg32, pk32, sig64, valid, i);
        err[i] = e;
    }
    sign_count_err(e, counter);
}
template <int UNUSED = 0>
__global__ __launch_bounds__(256) void k_xonly_decode(const uint8_t* pk32, uint8_t* px32, uint8_t* py32, size_t n, uint8_t* err,
                                                      unsigned long long* counter) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    uint8_t e = 0;
    if (i < n) {
        e = body_xonly_decode(pk32, px32, py32, i);
        err[i] = e;
    }
    sign_count_err(e, counter);
}

// the sum modulo n of the block's `v` (SCHNORR_AGG_LANES lanes), valid in lane 0: a tree in LDS, exact in any order
__device__ __forceinline__ U256 schnorr_block_sum(U256 v, u32 (&lds)[8][SCHNORR_AGG_LANES]) {
    const u32 t = threadIdx.x;
    P2E_UNROLL
    for (int k = 0; k < 8; k++) lds[k][t] = v.w[k];
    __syncthreads();
    for (u32 half = SCHNORR_AGG_LANES / 2; half > 0; half >>= 1) {
        if (t < half) {
            U256 o;
            P2E_UNROLL
            for (int k = 0; k < 8; k++) o.w[k] = lds[k][t + half];
            v = fe_add<SchnorrCV::Fn>(v, o);
            P2E_UNROLL
            for (int k = 0; k < 8; k++) lds[k][t] = v.w[k];
        }
        __syncthreads();
    }
    return v;
}
// thread g owns element g; block b leaves the sum of its a_i s_i in partial[b] (err nullable)
template <int UNUSED = 0>
__global__ __launch_bounds__(SCHNORR_AGG_LANES) void k_schnorr_agg_prepare(const uint8_t* msg32, const uint8_t* pk32, const uint8_t* sig64,
                                                                           const uint8_t* seed32, size_t n, uint8_t* k32, uint8_t* px32,
                                                                           uint8_t* py32, U256* partial, uint8_t* err,
                                                                           unsigned long long* counter) {
    __shared__ u32 lds[8][SCHNORR_AGG_LANES];
    const size_t i = (size_t)blockIdx.x * SCHNORR_AGG_LANES + threadIdx.x;
    uint8_t e = 0;
    U256 as = u256_zero();
    if (i < n) {
        e = body_schnorr_agg_prepare(msg32, pk32, sig64, seed32, n, k32, px32, py32, i, &as);
        if (err) err[i] = e;
    }
    sign_count_err(e, counter);
    const U256 sum = schnorr_block_sum(as, lds);
    if (threadIdx.x == 0) partial[blockIdx.x] = sum;
}
// one block: the `blocks` partial sums -> term 0
template <int UNUSED = 0>
__global__ __launch_bounds__(SCHNORR_AGG_LANES) void k_schnorr_agg_finish(const Aff* T, const U256* partial, u32 blocks, uint8_t* k32,
                                                                          uint8_t* px32, uint8_t* py32) {
    __shared__ u32 lds[8][SCHNORR_AGG_LANES];
    U256 v = u256_zero();
    for (u32 b = threadIdx.x; b < blocks; b += SCHNORR_AGG_LANES) v = fe_add<SchnorrCV::Fn>(v, partial[b]);
    const U256 sum = schnorr_block_sum(v, lds);
    if (threadIdx.x == 0) body_schnorr_agg_finish(T, sum, k32, px32, py32);
}
template <int UNUSED = 0>
__global__ void k_schnorr_agg_verdict(const uint8_t* msm_status, const unsigned long long* counter, uint8_t* verdict) {
    if (blockIdx.x == 0 && threadIdx.x == 0) *verdict = schnorr_agg_verdict(*msm_status, *counter);
}
#endif

}  // namespace p2e

// Silent payments (BIP-352) on secp256k1, for a batch (include/p2e.h p2e_sp_input_hash_batch, p2e_sp_label_batch,
// p2e_sp_send_batch, p2e_sp_scan_batch): the sender's output key and the receiver's scan of a transaction.  The reference
// has no counterpart: its only protocol is ECDSA (curve/ecdsa.rs).  Nothing here is new arithmetic: the ECDH is
// point_arith.hpp's point_glv_mul, B_spend + t G is sign.hpp's one-lane fixed-base walk and pmsm.hpp's complete msm_add (what
// hd.hpp's bip32_finish_pub sums), SHA-256 is hash.hpp's compression call, the inversion is sign_to_affine's.
//
// Bytes.  Points and the secret scalars of the key layer (ax32 / ay32, scan_sk32, a_sk32, spend_pk*, scan_pk*, label_*) are
// the library's 32-byte little-endian values (hd.hpp).  What BIP-352 defines as a byte string or a hash (outpoint36,
// input_hash32, the x-only outputs, tweak32, label_tweak32) is the standard's big-endian string (schnorr.hpp).
//
// Tagged hashes.  Each of "BIP0352/Inputs", "BIP0352/SharedSecret", "BIP0352/Label" is a CONSTANT chaining value (sp_midstate;
// tests/test_sp_cpu.py recomputes them).  input_hash absorbs 69 bytes (two compressions), t_k 37 bytes (one), l_m 36 (one).
//
// Codes.  err[i] is a WIRE_* code (wire.hpp), the first failing check in the order include/p2e.h gives; a flagged element
// writes zeros to all its outputs.  Arguments shared by the batch are checked by every lane and flag every element alike.
//
// Split at the hash (as hd.hpp's bip32_I / taproot.hpp's taproot_finish_*).  What produces t is sp_shared_secret (checks
// done by the body, scalar product, the GLV walk, ONE inversion, the compressed point) and sp_tweak (one compression per k);
// everything behind t is sp_finish_send / sp_finish, which a test drives with values of t no hash will ever produce.
//
// The compare needs no inversion.  A candidate stays Jacobian (X, Y, Z); x(C) == o is X == o Z^2 on canonical values.  A step k
// of the scan costs: one compression; the fixed-base walk (64 table reads, at most 64 mixed additions); one mixed addition
// with B_spend; then per candidate one squaring (Z^2) and per candidate and output one multiplication and one
// canonicalisation; per label one more complete mixed addition P_k + L_j.  No inversion: the transaction's only one is
// serP(S)'s.
//
// One lane per element.  Secrets (b_scan, a, the scalar product, S, the sender's t_k) live in registers only.  The scan's
// hit_tweak32 slots are written as the hits occur and cleared at the end where the element is flagged (the scan offers no
// in-place form: include/p2e.h); every other body reads all inputs of element i before its first store.
#pragma once
#include "taproot.hpp"
#include "point_arith.hpp"

namespace p2e {

typedef Secp256k1 SpCV;
constexpr int SP_TAG_INPUTS = 0, SP_TAG_SHARED_SECRET = 1, SP_TAG_LABEL = 2;
constexpr size_t SP_MAX_HITS = 8, SP_MAX_LABELS = 16;   // include/p2e.h P2E_SP_MAX_HITS, P2E_SP_MAX_LABELS

// the chaining value after the block SHA256(tag) || SHA256(tag), tag = "BIP0352/Inputs", "BIP0352/SharedSecret", "BIP0352/Label"
P2E_HD Sha256State sp_midstate(int tag) {
    Sha256State s;
    if (tag == SP_TAG_INPUTS) {
        s.h[0] = 0xd4143ffcu, s.h[1] = 0x012ea4b5u, s.h[2] = 0x36e21c8fu, s.h[3] = 0xf7ec7b54u;
        s.h[4] = 0x4dd4e2acu, s.h[5] = 0x9bcaa0a4u, s.h[6] = 0xe244899bu, s.h[7] = 0xcd06903eu;
    } else if (tag == SP_TAG_SHARED_SECRET) {
        s.h[0] = 0x88831537u, s.h[1] = 0x5127079bu, s.h[2] = 0x69c2137bu, s.h[3] = 0xab0303e6u;
        s.h[4] = 0x98fa21fau, s.h[5] = 0x4a888523u, s.h[6] = 0xbd99daabu, s.h[7] = 0xf25e5e0au;
    } else {
        s.h[0] = 0x26b95d63u, s.h[1] = 0x8bf1b740u, s.h[2] = 0x10a5986fu, s.h[3] = 0x06a387a5u;
        s.h[4] = 0x2d1c1c30u, s.h[5] = 0xd035951au, s.h[6] = 0x2d7f0f96u, s.h[7] = 0x29e3e0dbu;
    }
    return s;
}

// ---------------------------------------------------------------------------------------------------------------------
// checks and hashes
// ---------------------------------------------------------------------------------------------------------------------
// a point that must not be neutral: (0, 0) WIRE_INFINITY, then point_check's range and curve tests
P2E_HD uint8_t sp_point_check(const Aff& P) {
    bool neutral;
    const uint8_t e = point_check<SpCV>(P.x, P.y, neutral);
    return neutral ? WIRE_INFINITY : e;
}
// 0 < v < n, or WIRE_SCALAR_RANGE (nothing is reduced)
P2E_HD uint8_t sp_scalar_check(const U256& v) { return schnorr_key_ok(v) ? WIRE_OK : WIRE_SCALAR_RANGE; }

// big-endian word j (0 .. 8) of the 33 bytes serP = (02 | odd) || ser256(x); word 8 holds the last byte on top, zeros below
P2E_HD u32 sp_serp_word(const U256& x, u32 odd, int j) {
    if (j == 0) return ((2u | odd) << 24) | (x.w[7] >> 8);
    if (j == 8) return x.w[0] << 24;
    return (x.w[8 - j] << 24) | (x.w[7 - j] >> 8);
}
// int(H_Inputs(outpoint36 || serP(A))): 69 bytes, two compressions behind the midstate; op = the outpoint's 9 big-endian words
P2E_HD U256 sp_input_hash(const u32 (&op)[9], const Aff& A) {
    const u32 odd = A.y.w[0] & 1u;
    Sha256Block blk;
    P2E_UNROLL
    for (int j = 0; j < 9; j++) blk.w[j] = op[j];
    P2E_UNROLL
    for (int j = 0; j < 7; j++) blk.w[9 + j] = sp_serp_word(A.x, odd, j);
    const Sha256State s = sha256_compress_call(sp_midstate(SP_TAG_INPUTS), blk);
    blk.w[0] = sp_serp_word(A.x, odd, 7);
    blk.w[1] = sp_serp_word(A.x, odd, 8) | 0x00800000u;
    sha256_finish_block(blk, 2, 8 * (64 + 69));
    return schnorr_digest_int(sha256_compress_call(s, blk));
}
// t_k = int(H_SharedSecret(serP(S) || ser32(k))) for S = (sx, a y of parity s_odd): 37 bytes, one compression
P2E_HD U256 sp_tweak(const U256& sx, u32 s_odd, u32 k) {
    Sha256Block blk;
    P2E_UNROLL
    for (int j = 0; j < 8; j++) blk.w[j] = sp_serp_word(sx, s_odd, j);
    blk.w[8] = sp_serp_word(sx, s_odd, 8) | (k >> 8);
    blk.w[9] = (k << 24) | 0x00800000u;
    sha256_finish_block(blk, 10, 8 * (64 + 37));
    return schnorr_digest_int(sha256_compress_call(sp_midstate(SP_TAG_SHARED_SECRET), blk));
}
// l_m = int(H_Label(ser256(b_scan) || ser32(m))): 36 bytes, one compression
P2E_HD U256 sp_label_tweak(const U256& b_scan, u32 m) {
    Sha256Block blk;
    P2E_UNROLL
    for (int j = 0; j < 8; j++) blk.w[j] = b_scan.w[7 - j];
    blk.w[8] = m;
    blk.w[9] = 0x80000000u;
    sha256_finish_block(blk, 10, 8 * (64 + 36));
    return schnorr_digest_int(sha256_compress_call(sp_midstate(SP_TAG_LABEL), blk));
}
// S = (f d) P for a secret d and a factor f, both in [1, n - 1] (`with_factor` false: S = d P), P on the curve and not
// neutral: x(S) and the parity of y(S), what serP(S) needs.  One GLV walk, one inversion.  WIRE_INFINITY: it cannot occur
// (f d != 0 mod the prime n, P has order n).
P2E_HD uint8_t sp_shared_secret(const U256& d, bool with_factor, const U256& f, const Aff& P, U256& sx, u32& s_odd) {
    const U256 k = with_factor ? fe_mul<SpCV::Fn>(f, d) : d;
    const SignSum<SpCV> S = point_glv_mul<SpCV>(P, k);
    U256 sy;
    if (!S.have || !sign_to_affine<SpCV, true>(S, sx, sy)) return WIRE_INFINITY;
    s_odd = sy.w[0] & 1u;
    return WIRE_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// behind the hash: arithmetic that a test can drive with any t
// ---------------------------------------------------------------------------------------------------------------------
// P_k = B_spend + t G as a Jacobian sum.  t = 0 or t >= n: WIRE_SCALAR_RANGE (BIP-352 fails there); the neutral element
// (t G = -B_spend): WIRE_INFINITY.  t G = B_spend (the doubling) is computed.
P2E_HD uint8_t sp_output_point(const Aff* T, const Aff& B_spend, const U256& t, SignSum<SpCV>& Pk) {
    if (!schnorr_key_ok(t)) return WIRE_SCALAR_RANGE;
    SignSum<SpCV> B;
    B.p = SignArith<SpCV>::from_aff(B_spend);
    B.have = true;
    Pk = msm_add<SpCV, true>(sign_base_mul<SpCV, SIGN_PLAN_LANE>(T, t, 0), B);
    return Pk.have ? WIRE_OK : WIRE_INFINITY;
}
// the sender's side: out = x(B_spend + t G)
P2E_HD uint8_t sp_finish_send(const Aff* T, const Aff& B_spend, const U256& t, U256& out) {
    SignSum<SpCV> Pk;
    const uint8_t e = sp_output_point(T, B_spend, t, Pk);
    if (e) return e;
    U256 y;
    return sign_to_affine<SpCV, false>(Pk, out, y) ? WIRE_OK : WIRE_INFINITY;   // (a zero Z under `have` cannot occur)
}

// the hits of one transaction so far: output indices and labels (0 unlabelled, j + 1 for label j), in registers
struct SpHits {
    u32 out[SP_MAX_HITS], label[SP_MAX_HITS];
    u32 count;
};
P2E_HD SpHits sp_no_hits() {
    SpHits h;
    P2E_UNROLL
    for (int j = 0; j < (int)SP_MAX_HITS; j++) h.out[j] = h.label[j] = 0;
    h.count = 0;
    return h;
}
P2E_HD bool sp_is_taken(const SpHits& h, u32 out) {
    bool taken = false;
    P2E_UNROLL
    for (int j = 0; j < (int)SP_MAX_HITS; j++) taken = taken || ((u32)j < h.count && h.out[j] == out);
    return taken;
}
P2E_HD void sp_record(SpHits& h, u32 out, u32 label) {
    P2E_UNROLL
    for (int j = 0; j < (int)SP_MAX_HITS; j++) {
        h.out[j] = (u32)j == h.count ? out : h.out[j];
        h.label[j] = (u32)j == h.count ? label : h.label[j];
    }
    h.count++;
}
// the lowest-index free output of outputs[0, n_out) (32-byte big-endian strings) whose value is x(C); n_out where none is.
// Only indices below `below` are looked at.  An output >= p never matches.
P2E_HD u32 sp_match(const SignSum<SpCV>& C, const uint8_t* outputs, u32 n_out, u32 below, const SpHits& hits) {
    typedef RecField<SpCV> FA;
    if (!C.have) return n_out;   // the neutral element matches nothing
    const FA::E zz = FA::sqr(C.p.Z);
    const U256 X = FA::canon(C.p.X);
    const u32 end = below < n_out ? below : n_out;
    for (u32 j = 0; j < end; j++) {
        const U256 o = schnorr_load_be(outputs + 32 * (size_t)j);
        if (geq_mod<SpCV::Fp>(o.w) || sp_is_taken(hits, j)) continue;
        if (u256_eq(FA::canon(FA::mul(FA::from(o), zz)), X)) return j;
    }
    return n_out;
}
// Step k of the scan loop behind t = t_k: the candidates P_k, P_k + L_0, .. in this order against the outputs that are not yet
// hits.  The hit is the lowest-index matching output, under its first matching candidate; it is recorded in `hits`.
// `found` = a hit was recorded.  Codes as sp_output_point; a neutral P_k + L_j matches nothing and is no error.
// The labels are the batch's (x, y) little-endian arrays, already checked.
P2E_HD uint8_t sp_finish(const Aff* T, const Aff& B_spend, const uint8_t* label_x32, const uint8_t* label_y32, u32 n_labels, const U256& t,
                         const uint8_t* outputs, u32 n_out, SpHits& hits, bool& found) {
    found = false;
    SignSum<SpCV> Pk;
    const uint8_t e = sp_output_point(T, B_spend, t, Pk);
    if (e) return e;
    u32 best = sp_match(Pk, outputs, n_out, n_out, hits), best_label = 0;
    for (u32 j = 0; j < n_labels && best != 0; j++) {   // (a later candidate wins only with a LOWER output index)
        SignSum<SpCV> L;
        Aff l;
        l.x = load_packed(label_x32, j), l.y = load_packed(label_y32, j);
        L.p = SignArith<SpCV>::from_aff(l);
        L.have = true;
        const u32 at = sp_match(msm_add<SpCV, true>(Pk, L), outputs, n_out, best, hits);
        if (at < best) best = at, best_label = j + 1;
    }
    if (best < n_out) {
        sp_record(hits, best, best_label);
        found = true;
    }
    return WIRE_OK;
}

// ---- call 1: input_hash = int(H_Inputs(outpoint || serP(A))) ---------------------------------------------------------------------
P2E_HD uint8_t body_sp_input_hash(const uint8_t* outpoint36, const uint8_t* ax32, const uint8_t* ay32, uint8_t* input_hash32, size_t i) {
    Aff A;
    A.x = load_packed(ax32, i), A.y = load_packed(ay32, i);
    u32 op[9];
    const u32* q = reinterpret_cast<const u32*>(outpoint36 + 36 * i);
    P2E_UNROLL
    for (int j = 0; j < 9; j++) op[j] = hash_bswap32(q[j]);
    uint8_t e = sp_point_check(A);
    U256 h = u256_zero();
    if (!e) {
        h = sp_input_hash(op, A);
        e = sp_scalar_check(h);
    }
    schnorr_store_be(input_hash32 + 32 * i, e ? u256_zero() : h);
    return e;
}

// ---- call 2: label m of the one scan key: l_m and L_m = l_m G -----------------------------------------------------------------------
P2E_HD uint8_t body_sp_label(const Aff* T, const uint8_t* scan_sk32, const uint32_t* label_index, uint8_t* label_tweak32, uint8_t* label_x32,
                             uint8_t* label_y32, size_t i) {
    const U256 b = load_packed(scan_sk32, 0);
    const u32 m = label_index[i];
    uint8_t e = sp_scalar_check(b);
    U256 l = u256_zero(), x = u256_zero(), y = u256_zero();
    if (!e) {
        l = sp_label_tweak(b, m);
        e = sp_scalar_check(l);
        if (!e && !schnorr_base_mul(T, l, x, y)) e = WIRE_INFINITY;   // (it cannot: 0 < l < n)
    }
    schnorr_store_be(label_tweak32 + 32 * i, e ? u256_zero() : l);
    hd_store_key(label_x32, i, x, e != 0);
    hd_store_key(label_y32, i, y, e != 0);
    return e;
}

// ---- call 3: the sender's output key x(B_spend + t_k G), S = (input_hash a) B_scan ----------------------------------------------------
// (include/p2e.h BUFFER OVERLAP relies on this body reading every input of element i before its first store)
P2E_HD uint8_t body_sp_send(const Aff* T, const uint8_t* a_sk32, const uint8_t* input_hash32, const uint8_t* scan_pkx32,
                            const uint8_t* scan_pky32, const uint8_t* spend_pkx32, const uint8_t* spend_pky32, const uint32_t* k,
                            uint8_t* out_pk32, size_t i) {
    const U256 a = load_packed(a_sk32, i), ih = schnorr_load_be(input_hash32 + 32 * i);
    Aff Bscan, Bspend;
    Bscan.x = load_packed(scan_pkx32, i), Bscan.y = load_packed(scan_pky32, i);
    Bspend.x = load_packed(spend_pkx32, i), Bspend.y = load_packed(spend_pky32, i);
    const u32 kk = k[i];
    uint8_t e = sp_scalar_check(a);
    if (!e) e = sp_scalar_check(ih);
    if (!e) e = sp_point_check(Bscan);
    if (!e) e = sp_point_check(Bspend);
    U256 out = u256_zero();
    if (!e) {
        U256 sx;
        u32 s_odd = 0;
        e = sp_shared_secret(a, true, ih, Bscan, sx, s_odd);
        if (!e) e = sp_finish_send(T, Bspend, sp_tweak(sx, s_odd, kk), out);
    }
    schnorr_store_be(out_pk32 + 32 * i, e ? u256_zero() : out);
    return e;
}

// ---- call 4: the receiver's scan of transaction i, S = (input_hash b_scan) A -------------------------------------------------------------
// outputs of transaction i: outputs32 + 32 out_offsets[i] .. 32 out_offsets[i + 1].  input_hash32 nullable: S = b_scan A.
P2E_HD uint8_t body_sp_scan(const Aff* T, const uint8_t* scan_sk32, const uint8_t* spend_pkx32, const uint8_t* spend_pky32,
                            const uint8_t* label_x32, const uint8_t* label_y32, u32 n_labels, const uint8_t* ax32, const uint8_t* ay32,
                            const uint8_t* input_hash32, const uint8_t* outputs32, const uint64_t* out_offsets, u32 max_hits, uint8_t* n_hits,
                            uint32_t* hit_output, uint8_t* hit_label, uint8_t* hit_tweak32, size_t i) {
    const U256 b = load_packed(scan_sk32, 0);
    Aff Bspend, A;
    Bspend.x = load_packed(spend_pkx32, 0), Bspend.y = load_packed(spend_pky32, 0);
    A.x = load_packed(ax32, i), A.y = load_packed(ay32, i);
    const U256 ih = input_hash32 ? schnorr_load_be(input_hash32 + 32 * i) : u256_zero();
    const u64 lo = out_offsets[i], hi = out_offsets[i + 1];
    uint8_t e = sp_scalar_check(b);
    if (!e) e = sp_point_check(Bspend);
    for (u32 j = 0; j < n_labels && !e; j++) {
        Aff l;
        l.x = load_packed(label_x32, j), l.y = load_packed(label_y32, j);
        e = sp_point_check(l);
    }
    if (!e) e = sp_point_check(A);
    if (!e && input_hash32) e = sp_scalar_check(ih);
    if (!e && (hi < lo || hi - lo > 0xFFFFFFFFull)) e = WIRE_BAD_LENGTH;
    SpHits hits = sp_no_hits();
    uint8_t* const tweaks = hit_tweak32 + 32 * (size_t)max_hits * i;
    if (!e) {
        U256 sx;
        u32 s_odd = 0;
        e = sp_shared_secret(b, input_hash32 != nullptr, ih, A, sx, s_odd);
        const uint8_t* outputs = outputs32 + 32 * (size_t)lo;
        const u32 n_out = (u32)(hi - lo);
        while (!e && hits.count < max_hits) {
            const U256 t = sp_tweak(sx, s_odd, hits.count);
            bool found;
            e = sp_finish(T, Bspend, label_x32, label_y32, n_labels, t, outputs, n_out, hits, found);
            if (e || !found) break;
            schnorr_store_be(tweaks + 32 * (size_t)(hits.count - 1), t);
        }
    }
    const u32 kept = e ? 0u : hits.count;   // (a flag at a step k > 0 drops the hits already recorded)
    n_hits[i] = (uint8_t)kept;
    P2E_UNROLL
    for (int h = 0; h < (int)SP_MAX_HITS; h++) {
        if ((u32)h >= max_hits) continue;
        const bool used = (u32)h < kept;
        hit_output[(size_t)max_hits * i + h] = used ? hits.out[h] : 0u;
        hit_label[(size_t)max_hits * i + h] = used ? (uint8_t)hits.label[h] : (uint8_t)0;
        if (!used) schnorr_store_be(tweaks + 32 * (size_t)h, u256_zero());
    }
    return e;
}

#if defined(__HIPCC__)
// thread g owns element g
template <int UNUSED = 0>   // (templates so that every translation unit that includes this file may hold the definitions)
__global__ __launch_bounds__(256) void k_sp_input_hash(const uint8_t* outpoint36, const uint8_t* ax32, const uint8_t* ay32, uint8_t* input_hash32,
                                                       size_t count, uint8_t* err, unsigned long long* counter) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    uint8_t e = 0;
    if (i < count) {
        e = body_sp_input_hash(outpoint36, ax32, ay32, input_hash32, i);
        err[i] = e;
    }
    sign_count_err(e, counter);
}
template <int UNUSED = 0>
__global__ __launch_bounds__(256) void k_sp_label(const Aff* T, const uint8_t* scan_sk32, const uint32_t* label_index, uint8_t* label_tweak32,
                                                  uint8_t* label_x32, uint8_t* label_y32, size_t count, uint8_t* err,
                                                  unsigned long long* counter) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    uint8_t e = 0;
    if (i < count) {
        e = body_sp_label(T, scan_sk32, label_index, label_tweak32, label_x32, label_y32, i);
        err[i] = e;
    }
    sign_count_err(e, counter);
}
template <int UNUSED = 0>
__global__ __launch_bounds__(256) void k_sp_send(const Aff* T, const uint8_t* a_sk32, const uint8_t* input_hash32, const uint8_t* scan_pkx32,
                                                 const uint8_t* scan_pky32, const uint8_t* spend_pkx32, const uint8_t* spend_pky32,
                                                 const uint32_t* k, uint8_t* out_pk32, size_t count, uint8_t* err, unsigned long long* counter) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    uint8_t e = 0;
    if (i < count) {
        e = body_sp_send(T, a_sk32, input_hash32, scan_pkx32, scan_pky32, spend_pkx32, spend_pky32, k, out_pk32, i);
        err[i] = e;
    }
    sign_count_err(e, counter);
}
template <int UNUSED = 0>
__global__ __launch_bounds__(256) void k_sp_scan(const Aff* T, const uint8_t* scan_sk32, const uint8_t* spend_pkx32, const uint8_t* spend_pky32,
                                                 const uint8_t* label_x32, const uint8_t* label_y32, u32 n_labels, const uint8_t* ax32,
                                                 const uint8_t* ay32, const uint8_t* input_hash32, const uint8_t* outputs32,
                                                 const uint64_t* out_offsets, u32 max_hits, uint8_t* n_hits, uint32_t* hit_output,
                                                 uint8_t* hit_label, uint8_t* hit_tweak32, size_t count, uint8_t* err,
                                                 unsigned long long* counter) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    uint8_t e = 0;
    if (i < count) {
        e = body_sp_scan(T, scan_sk32, spend_pkx32, spend_pky32, label_x32, label_y32, n_labels, ax32, ay32, input_hash32, outputs32,
                         out_offsets, max_hits, n_hits, hit_output, hit_label, hit_tweak32, i);
        err[i] = e;
    }
    sign_count_err(e, counter);
}
#endif

}  // namespace p2e

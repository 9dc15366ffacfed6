// Taproot (BIP-341) on secp256k1, for a batch (include/p2e.h p2e_taproot_leaf_hash_batch, p2e_taproot_merkle_root_batch,
// p2e_taproot_tweak_pubkey_batch, p2e_taproot_tweak_seckey_batch, p2e_taproot_verify_commitment_batch): what lies between an
// x-only key and a BIP-340 signature.  The reference has no counterpart: its only signature is ECDSA (curve/ecdsa.rs).
// Nothing here is new arithmetic: SHA-256 is hash.hpp's compression, lift_x is schnorr.hpp's (recover.hpp's
// recover_decompress), and P + t G is hd.hpp's bip32_finish_pub -- sign.hpp's one-lane fixed-base walk and pmsm.hpp's complete
// msm_add (it doubles where t G = P, returns P for t = 0 and yields the neutral element where t G = -P).
//
// Bytes.  Every key, hash and tweak is the standard's big-endian 32-byte string, element i at +32 i, 4-byte aligned
// (schnorr.hpp).  A hash that only travels into another block stays 8 big-endian words (Words8: word 0 = bytes 0 .. 3, loaded
// and stored as hd.hpp does chain codes); a key or tweak that is computed with is a U256 (word 7 - j = big-endian word j).  `script` is a concatenated buffer at any
// alignment, read as hash.hpp reads messages.
//
// Tagged hashes.  SHA256(SHA256(tag) || SHA256(tag) || data): each of "TapLeaf", "TapBranch", "TapTweak" is a CONSTANT
// chaining value (taproot_midstate; tests/test_taproot_cpu.py recomputes them).  A branch and a tweak over a root are two
// compressions from there (64 bytes of data, then the padding block), a tweak over the key alone is one.
//
// The leaf hash absorbs version || compact_size(len) || script: a prefix of 2, 4 or 6 bytes in front of a message of the
// buffer (sha256_prefixed_message).  The stream is the script's view moved back by the prefix length; its words in front
// of the script's first word are never read, the prefix bytes are merged into stream words 0 and 1 instead.
//
// Codes.  err[i] is a WIRE_* code (wire.hpp), the first failing check in the order include/p2e.h gives; a flagged element
// writes zeros to all its outputs.
//
// Split at the hash (as hd.hpp's bip32_I / bip32_finish_*): everything behind t is taproot_finish_pub / taproot_finish_sec,
// which a test drives with values of t no hash will ever produce.
//
// One lane per element, no LDS, nothing in the private segment.  The SHA-256 compression stays hash.hpp's call
// (sha256_compress_call, 24 words in registers): a kernel holds the rounds once however many levels a path has.  The
// secret-key call's d, t and d + t live in registers only; the one thing stored is the tweaked key.
#pragma once
#include "hd.hpp"
#include "schnorr.hpp"

namespace p2e {

typedef Secp256k1 TaprootCV;
constexpr int TAPROOT_TAG_LEAF = 0, TAPROOT_TAG_BRANCH = 1, TAPROOT_TAG_TWEAK = 2;
constexpr size_t TAPROOT_MAX_DEPTH = 128;   // BIP-341: a control block holds at most 128 nodes

// the chaining value after the block SHA256(tag) || SHA256(tag), tag = "TapLeaf", "TapBranch", "TapTweak"
P2E_HD Sha256State taproot_midstate(int tag) {
    Sha256State s;
    if (tag == TAPROOT_TAG_LEAF) {
        s.h[0] = 0x9ce0e4e6u, s.h[1] = 0x7c116c39u, s.h[2] = 0x38b3caf2u, s.h[3] = 0xc30f5089u;
        s.h[4] = 0xd3f3936cu, s.h[5] = 0x47636e60u, s.h[6] = 0x7db33eeau, s.h[7] = 0xddc6f0c9u;
    } else if (tag == TAPROOT_TAG_BRANCH) {
        s.h[0] = 0x23a865a9u, s.h[1] = 0xb8a40da7u, s.h[2] = 0x977c1e04u, s.h[3] = 0xc49e246fu;
        s.h[4] = 0xb5be1376u, s.h[5] = 0x9d24c9b7u, s.h[6] = 0xb583b5d4u, s.h[7] = 0xa8d226d2u;
    } else {
        s.h[0] = 0xd129a2f3u, s.h[1] = 0x701c655du, s.h[2] = 0x6583b6c3u, s.h[3] = 0xb9419727u;
        s.h[4] = 0x95f4e232u, s.h[5] = 0x94fd54f4u, s.h[6] = 0xa2ae8d85u, s.h[7] = 0x47ca590bu;
    }
    return s;
}

// ---------------------------------------------------------------------------------------------------------------------
// SHA-256 from a given chaining value over  prefix || message  (sha256_message, generalised)
// ---------------------------------------------------------------------------------------------------------------------
// up to 8 bytes in front of a message: big-endian words (the first byte on top of w[0]), bytes beyond `len` zero
struct ShaPrefix {
    u32 w[2];
    u32 len;
};
// The message's view moved back by `back` < 8 bytes: stream byte s is the byte at (first script byte) - back + s.  word(k)
// is aligned word k of the STREAM, or 0 where that word holds no byte of the message -- the words in front of the message's
// own first word included, which the plain view never reaches.
struct ShiftedView {
    uintptr_t q;        // the address of the aligned word that holds stream byte 0 (it may lie in front of the buffer)
    u32 sh;             // 8 * (address of stream byte 0 mod 4)
    uintptr_t first;    // the message's own first aligned word
    uintptr_t end;      // MsgView::end
    P2E_HD u32 word(u64 k) const {
        const uintptr_t a = q + 4 * (uintptr_t)k;
        return (a >= first && a < end) ? *reinterpret_cast<const u32*>(a) : 0u;
    }
};
P2E_HD ShiftedView shifted_view(const MsgView& m, u32 back) {
    const uintptr_t a = (uintptr_t)m.p + (m.sh >> 3) - back;
    ShiftedView v;
    v.q = a & ~(uintptr_t)3;
    v.sh = 8u * (u32)(a & 3u);
    v.first = (uintptr_t)m.p;
    v.end = m.end;
    return v;
}
// SHA-256 continued from `start`, which stands for `done` bytes (a multiple of 64), over px || m
P2E_HD Sha256State sha256_prefixed_message(const Sha256State& start, u64 done, const ShaPrefix& px, const MsgView& m) {
    Sha256State st = start;
    const ShiftedView sv = shifted_view(m, px.len);
    const u64 len = px.len + m.len;             // of the stream
    const u64 nblocks = (len + 8) / 64 + 1;     // the 0x80 byte and the 64-bit length always fit
    const u64 bits = 8 * (done + len);
    u32 carry = sv.word(0);
    for (u64 b = 0; b < nblocks; b++) {
        Sha256Block blk;
        const u64 pos = 64 * b;
        P2E_UNROLL
        for (int j = 0; j < 16; j++) {
            const u32 next = sv.word(16 * b + j + 1);
            u32 v = hash_bswap32(hash_join(carry, next, sv.sh));   // stream bytes pos + 4 j .. + 3, first byte on top
            carry = next;
            if (j < 2 && b == 0) {                                  // the prefix's 0 .. 4 bytes of this word, from the top
                const u32 nb = px.len > 4u * j ? (px.len - 4u * j < 4u ? px.len - 4u * j : 4u) : 0u;
                const u32 pm = nb ? 0xFFFFFFFFu << (8 * (4 - nb)) : 0u;
                v = (v & ~pm) | (px.w[j & 1] & pm);
            }
            const u64 at = pos + 4 * j;
            if (at + 4 > len) {                                    // the stream ends inside or before this word
                const u32 keep = at < len ? (u32)(len - at) : 0u;
                const u32 cut = 0xFFFFFFFFu >> (8 * keep);
                v = at <= len ? ((v & ~cut) | (0x80000000u >> (8 * keep))) : 0u;
            }
            blk.w[j] = v;
        }
        if (b + 1 == nblocks) {
            blk.w[14] = (u32)(bits >> 32);
            blk.w[15] = (u32)bits;
        }
        st = sha256_compress_call(st, blk);
    }
    return st;
}

// ---------------------------------------------------------------------------------------------------------------------
// the three tagged hashes
// ---------------------------------------------------------------------------------------------------------------------
P2E_HD Words8 taproot_zero_words() {
    Words8 r;
    P2E_UNROLL
    for (int j = 0; j < 8; j++) r.w[j] = 0;
    return r;
}
// version || compact_size(len): 2 bytes below 253, fd + 2 little-endian bytes up to 0xffff, fe + 4 above (len < 2^32)
P2E_HD ShaPrefix taproot_leaf_prefix(u32 version, u32 len) {
    ShaPrefix p;
    p.w[1] = 0;
    if (len < 253u) {
        p.w[0] = (version << 24) | (len << 16);
        p.len = 2;
    } else if (len <= 0xFFFFu) {
        p.w[0] = (version << 24) | (0xFDu << 16) | ((len & 0xFFu) << 8) | (len >> 8);
        p.len = 4;
    } else {
        p.w[0] = (version << 24) | (0xFEu << 16) | ((len & 0xFFu) << 8) | ((len >> 8) & 0xFFu);
        p.w[1] = (((len >> 16) & 0xFFu) << 24) | ((len >> 24) << 16);
        p.len = 6;
    }
    return p;
}
// H_TapLeaf(version || compact_size(len) || script), len < 2^32
P2E_HD Words8 taproot_leaf_hash(u32 version, const MsgView& script) {
    return hd_digest_words(sha256_prefixed_message(taproot_midstate(TAPROOT_TAG_LEAF), 64, taproot_leaf_prefix(version, (u32)script.len), script));
}
// a < b as 32-byte strings (lexicographic = big-endian words from word 0)
P2E_HD bool taproot_less(const Words8& a, const Words8& b) {
    bool less = false, decided = false;
    P2E_UNROLL
    for (int j = 0; j < 8; j++) {
        less = decided ? less : a.w[j] < b.w[j];
        decided = decided || a.w[j] != b.w[j];
    }
    return less;
}
// H_TapBranch(min(a, b) || max(a, b)): two compressions behind the midstate
P2E_HD Words8 taproot_branch(const Words8& a, const Words8& b) {
    const bool swap = taproot_less(b, a);
    Sha256Block blk;
    P2E_UNROLL
    for (int j = 0; j < 8; j++) blk.w[j] = swap ? b.w[j] : a.w[j], blk.w[8 + j] = swap ? a.w[j] : b.w[j];
    const Sha256State s = sha256_compress_call(taproot_midstate(TAPROOT_TAG_BRANCH), blk);
    blk.w[0] = 0x80000000u;
    sha256_finish_block(blk, 1, 8 * (64 + 64));
    return hd_digest_words(sha256_compress_call(s, blk));
}
// k = leaf; k = H_TapBranch(k, node j) for the `depth` nodes at path32 + 32 (first + j)
P2E_HD Words8 taproot_walk(Words8 k, const uint8_t* path32, size_t first, u32 depth) {
    for (u32 j = 0; j < depth; j++) k = taproot_branch(k, hd_load_cc(path32, first + j));
    return k;
}
// t = int(H_TapTweak(bytes(px) || root)); !with_root: nothing is appended (BIP-86's key-path-only output), one compression
P2E_HD U256 taproot_tweak(const U256& px, bool with_root, const Words8& root) {
    Sha256Block blk;
    P2E_UNROLL
    for (int j = 0; j < 8; j++) blk.w[j] = px.w[7 - j], blk.w[8 + j] = with_root ? root.w[j] : (j == 0 ? 0x80000000u : 0u);
    if (!with_root) blk.w[15] = 8 * (64 + 32);
    Sha256State s = sha256_compress_call(taproot_midstate(TAPROOT_TAG_TWEAK), blk);
    if (with_root) {
        blk.w[0] = 0x80000000u;
        sha256_finish_block(blk, 1, 8 * (64 + 64));
        s = sha256_compress_call(s, blk);
    }
    return schnorr_digest_int(s);
}

// ---------------------------------------------------------------------------------------------------------------------
// behind the hash: arithmetic that a test can drive with any t
// ---------------------------------------------------------------------------------------------------------------------
// Q = P + t G for a P on the curve.  t >= n: WIRE_SCALAR_RANGE (not reduced); the neutral element: WIRE_INFINITY.  t = 0 (an
// empty walk: Q = P) and t G = P (the doubling) are computed.  qx = x(Q), parity = y(Q) & 1.
P2E_HD uint8_t taproot_finish_pub(const Aff* T, const Aff& P, const U256& t, U256& qx, u32& parity) {
    Aff Q;
    const uint8_t e = bip32_finish_pub(T, t, P, Q);   // (the same sum: I_L G + K_par there, t G + P here, with the same codes)
    if (e) return e;
    qx = Q.x;
    parity = Q.y.w[0] & 1u;
    return WIRE_OK;
}
// out = d + t mod n for the adjusted key d (0 < d < n, its point has even y).  t >= n: WIRE_SCALAR_RANGE; 0: WIRE_INFINITY.
P2E_HD uint8_t taproot_finish_sec(const U256& d, const U256& t, U256& out) { return bip32_finish_priv(t, d, out); }
// the tweaked key of the x-only key pk: the two key checks, the hash, the arithmetic
P2E_HD uint8_t taproot_output_key(const Aff* T, const U256& pk, bool with_root, const Words8& root, U256& qx, u32& parity) {
    Aff P;
    const uint8_t e = schnorr_lift_x(pk, false, P);
    if (e) return e;
    return taproot_finish_pub(T, P, taproot_tweak(pk, with_root, root), qx, parity);
}

// ---- call 1: leaf32 = H_TapLeaf(version || compact_size(len) || script) -----------------------------------------------------------
P2E_HD uint8_t body_taproot_leaf_hash(const uint8_t* leaf_version, const uint8_t* script, const uint64_t* offsets, uint8_t* leaf32, size_t i) {
    const u32 version = leaf_version[i];
    const u64 lo = offsets[i], hi = offsets[i + 1];
    uint8_t e = WIRE_OK;
    Words8 h = taproot_zero_words();
    if (version & 1u) {            // bit 0 is the control block's parity bit
        e = WIRE_BAD_PREFIX;
    } else if (hi < lo || hi - lo >= ((u64)1 << 32)) {
        e = WIRE_BAD_LENGTH;
    } else {
        bool bad;
        h = taproot_leaf_hash(version, msg_view(script, offsets, i, &bad));
    }
    hd_store_cc(leaf32, i, h, false);
    return e;
}

// ---- call 2: the Merkle root of a leaf and its path ---------------------------------------------------------------------------------
// (include/p2e.h BUFFER OVERLAP relies on this body reading every input of element i before its first store)
P2E_HD uint8_t body_taproot_merkle_root(const uint8_t* leaf32, const uint8_t* path32, const uint8_t* depth, size_t max_depth,
                                        uint8_t* root32, size_t i) {
    const u32 d = depth[i];
    Words8 k = hd_load_cc(leaf32, i);
    uint8_t e = WIRE_OK;
    if (d > max_depth) {
        e = WIRE_BAD_LENGTH;
        k = taproot_zero_words();
    } else {
        k = taproot_walk(k, path32, i * max_depth, d);
    }
    hd_store_cc(root32, i, k, false);
    return e;
}

// ---- call 3: BIP-341 taproot_tweak_pubkey (root32 nullable: no root) -------------------------------------------------------------------
// (include/p2e.h BUFFER OVERLAP relies on this body reading every input of element i before its first store)
P2E_HD uint8_t body_taproot_tweak_pubkey(const Aff* T, const uint8_t* pk32, const uint8_t* root32, uint8_t* out_pk32, uint8_t* out_parity,
                                         size_t i) {
    const U256 pk = schnorr_load_be(pk32 + 32 * i);
    const Words8 root = root32 ? hd_load_cc(root32, i) : taproot_zero_words();
    U256 qx = u256_zero();
    u32 parity = 0;
    const uint8_t e = taproot_output_key(T, pk, root32 != nullptr, root, qx, parity);
    schnorr_store_be(out_pk32 + 32 * i, e ? u256_zero() : qx);
    out_parity[i] = e ? 0 : (uint8_t)parity;
    return e;
}

// ---- call 4: BIP-341 taproot_tweak_seckey ------------------------------------------------------------------------------------------------
// (include/p2e.h BUFFER OVERLAP relies on this body reading every input of element i before its first store)
P2E_HD uint8_t body_taproot_tweak_seckey(const Aff* T, const uint8_t* sk32, const uint8_t* root32, uint8_t* out_sk32, size_t i) {
    typedef TaprootCV::Fn Fn;
    const U256 d0 = schnorr_load_be(sk32 + 32 * i);
    const Words8 root = root32 ? hd_load_cc(root32, i) : taproot_zero_words();
    uint8_t e = WIRE_OK;
    U256 out = u256_zero(), px, py;
    if (!schnorr_key_ok(d0)) {
        e = WIRE_SCALAR_RANGE;
    } else if (!schnorr_base_mul(T, d0, px, py)) {
        e = WIRE_INFINITY;   // (it cannot: 0 < d < n)
    } else {
        const U256 d = u256_select((py.w[0] & 1u) != 0, fe_neg<Fn>(d0), d0);
        e = taproot_finish_sec(d, taproot_tweak(px, root32 != nullptr, root), out);
    }
    schnorr_store_be(out_sk32 + 32 * i, e ? u256_zero() : out);
    return e;
}

// ---- call 5: BIP-341's script-path commitment: Merkle walk, tweak, point, compare ------------------------------------------------------------
// (valid[i] is this body's only store and comes last)
P2E_HD uint8_t body_taproot_verify_commitment(const Aff* T, const uint8_t* out_pk32, const uint8_t* out_parity, const uint8_t* pk32,
                                              const uint8_t* leaf32, const uint8_t* path32, const uint8_t* depth, size_t max_depth,
                                              uint8_t* valid, size_t i) {
    const u32 want_parity = out_parity[i], d = depth[i];
    uint8_t e = WIRE_OK;
    bool ok = false;
    if (want_parity > 1u) {
        e = WIRE_BAD_PREFIX;
    } else if (d > max_depth) {
        e = WIRE_BAD_LENGTH;
    } else {
        const U256 pk = schnorr_load_be(pk32 + 32 * i);
        Aff P;
        e = schnorr_lift_x(pk, false, P);
        if (!e) {
            const Words8 root = taproot_walk(hd_load_cc(leaf32, i), path32, i * max_depth, d);
            U256 qx = u256_zero();
            u32 parity = 0;
            e = taproot_finish_pub(T, P, taproot_tweak(pk, true, root), qx, parity);
            ok = !e && parity == want_parity && u256_eq(qx, schnorr_load_be(out_pk32 + 32 * i));   // (an out_pk >= p never matches)
        }
    }
    valid[i] = ok ? 1 : 0;
    return e;
}

#if defined(__HIPCC__)
// thread g owns element g
template <int UNUSED = 0>   // (templates so that every translation unit that includes this file may hold the definitions)
__global__ __launch_bounds__(256) void k_taproot_leaf_hash(const uint8_t* leaf_version, const uint8_t* script, const uint64_t* offsets,
                                                           uint8_t* leaf32, size_t count, uint8_t* err, unsigned long long* counter) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    uint8_t e = 0;
    if (i < count) {
        e = body_taproot_leaf_hash(leaf_version, script, offsets, leaf32, i);
        err[i] = e;
    }
    sign_count_err(e, counter);
}
template <int UNUSED = 0>
__global__ __launch_bounds__(256) void k_taproot_merkle_root(const uint8_t* leaf32, const uint8_t* path32, const uint8_t* depth,
                                                             size_t max_depth, uint8_t* root32, size_t count, uint8_t* err,
                                                             unsigned long long* counter) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    uint8_t e = 0;
    if (i < count) {
        e = body_taproot_merkle_root(leaf32, path32, depth, max_depth, root32, i);
        err[i] = e;
    }
    sign_count_err(e, counter);
}
template <int UNUSED = 0>
__global__ __launch_bounds__(256) void k_taproot_tweak_pubkey(const Aff* T, const uint8_t* pk32, const uint8_t* root32, uint8_t* out_pk32,
                                                              uint8_t* out_parity, size_t count, uint8_t* err,
                                                              unsigned long long* counter) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    uint8_t e = 0;
    if (i < count) {
        e = body_taproot_tweak_pubkey(T, pk32, root32, out_pk32, out_parity, i);
        err[i] = e;
    }
    sign_count_err(e, counter);
}
template <int UNUSED = 0>
__global__ __launch_bounds__(256) void k_taproot_tweak_seckey(const Aff* T, const uint8_t* sk32, const uint8_t* root32, uint8_t* out_sk32,
                                                              size_t count, uint8_t* err, unsigned long long* counter) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    uint8_t e = 0;
    if (i < count) {
        e = body_taproot_tweak_seckey(T, sk32, root32, out_sk32, i);
        err[i] = e;
    }
    sign_count_err(e, counter);
}
template <int UNUSED = 0>
__global__ __launch_bounds__(256) void k_taproot_verify_commitment(const Aff* T, const uint8_t* out_pk32, const uint8_t* out_parity,
                                                                   const uint8_t* pk32, const uint8_t* leaf32, const uint8_t* path32,
                                                                   const uint8_t* depth, size_t max_depth, size_t count, uint8_t* err,
                                                                   uint8_t* valid, unsigned long long* counter) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    uint8_t e = 0;
    if (i < count) {
        e = body_taproot_verify_commitment(T, out_pk32, out_parity, pk32, leaf32, path32, depth, max_depth, valid, i);
        err[i] = e;
    }
    sign_count_err(e, counter);
}
#endif

}  // namespace p2e

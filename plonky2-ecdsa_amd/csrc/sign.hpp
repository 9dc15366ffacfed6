// The two native functions of curve/ecdsa.rs that produce signatures, for a batch, on either curve:
//   ECDSASecretKey::to_public  (curve/ecdsa.rs:16-20)   pk = sk G
//   sign_message               (curve/ecdsa.rs:25-40)   R = k G, r = R.x mod n, s = k^-1 (msg + r sk) mod n,
//                                                       with the nonce k as an INPUT (the reference draws it)
// (verify_message, :42-62, is p2e_ecdsa_verify_batch / p2e_p256_verify_batch.)
//
// Inputs.  sk, msg and k are 32-byte little-endian values, taken modulo n with ONE conditional subtraction (both group
// orders are above 2^255, so 2 n > 2^256 and one subtraction is a full reduction).  The reference's arguments are field
// elements (Secp256K1Scalar / P256Scalar) and cannot hold anything else; for a raw value below 2^256 this is what
// from_noncanonical_biguint yields.  Nothing below 2^256 is flagged for being >= n.
//
// k G through the circuit's fixed-base table T[w][d] = d 16^w G, d = 1..15 (gadgets/curve_fixed_base.rs:24-30):
//     k G = sum over the 64 nibbles d_w of k of T[w][d_w],
// no doublings.  Slot 0 of every window holds a COPY OF SLOT 1 (the circuit's quirk, gadgets/curve_fixed_base.rs:45-56:
// its conditional add fetches the entry first and discards the sum afterwards); here a zero digit adds nothing and slot
// 0 is never taken for "zero" -- it is fetched (the fetch of window w + 1 is issued before the addition of window w, as
// in body_fb_windows_quad) and dropped by the select on the digit.
//
// Two plans:
//   lane  (body_base_mul)       one lane per scalar: the first non-zero digit's entry, then one mixed Jacobian addition
//                               per further non-zero digit -- a 64-deep dependent chain;
//   quad  (body_base_mul_quad)  four lanes per scalar: role j sums windows 16 j .. 16 j + 15 into its own partial sum
//                               (possibly EMPTY = the point at infinity: an explicit flag, no coordinates), then two
//                               levels of general additions, (P0 + P1) + (P2 + P3), the operands exchanged inside the
//                               quad by DPP quad_perm moves (no LDS, no barrier).  The lower window range is always the
//                               first operand, so both lanes of a pair compute the same limbs and after the second
//                               level all four lanes hold the same result; role 0 inverts and stores.
// secp256k1 computes on lazy 29-bit limbs (jac_add29), P-256 on fe.hpp's canonical words (jac_add_cv<P256, ...>).
//
// Why the incomplete addition formulas suffice.  Every addition done here -- the running sum of windows [a, w) plus
// T[w][d_w] in either plan, P0 + P1, P2 + P3 and (P0 + P1) + (P2 + P3) in the quad plan -- adds u G and v G where u and
// v are the integers spelled by two DISJOINT, non-empty-valued digit ranges of one canonical scalar k < n (an operand
// whose digits are all zero is an empty sum and is not added: the flag selects the other operand).  The digit ranges are
// disjoint and both values non-zero, so u != v as integers, and 0 < u, v and u + v <= k < n.  Hence u != v (mod n) -- no
// doubling -- and u + v != 0 (mod n) -- no point at infinity: h = U2 - U1 != 0 in every addition and Z3 != 0.
// Independently of that argument, the result's Z is tested before it is inverted: Z3 = Z1 Z2 h carries a zero of any
// earlier addition to the end, so a zero Z of a NON-EMPTY sum sets P2E_ERR_INVERSE_OF_ZERO and writes zeros -- never a
// silent wrong point.
//
// Exceptional inputs:
//   sk = 0 (mod n)   to_public returns AffinePoint::ZERO (curve/curve_types.rs:163-171), which 64 bytes cannot express:
//                    zeros are written and P2E_ERR_POINT_AT_INFINITY is set.
//   k = 0 (mod n)    the reference redraws its nonce (curve/ecdsa.rs:29-32: the zero point's x is 0); the nonce is an
//                    input here: P2E_ERR_INVERSE_OF_ZERO, zeros written.
//   r = 0 or s = 0   returned as computed and NOT flagged, exactly as sign_message returns them.  Such a signature
//                    does not verify (the verifier inverts s; r = 0 never equals an x coordinate's residue check).
#pragma once
#include "ec29.hpp"
#include "pipeline.hpp"

namespace p2e {

constexpr uint8_t ERR_POINT_AT_INFINITY = 64;   // include/p2e.h P2E_ERR_POINT_AT_INFINITY
constexpr int SIGN_PLAN_AUTO = 0, SIGN_PLAN_LANE = 1, SIGN_PLAN_QUAD = 2;
constexpr int SIGN_WINDOWS = 64;   // nibbles of a 256-bit scalar (the table has FB_WINDOWS = 66 rows: two spare)

// the accumulator's arithmetic: lazy limbs where the curve has them, canonical words otherwise
template <class CV, bool LAZY = LazyLimbs<CV>::available>
struct SignArith;
template <class CV>
struct SignArith<CV, false> {
    typedef Jac Pt;
    P2E_HD static Pt from_aff(const Aff& a) { return jac_from_aff(a); }
    P2E_HD static Pt zero() {
        Pt r;
        r.X = r.Y = r.Z = u256_zero();
        return r;
    }
    P2E_HD static Pt add_mixed(const Pt& p, const Pt& q) { return jac_add_cv<CV, false, true>(p, q).p; }
    P2E_HD static Pt add(const Pt& p, const Pt& q) { return jac_add_cv<CV, false, false>(p, q).p; }
    P2E_HD static Pt dbl(const Pt& p) { return jac_dbl_cv<CV>(p).p; }   // (recover.hpp; nothing in this file doubles)
    P2E_HD static Pt select(bool c, const Pt& t, const Pt& f) {
        Pt r;
        r.X = u256_select(c, t.X, f.X);
        r.Y = u256_select(c, t.Y, f.Y);
        r.Z = u256_select(c, t.Z, f.Z);
        return r;
    }
    P2E_HD static Jac canon(const Pt& p) { return p; }
#if defined(__HIP_DEVICE_COMPILE__)
    template <int SEL>
    __device__ __forceinline__ static U256 xchg1(const U256& v) {
        U256 r;
        P2E_UNROLL
        for (int k = 0; k < 8; k++) r.w[k] = (u32)__builtin_amdgcn_mov_dpp((int)v.w[k], SEL, 0xF, 0xF, true);
        return r;
    }
    template <int SEL>
    __device__ __forceinline__ static Pt xchg(const Pt& p) {
        Pt r;
        r.X = xchg1<SEL>(p.X);
        r.Y = xchg1<SEL>(p.Y);
        r.Z = xchg1<SEL>(p.Z);
        return r;
    }
#endif
};
template <class CV>
struct SignArith<CV, true> {
    typedef JacL Pt;
    P2E_HD static Pt from_aff(const Aff& a) {
        Pt r;
        r.X = f29_from_u256(a.x);
        r.Y = f29_from_u256(a.y);
        r.Z = f29_small(1);
        return r;
    }
    P2E_HD static Pt zero() {
        Pt r;
        r.X = r.Y = r.Z = f29_small(0);
        return r;
    }
    // (operands and results: tight limbs -- X3, Y3 leave jac_add29 through f29_norm, Z3 through a multiplication)
    P2E_HD static Pt add_mixed(const Pt& p, const Pt& q) { return jac_add29<false, true>(p, q).p; }
    P2E_HD static Pt add(const Pt& p, const Pt& q) { return jac_add29<false, false>(p, q).p; }
    P2E_HD static Pt dbl(const Pt& p) { return jac_dbl29(p).p; }
    P2E_HD static Pt select(bool c, const Pt& t, const Pt& f) {
        Pt r;
        r.X = f29_select(c, t.X, f.X);
        r.Y = f29_select(c, t.Y, f.Y);
        r.Z = f29_select(c, t.Z, f.Z);
        return r;
    }
    P2E_HD static Jac canon(const Pt& p) { return jacl_canon(p); }
#if defined(__HIP_DEVICE_COMPILE__)
    template <int SEL>
    __device__ __forceinline__ static F29 xchg1(const F29& v) {
        F29 r;
        P2E_UNROLL
        for (int k = 0; k < 9; k++) r.l[k] = (u32)__builtin_amdgcn_mov_dpp((int)v.l[k], SEL, 0xF, 0xF, true);
        return r;
    }
    template <int SEL>
    __device__ __forceinline__ static Pt xchg(const Pt& p) {
        Pt r;
        r.X = xchg1<SEL>(p.X);
        r.Y = xchg1<SEL>(p.Y);
        r.Z = xchg1<SEL>(p.Z);
        return r;
    }
#endif
};

// a sum of table entries: `have` = not empty (empty = the point at infinity, p is then meaningless)
template <class CV>
struct SignSum {
    typename SignArith<CV>::Pt p;
    bool have;
};

// 32-byte little-endian scalar -> its residue modulo n (see the header: one conditional subtraction)
template <class CV>
P2E_HD U256 sign_scalar(const uint8_t* base, size_t i) {
    return fe_canon<typename CV::Fn>(load_packed(base, i));
}
P2E_HD void store_packed(uint8_t* base, size_t i, const U256& v) {
    u32* p = reinterpret_cast<u32*>(base + 32 * i);
    P2E_UNROLL
    for (int k = 0; k < 8; k++) p[k] = v.w[k];
}

// sum of T[w0 + t][digit t of d], t = 0 .. 8 WORDS - 1, the non-zero digits only.  d (WORDS little-endian words) is
// consumed: the digit is always the low nibble of d[0] and the words move down four bits per window, so every index is
// a compile-time constant and the scalar stays in registers while the loop stays rolled (one addition of code).
// The entry of window t + 1 is fetched before the addition of window t; the last fetch reads row w0 + 8 WORDS <= 64 of
// the table's 66 rows with digit 0 and is dropped.
template <class CV, int WORDS>
P2E_HD SignSum<CV> sign_window_sum(const Aff* T, u32 (&d)[WORDS], int w0) {
    typedef SignArith<CV> A;
    auto next_digit = [&]() {
        const u32 v = d[0] & 15u;
        P2E_UNROLL
        for (int k = 0; k + 1 < WORDS; k++) d[k] = (d[k] >> 4) | (d[k + 1] << 28);
        d[WORDS - 1] >>= 4;
        return v;
    };
    SignSum<CV> s;
    s.p = A::zero();
    s.have = false;
    u32 d_cur = next_digit();
    Aff p_cur = T[(size_t)w0 * 16 + d_cur];
    for (int t = 0; t < 8 * WORDS; t++) {
        const u32 d_nxt = next_digit();   // (zero once the words have run out)
        const Aff p_nxt = T[(size_t)(w0 + t + 1) * 16 + d_nxt];
        const typename A::Pt e = A::from_aff(p_cur);
        const typename A::Pt sum = A::add_mixed(s.p, e);   // (on an empty s.p: computed on zeros and dropped)
        const bool take = d_cur != 0;
        s.p = A::select(take, A::select(s.have, sum, e), s.p);
        s.have = s.have || take;
        d_cur = d_nxt;
        p_cur = p_nxt;
    }
    return s;
}

// lo + hi, lo being the sum over the LOWER window range (the operand order is part of the result's limbs)
template <class CV>
P2E_HD SignSum<CV> sign_sum_add(const SignSum<CV>& lo, const SignSum<CV>& hi) {
    typedef SignArith<CV> A;
    SignSum<CV> r;
    const typename A::Pt sum = A::add(lo.p, hi.p);
    r.p = A::select(lo.have && hi.have, sum, A::select(lo.have, lo.p, hi.p));
    r.have = lo.have || hi.have;
    return r;
}

// k G, lane per scalar (k < n canonical)
template <class CV>
P2E_HD SignSum<CV> body_base_mul(const Aff* T, const U256& k) {
    u32 d[8];
    P2E_UNROLL
    for (int j = 0; j < 8; j++) d[j] = k.w[j];
    return sign_window_sum<CV, 8>(T, d, 0);
}

#if defined(__HIP_DEVICE_COMPILE__)
// the partner's sum (lane ^ 1: quad_perm [1,0,3,2] = 0xB1; lane ^ 2: quad_perm [2,3,0,1] = 0x4E), ordered by role
template <class CV, int SEL, int BIT>
__device__ __forceinline__ SignSum<CV> sign_quad_level(int role, const SignSum<CV>& mine) {
    typedef SignArith<CV> A;
    SignSum<CV> other;
    other.p = A::template xchg<SEL>(mine.p);
    other.have = __builtin_amdgcn_mov_dpp((int)mine.have, SEL, 0xF, 0xF, true) != 0;
    const bool upper = (role & BIT) != 0;   // this lane holds the upper window range of the pair
    SignSum<CV> lo, hi;
    lo.p = A::select(upper, other.p, mine.p);
    hi.p = A::select(upper, mine.p, other.p);
    lo.have = upper ? other.have : mine.have;
    hi.have = upper ? mine.have : other.have;
    return sign_sum_add<CV>(lo, hi);
}
#endif

// k G, four lanes per scalar: this lane is role `role` of its quad; every lane returns the full sum.
// Host (emulation) form: one caller computes the four partial sums and the same two levels in the same operand order.
template <class CV>
P2E_HD SignSum<CV> body_base_mul_quad(const Aff* T, const U256& k, int role) {
#if defined(__HIP_DEVICE_COMPILE__)
    u32 d[2];
    d[0] = role == 0 ? k.w[0] : role == 1 ? k.w[2] : role == 2 ? k.w[4] : k.w[6];
    d[1] = role == 0 ? k.w[1] : role == 1 ? k.w[3] : role == 2 ? k.w[5] : k.w[7];
    SignSum<CV> s = sign_window_sum<CV, 2>(T, d, 16 * role);
    s = sign_quad_level<CV, 0xB1, 1>(role, s);
    return sign_quad_level<CV, 0x4E, 2>(role, s);
#else
    (void)role;
    SignSum<CV> part[4];
    for (int j = 0; j < 4; j++) {
        u32 d[2] = {k.w[2 * j], k.w[2 * j + 1]};
        part[j] = sign_window_sum<CV, 2>(T, d, 16 * j);
    }
    return sign_sum_add<CV>(sign_sum_add<CV>(part[0], part[1]), sign_sum_add<CV>(part[2], part[3]));
#endif
}

template <class CV, int PLAN>
P2E_HD SignSum<CV> sign_base_mul(const Aff* T, const U256& k, int role) {
    if (PLAN == SIGN_PLAN_QUAD) return body_base_mul_quad<CV>(T, k, role);
    return body_base_mul<CV>(T, k);
}

// affine x (and y) of a non-empty sum through one safegcd inversion of Z; false: Z == 0 (see the header)
template <class CV, bool WANT_Y>
P2E_HD bool sign_to_affine(const SignSum<CV>& s, U256& x, U256& y) {
    typedef typename CV::Fp F;
    const Jac j = SignArith<CV>::canon(s.p);
    U256 zi;
    if (!fe_inv_safegcd<F>(j.Z, zi)) return false;
    const U256 zi2 = fe_sqr<F>(zi);
    x = fe_mul<F>(j.X, zi2);
    if (WANT_Y) y = fe_mul<F>(j.Y, fe_mul<F>(zi2, zi));
    return true;
}

// to_public of element i; the returned err byte is meaningful (and the outputs are written) in role 0 only
// (include/p2e.h BUFFER OVERLAP relies on this body reading every input of element i before its first store)
template <class CV, int PLAN>
P2E_HD uint8_t body_public_key(const Aff* T, const uint8_t* sk32, uint8_t* pkx32, uint8_t* pky32, size_t i, int role) {
    const U256 sk = sign_scalar<CV>(sk32, i);
    const SignSum<CV> s = sign_base_mul<CV, PLAN>(T, sk, role);
    if (role != 0) return 0;
    uint8_t e = 0;
    U256 x = u256_zero(), y = u256_zero();
    if (!s.have) {
        e = ERR_POINT_AT_INFINITY;
    } else if (!sign_to_affine<CV, true>(s, x, y)) {
        e = ERR_INVERSE_OF_ZERO;
        x = y = u256_zero();
    }
    store_packed(pkx32, i, x);
    store_packed(pky32, i, y);
    return e;
}

// sign_message of element i with nonce k32[i].  RECOVERABLE: also v8[i] = (R.y & 1) | (R.x >= n ? 2 : 0), what
// recover.hpp needs to find R again (0 where flagged); r, s and the err byte are those of the plain form.
// (include/p2e.h BUFFER OVERLAP relies on this body reading every input of element i before its first store)
template <class CV, int PLAN, bool RECOVERABLE = false>
P2E_HD uint8_t body_sign(const Aff* T, const uint8_t* msg32, const uint8_t* sk32, const uint8_t* k32, uint8_t* r32, uint8_t* s32,
                         size_t i, int role, uint8_t* v8 = nullptr) {
    typedef typename CV::Fn Fn;
    const U256 k = sign_scalar<CV>(k32, i);
    const SignSum<CV> R = sign_base_mul<CV, PLAN>(T, k, role);
    if (role != 0) return 0;
    uint8_t e = 0;
    U256 r = u256_zero(), s = u256_zero(), x, y;
    U256 kinv;
    u32 v = 0;
    if (!R.have || !fe_inv_safegcd<Fn>(k, kinv)) {   // k = 0 (mod n): both at once
        e = ERR_INVERSE_OF_ZERO;
    } else if (!sign_to_affine<CV, RECOVERABLE>(R, x, y)) {
        e = ERR_INVERSE_OF_ZERO;
    } else {
        const U256 sk = sign_scalar<CV>(sk32, i), msg = sign_scalar<CV>(msg32, i);
        r = fe_canon<Fn>(x);   // base_to_scalar (curve/curve_types.rs:280-282): x < p < 2 n
        s = fe_mul<Fn>(kinv, fe_add<Fn>(msg, fe_mul<Fn>(r, sk)));
        if (RECOVERABLE) v = (y.w[0] & 1u) | (geq_mod<Fn>(x.w) ? 2u : 0u);
    }
    store_packed(r32, i, r);
    store_packed(s32, i, s);
    if (RECOVERABLE) v8[i] = (uint8_t)v;
    return e;
}

#if defined(__HIPCC__)
// PLAN = SIGN_PLAN_LANE: thread g owns element g; SIGN_PLAN_QUAD: the four consecutive threads 4 i .. 4 i + 3 own
// element i (a quad never straddles the end of the batch: its four lanes run or idle together).
__device__ __forceinline__ void sign_count_err(uint8_t e, unsigned long long* counter) {
    const unsigned long long m = __ballot(e != 0);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(counter, (unsigned long long)__popcll(m));
}
template <class CV, int PLAN>
__global__ __launch_bounds__(256) void k_public_key(const Aff* T, const uint8_t* sk32, uint8_t* pkx32, uint8_t* pky32, size_t n,
                                                    uint8_t* err, unsigned long long* counter) {
    const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t i = PLAN == SIGN_PLAN_QUAD ? g >> 2 : g;
    const int role = PLAN == SIGN_PLAN_QUAD ? (int)(g & 3) : 0;
    uint8_t e = 0;
    if (i < n) {
        e = body_public_key<CV, PLAN>(T, sk32, pkx32, pky32, i, role);
        if (role == 0) err[i] = e;
    }
    sign_count_err(e, counter);
}
template <class CV, int PLAN>
__global__ __launch_bounds__(256) void k_sign(const Aff* T, const uint8_t* msg32, const uint8_t* sk32, const uint8_t* k32, uint8_t* r32,
                                              uint8_t* s32, size_t n, uint8_t* err, unsigned long long* counter) {
    const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t i = PLAN == SIGN_PLAN_QUAD ? g >> 2 : g;
    const int role = PLAN == SIGN_PLAN_QUAD ? (int)(g & 3) : 0;
    uint8_t e = 0;
    if (i < n) {
        e = body_sign<CV, PLAN>(T, msg32, sk32, k32, r32, s32, i, role);
        if (role == 0) err[i] = e;
    }
    sign_count_err(e, counter);
}
// k_sign with the recovery byte (body_sign<CV, PLAN, true>)
template <class CV, int PLAN>
__global__ __launch_bounds__(256) void k_sign_recoverable(const Aff* T, const uint8_t* msg32, const uint8_t* sk32, const uint8_t* k32,
                                                          uint8_t* r32, uint8_t* s32, uint8_t* v8, size_t n, uint8_t* err,
                                                          unsigned long long* counter) {
    const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t i = PLAN == SIGN_PLAN_QUAD ? g >> 2 : g;
    const int role = PLAN == SIGN_PLAN_QUAD ? (int)(g & 3) : 0;
    uint8_t e = 0;
    if (i < n) {
        e = body_sign<CV, PLAN, true>(T, msg32, sk32, k32, r32, s32, i, role, v8);
        if (role == 0) err[i] = e;
    }
    sign_count_err(e, counter);
}
#endif

}  // namespace p2e

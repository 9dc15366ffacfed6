// Public-key recovery from (msg, r, s, v), for a batch, on either curve: the fourth corner next to sign.hpp's to_public and
// sign_message and the verifiers.  (msg, r, s, v) on the device becomes (msg, r, s, pk), the input of the witness fill.
//     R  = the curve point with x = r + n (v >> 1) and y = v & 1 (mod 2)
//     pk = r^-1 (s R - msg G) = u1 G + u2 R,   u1 = -msg r^-1,  u2 = s r^-1  (mod n)
//
// Inputs.  msg is taken modulo n with one conditional subtraction, exactly as the signer takes it (reduced, not flagged).
// r and s are NOT reduced: r = 0, r >= n, s = 0, s >= n, v > 3, x >= p, or an x for which x^3 + a x + b is no square, set
// ERR_NOT_RECOVERABLE.  v carries no offset (Ethereum's 27 or the EIP-155 term is the caller's to subtract).
//
// Per element, one lane:
//   1. range checks; r^-1 mod n by safegcd; u1, u2.
//   2. decompression: t = x^3 + a x + b, y = t^((p + 1) / 4) (both primes are 3 mod 4) through one fixed addition chain per
//      curve (recover_sqrt), y^2 == t tested on canonical values, y negated when its parity is not v & 1.
//   3. u2 R: 128 fixed 2-bit windows, most significant first; the table {R, 2 R, 3 R} stays in registers (2 R = dbl(R),
//      3 R = 2 R + R, a mixed addition since R is affine).  A window is two doublings and one addition of the entry the
//      digit selects; leading zero digits leave an explicit "empty" flag set, as SignSum does.  The selected entry goes
//      through ONE general addition (R as a Jacobian point with Z = 1): the lanes of a wave hold different digits, so a
//      separate mixed-addition path for digit 1 would be executed by every wave in addition to the general one.
//      (2 bits: a 4-bit table is 15 points per lane -- in registers it would spill to the private segment, which no kernel
//      of this library uses; in LDS it would limit a CU to about two waves.)
//   4. u1 G: sign.hpp's sign_base_mul<CV, SIGN_PLAN_LANE>, unchanged.
//   5. A + B, A = u1 G, B = u2 R: the only addition whose operands are unrelated.  Both zero tests are explicit, on
//      canonical values: A empty (msg = 0 mod n) -> B;  h != 0 -> the ordinary sum;  h = 0 and r = 0 -> dbl(B);
//      h = 0 and r != 0 -> the neutral element: ERR_POINT_AT_INFINITY (s R = msg G).  Then one inversion of Z and the
//      stores.  jac_add29 / jac_add_cv are used as they are (for the ordinary sum only).
// secp256k1 computes on lazy 29-bit limbs, P-256 on fe.hpp's canonical words: RecField<CV> is the field-element sibling
// of SignArith<CV>, which supplies the point formulas (plus `dbl`, added there).
//
// Why steps 3 and 4 need no exceptional handling.  R is a point of the curve, both curves have cofactor 1, so R has prime
// order n (it is not the neutral element: it has coordinates).  Table: 2 R = dbl(R) has Z = 2 y != 0 because a point of
// odd order has y != 0; 3 R = 2 R + R adds two different points that are not opposite (n > 3).  Walk: after any prefix
// with a non-zero digit the accumulator is m R with m >= 1; the window step doubles twice -- doubling a point of odd
// prime order never yields the neutral element -- and adds d R with 1 <= d <= 3 < 4 m, where 4 m + d <= u2 < n.  So
// 4 m != d and 4 m + d != 0 (mod n): no doubling and no neutral element inside the walk.  Step 4 is sign.hpp's argument.
// Independently of that argument, a zero Z at the end sets ERR_INVERSE_OF_ZERO and writes zeros -- never a silent wrong
// point (Z3 = Z1 Z2 h and Z3 = 2 Y Z carry a zero of any earlier step to the end).
//
// The recoverable signer (sign.hpp body_sign<CV, PLAN, true>) writes the v this file reads:
// v = (R.y & 1) | (R.x >= n ? 2 : 0).
#pragma once
#include "sign.hpp"

namespace p2e {

constexpr uint8_t ERR_NOT_RECOVERABLE = 128;   // include/p2e.h P2E_ERR_NOT_RECOVERABLE
constexpr int RECOVER_WINDOWS = 128;           // 2-bit digits of a 256-bit scalar

// base-field elements in the accumulator's representation (SignArith<CV>::Pt's coordinates): operands and results tight
template <class CV, bool LAZY = LazyLimbs<CV>::available>
struct RecField;
template <class CV>
struct RecField<CV, false> {
    typedef U256 E;
    typedef typename CV::Fp F;
    P2E_HD static E from(const U256& a) { return a; }
    P2E_HD static U256 canon(const E& a) { return a; }
    P2E_HD static E mul(const E& a, const E& b) { return fe_mul<F>(a, b); }
    P2E_HD static E sqr(const E& a) { return fe_sqr<F>(a); }
    P2E_HD static E sub(const E& a, const E& b) { return fe_sub<F>(a, b); }
};
template <class CV>
struct RecField<CV, true> {
    typedef F29 E;
    P2E_HD static E from(const U256& a) { return f29_from_u256(a); }
    P2E_HD static U256 canon(const E& a) { return f29_canon(a); }
    P2E_HD static E mul(const E& a, const E& b) { return f29_mul_call(a, b); }
    P2E_HD static E sqr(const E& a) { return f29_sqr_call(a); }
    P2E_HD static E sub(const E& a, const E& b) { return f29_norm(f29_sub<1>(a, b)); }
};

template <class FA>
P2E_HD typename FA::E recover_sqr_n(typename FA::E x, int n) {
    for (int i = 0; i < n; i++) x = FA::sqr(x);
    return x;
}
// t^((p + 1) / 4): a square root of t if t is a square (the caller checks).  One fixed chain per curve.
template <class CV>
P2E_HD typename RecField<CV>::E recover_sqrt(const typename RecField<CV>::E& t) {
    typedef RecField<CV> FA;
    typedef typename FA::E E;
    const E x2 = FA::mul(FA::sqr(t), t);   // x_k = t^(2^k - 1)
    if (CV::kAZero) {
        // secp256k1: (p + 1) / 4 = 2^254 - 2^30 - 244 = [223 ones] 0 [22 ones] 0000 11 00
        const E x3 = FA::mul(FA::sqr(x2), t);
        const E x6 = FA::mul(recover_sqr_n<FA>(x3, 3), x3);
        const E x9 = FA::mul(recover_sqr_n<FA>(x6, 3), x3);
        const E x11 = FA::mul(recover_sqr_n<FA>(x9, 2), x2);
        const E x22 = FA::mul(recover_sqr_n<FA>(x11, 11), x11);
        const E x44 = FA::mul(recover_sqr_n<FA>(x22, 22), x22);
        const E x88 = FA::mul(recover_sqr_n<FA>(x44, 44), x44);
        const E x176 = FA::mul(recover_sqr_n<FA>(x88, 88), x88);
        const E x220 = FA::mul(recover_sqr_n<FA>(x176, 44), x44);
        const E x223 = FA::mul(recover_sqr_n<FA>(x220, 3), x3);
        E y = FA::mul(recover_sqr_n<FA>(x223, 23), x22);
        y = FA::mul(recover_sqr_n<FA>(y, 6), x2);
        return recover_sqr_n<FA>(y, 2);
    }
    // P-256: (p + 1) / 4 = 2^254 - 2^222 + 2^190 + 2^94 = ((2^32 - 1) 2^128 + 2^96 + 1) 2^94
    const E x4 = FA::mul(recover_sqr_n<FA>(x2, 2), x2);
    const E x8 = FA::mul(recover_sqr_n<FA>(x4, 4), x4);
    const E x16 = FA::mul(recover_sqr_n<FA>(x8, 8), x8);
    const E x32 = FA::mul(recover_sqr_n<FA>(x16, 16), x16);
    E y = FA::mul(recover_sqr_n<FA>(x32, 32), t);
    y = FA::mul(recover_sqr_n<FA>(y, 96), t);
    return recover_sqr_n<FA>(y, 94);
}

// the point with abscissa x (canonical, < p) and ordinate parity `odd`; false: x^3 + a x + b is not a square
template <class CV>
P2E_HD bool recover_decompress(const U256& x, bool odd, Aff& R) {
    typedef typename CV::Fp F;
    typedef RecField<CV> FA;
    U256 t = fe_mul<F>(fe_sqr<F>(x), x);
    if (!CV::kAZero) t = fe_add<F>(t, fe_mul<F>(CV::a(), x));
    t = fe_add<F>(t, CV::b());
    const typename FA::E y = recover_sqrt<CV>(FA::from(t));
    const U256 yc = FA::canon(y);
    const bool ok = u256_eq(FA::canon(FA::sqr(y)), t);
    R.x = x;
    R.y = u256_select(((yc.w[0] & 1u) != 0) != odd, fe_neg<F>(yc), yc);   // (y = 0 cannot occur: no point of order 2)
    return ok;
}

// u2 R for 0 < u2 < n and R of order n (see the header for why the incomplete formulas suffice)
template <class CV>
P2E_HD SignSum<CV> recover_var_mul(const Aff& R, const U256& u2) {
    typedef SignArith<CV> A;
    typedef typename A::Pt Pt;
    const Pt r1 = A::from_aff(R);
    const Pt r2 = A::dbl(r1);
    const Pt r3 = A::add_mixed(r2, r1);
    u32 d[8];
    P2E_UNROLL
    for (int j = 0; j < 8; j++) d[j] = u2.w[j];
    SignSum<CV> s;
    s.p = A::zero();
    s.have = false;
    for (int t = 0; t < RECOVER_WINDOWS; t++) {
        const u32 dig = d[7] >> 30;   // the digit is always the top two bits: the words move up two bits per window
        P2E_UNROLL
        for (int k = 7; k > 0; k--) d[k] = (d[k] << 2) | (d[k - 1] >> 30);
        d[0] <<= 2;
        const Pt q = A::dbl(A::dbl(s.p));   // (on an empty s.p: computed on zeros and dropped)
        const Pt e = A::select(dig == 1, r1, A::select(dig == 2, r2, r3));
        const Pt sum = A::add(q, e);
        const bool take = dig != 0;
        s.p = A::select(s.have, A::select(take, sum, q), A::select(take, e, s.p));
        s.have = s.have || take;
    }
    return s;
}

// A + B for unrelated A (possibly empty) and B (not empty); returns the err bits (0: `out` holds the sum)
template <class CV>
P2E_HD uint8_t recover_final_add(const SignSum<CV>& A_, const typename SignArith<CV>::Pt& B, SignSum<CV>& out) {
    typedef SignArith<CV> A;
    typedef RecField<CV> FA;
    typedef typename FA::E E;
    const E zz1 = FA::sqr(A_.p.Z), zz2 = FA::sqr(B.Z);
    const E u1 = FA::mul(A_.p.X, zz2), u2 = FA::mul(B.X, zz1);
    const E s1 = FA::mul(A_.p.Y, FA::mul(zz2, B.Z)), s2 = FA::mul(B.Y, FA::mul(zz1, A_.p.Z));
    const bool h_zero = u256_is_zero(FA::canon(FA::sub(u2, u1)));   // same x
    const bool r_zero = u256_is_zero(FA::canon(FA::sub(s2, s1)));   // same y
    const typename A::Pt sum = A::add(A_.p, B);
    const typename A::Pt twice = A::dbl(B);
    out.have = true;
    out.p = A::select(!A_.have, B, A::select(h_zero, twice, sum));
    return (A_.have && h_zero && !r_zero) ? ERR_POINT_AT_INFINITY : 0;
}

// x = r + n (hi ? 1 : 0); false: x >= p (or x >= 2^256)
template <class CV>
P2E_HD bool recover_abscissa(const U256& r, bool hi, U256& x) {
    u32 c = 0;
    P2E_UNROLL
    for (int k = 0; k < 8; k++) x.w[k] = addc32(r.w[k], hi ? CV::Fn::m(k) : 0u, c);
    return c == 0 && !geq_mod<typename CV::Fp>(x.w);
}

// recovery of element i; returns its err byte (zeros are written where it is not 0)
// (include/p2e.h BUFFER OVERLAP relies on this body reading every input of element i before its first store)
template <class CV>
P2E_HD uint8_t body_recover(const Aff* T, const uint8_t* msg32, const uint8_t* r32, const uint8_t* s32, const uint8_t* v8,
                            uint8_t* pkx32, uint8_t* pky32, size_t i) {
    typedef typename CV::Fn Fn;
    const U256 r = load_packed(r32, i), s = load_packed(s32, i);
    const u32 v = v8[i];
    uint8_t e = 0;
    U256 px = u256_zero(), py = u256_zero(), x, rinv;
    Aff R;
    if (u256_is_zero(r) || geq_mod<Fn>(r.w) || u256_is_zero(s) || geq_mod<Fn>(s.w) || v > 3u || !recover_abscissa<CV>(r, (v & 2u) != 0, x) ||
        !recover_decompress<CV>(x, (v & 1u) != 0, R) || !fe_inv_safegcd<Fn>(r, rinv)) {
        e = ERR_NOT_RECOVERABLE;
    } else {
        const U256 msg = sign_scalar<CV>(msg32, i);
        const U256 u1 = fe_neg<Fn>(fe_mul<Fn>(msg, rinv)), u2 = fe_mul<Fn>(s, rinv);
        const SignSum<CV> B = recover_var_mul<CV>(R, u2);
        const SignSum<CV> A_ = sign_base_mul<CV, SIGN_PLAN_LANE>(T, u1, 0);
        SignSum<CV> P;
        e = recover_final_add<CV>(A_, B.p, P);
        if (!B.have) e = ERR_INVERSE_OF_ZERO;   // (u2 = 0 needs s = 0 or r^-1 = 0: excluded above)
        if (!e && !sign_to_affine<CV, true>(P, px, py)) e = ERR_INVERSE_OF_ZERO;
        if (e) px = py = u256_zero();
    }
    store_packed(pkx32, i, px);
    store_packed(pky32, i, py);
    return e;
}

#if defined(__HIPCC__)
// thread g owns element g
template <class CV>
__global__ __launch_bounds__(256) void k_recover(const Aff* T, const uint8_t* msg32, const uint8_t* r32, const uint8_t* s32,
                                                 const uint8_t* v8, uint8_t* pkx32, uint8_t* pky32, size_t n, uint8_t* err,
                                                 unsigned long long* counter) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    uint8_t e = 0;
    if (i < n) {
        e = body_recover<CV>(T, msg32, r32, s32, v8, pkx32, pky32, i);
        err[i] = e;
    }
    sign_count_err(e, counter);
}
#endif

}  // namespace p2e

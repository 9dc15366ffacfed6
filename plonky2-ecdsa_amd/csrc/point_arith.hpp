// The native point layer, per element, for a batch, on either curve (include/p2e.h p2e_point_mul_batch,
// p2e_point_lincomb_batch, p2e_point_add_batch):
//   k P            CurveScalar * ProjectivePoint   (curve/curve_multiplication.rs:86-100)
//                  and, on secp256k1, the native glv_mul (curve/glv.rs:84-102)
//   a G + b P      the verification equation with the caller's own scalars (curve/ecdsa.rs:42-62 computes it from a signature)
//   P + Q          the additions of curve/curve_adds.rs
// One lane per element, one kernel per call; no table in LDS, no scratch block, nothing in the private segment.
//
// Inputs.  Scalars are taken modulo n with one conditional subtraction (sign_scalar: reduced, not flagged).  (0, 0) is the
// neutral element and a legal operand; any other point is range-checked and then tested against the curve equation, P
// before Q.  The error byte is a CODE (wire.hpp WIRE_*): WIRE_COORD_RANGE or WIRE_NOT_ON_CURVE for the first failing
// check; WIRE_INFINITY where the operands are fine and the RESULT is the neutral element, which 64 bytes cannot express.
// Every non-zero code writes zeros -- the valid neutral operand of a next call.
//
// Two walks for k P, k != 0 (mod n), P not neutral (both excluded before the walk; P then has prime order n: cofactor 1):
//   PLAIN  recover.hpp's recover_var_mul as it is: 128 two-bit windows, the table {P, 2 P, 3 P} in registers, incomplete
//          additions.  Its no-exception argument needs a point of order n and 0 < k < n, nothing else.
//   GLV    secp256k1 only.  glv_decompose (wit.hpp) writes k = s1 k1 + s2 k2 lambda (mod n), s1, s2 = +-1, and the walk runs
//          over k1 and k2 TOGETHER: per window two doublings, then s1 d1 P and s2 lambda (d2 P) for the two digits.  The
//          lambda-image of a Jacobian point costs one multiplication, lambda (X, Y, Z) = (beta X, Y, Z) (the affine map
//          (x, y) -> (beta x, y) and x = X / Z^2), and a sign is a negated Y, so the one table {P, 2 P, 3 P} serves all four.
//
// The constants.  glv_decompose's basis is v1 = (a1, b1), v2 = (a2, b2) with b1 = -GLV_MINUS_B1, b2 = a1, both in the
// lattice {(x, y): x + y lambda = 0 (mod n)}.  Hence lambda = -a1 / b1 = a1 / GLV_MINUS_B1 (mod n), and beta is the cube
// root of unity mod p with lambda G = (beta G.x, G.y).  tests/test_point_arith_cpu.py recomputes both from these two
// equations with Python integers (they are the values of curve/glv.rs:11-24).
//
// Window count: 64.  glv_decompose computes c1 = round(b2 k / n), c2 = round(-b1 k / n) (glv_round_div: exact rounding to
// nearest) and (k1, k2) = (k, 0) - c1 v1 - c2 v2.  Since a1 b2 - a2 b1 = n, (k, 0) = (b2 k / n) v1 + (-b1 k / n) v2 over
// the rationals, so (k1, k2) = e1 v1 + e2 v2 with |e1|, |e2| <= 1/2:
//     |k1| <= (a1 + a2) / 2   = 0xa2a8918ca85bafe22016d0b917e4dd76 < 2^128,
//     |k2| <= (|b1| + b2) / 2 = 0x8a65287bd47179fb2be08846cea267ec < 2^128.
// Both halves fit 64 two-bit digits.  The CPU build (-DP2E_F29_BOUNDS) aborts on a decomposition that breaks the bound.
//
// The additions of the GLV walk.  The accumulator is (m1 + m2 lambda) P for two signed integers, so recover.hpp's size
// argument (4 m + d <= k < n) does not carry over: whether m1 + m2 lambda meets +-d or +-d lambda modulo n is a statement
// about short lattice vectors, not about sizes.  No such proof is attempted; every addition of the walk is pmsm.hpp's
// COMPLETE msm_add: the neutral element is the explicit `have` flag, h and r are tested on canonical values, equal
// operands are doubled, opposite operands give the neutral element.  A zero Z under `have` at the end (it cannot occur)
// sets WIRE_INFINITY and writes zeros -- never a silent wrong point.
//
// a G + b P: sign.hpp's sign_base_mul<CV, SIGN_PLAN_LANE> for a G, the chosen walk for b P, then ONE complete addition
// (either operand may be empty: a = 0, b = 0, P neutral; a G = b P is doubled; a G = -b P is the neutral element).
// P + Q: one complete mixed addition of the two affine points, then one inversion.
//
// a P + b Q (p2e_point_lincomb2_batch): ONE joint (Straus) walk with one accumulator, one-bit digits over the AFFINE operands.
//   PLAIN  the 128 two-bit windows of a and b together, each window two steps of (double, + P if a's bit, + Q if b's bit).
//   GLV    the four 128-bit halves of the two decompositions together, 128 doublings in all: per step + (+-P), + (+-lambda P),
//          + (+-Q), + (+-lambda Q).  lambda (x, y) = (beta x, y) is one multiplication per operand before the loop.
// Every addition is mixed (Z2 = 1) and COMPLETE (msm_add): with two points the size arguments carry over even less than above
// -- Q may be +-P or +-lambda P, so entries of the two operands coincide or cancel in the middle of the walk.  Nothing but P, Q,
// beta x_P, beta x_Q and the accumulator lives across the loop (174 / 210 VGPRs on secp256k1, two waves per SIMD; two-bit digits
// over two Jacobian tables need 256 + 57 and one wave: NEGATIVE_RESULTS.md section 4).  A wave runs an addition when any lane
// has the bit, so per wave this is 4 x 128 mixed additions under GLV (MEASUREMENTS.md section 24).
// secp256k1 computes on lazy 29-bit limbs, P-256 on canonical words (RecField<CV>); PLAIN, a G + b P and P + Q are one
// text for both.
#pragma once
#include "pmsm.hpp"
#include "wire.hpp"
#include "wit.hpp"

#if defined(P2E_F29_BOUNDS) && !defined(__HIP_DEVICE_COMPILE__)
#include <cstdio>
#include <cstdlib>
#endif

namespace p2e {

constexpr int MUL_PLAN_AUTO = 0, MUL_PLAN_PLAIN = 1, MUL_PLAN_GLV = 2;   // include/p2e.h P2E_MUL_PLAN_*
constexpr int GLV_WINDOWS = 64;                                          // 2-bit digits of |k1|, |k2| < 2^128 (see the header)

// lambda = a1 / GLV_MINUS_B1 (mod n) and beta with lambda G = (beta G.x, G.y): see the header
P2E_HD U256 glv_lambda() {
    U256 r;
    r.w[0] = 0x1b23bd72u, r.w[1] = 0xdf02967cu, r.w[2] = 0x20816678u, r.w[3] = 0x122e22eau;
    r.w[4] = 0x8812645au, r.w[5] = 0xa5261c02u, r.w[6] = 0xc05c30e0u, r.w[7] = 0x5363ad4cu;
    return r;
}
P2E_HD U256 glv_beta() {
    U256 r;
    r.w[0] = 0x719501eeu, r.w[1] = 0xc1396c28u, r.w[2] = 0x12f58995u, r.w[3] = 0x9cf04975u;
    r.w[4] = 0xac3434e9u, r.w[5] = 0x6e64479eu, r.w[6] = 0x657c0710u, r.w[7] = 0x7ae96a2bu;
    return r;
}

// WIRE_OK, WIRE_COORD_RANGE or WIRE_NOT_ON_CURVE of one operand; (0, 0) is the neutral element and fine
template <class CV>
P2E_HD uint8_t point_check(const U256& x, const U256& y, bool& neutral) {
    typedef typename CV::Fp F;
    neutral = u256_is_zero(x) && u256_is_zero(y);
    if (neutral) return WIRE_OK;
    if (geq_mod<F>(x.w) || geq_mod<F>(y.w)) return WIRE_COORD_RANGE;
    return msm_on_curve<CV>(x, y) ? WIRE_OK : WIRE_NOT_ON_CURVE;
}

// table entry `dig` (1 .. 3; anything for 0: dropped by `have`) of {t1, t2, t3}, negated if `neg`, its lambda-image if LAMBDA
template <class CV, bool LAMBDA>
P2E_HD SignSum<CV> glv_entry(const typename SignArith<CV>::Pt& t1, const typename SignArith<CV>::Pt& t2, const typename SignArith<CV>::Pt& t3,
                             u32 dig, bool neg, const typename RecField<CV>::E& beta) {
    typedef SignArith<CV> A;
    typedef RecField<CV> FA;
    SignSum<CV> e;
    e.p = A::select(dig == 1, t1, A::select(dig == 2, t2, t3));
    e.have = dig != 0;
    if (LAMBDA) e.p.X = FA::mul(e.p.X, beta);
    typename A::Pt m = e.p;
    m.Y = FA::sub(FA::from(u256_zero()), e.p.Y);
    e.p = A::select(neg, m, e.p);   // (a register select, as everywhere: no private memory)
    return e;
}

// k P on secp256k1 through the endomorphism, for 0 < k < n and P of order n (see the header); complete additions throughout
template <class CV>
P2E_HD SignSum<CV> point_glv_mul(const Aff& P, const U256& k) {
    typedef SignArith<CV> A;
    typedef typename A::Pt Pt;
    typedef RecField<CV> FA;
    const GlvOut g = glv_decompose(k);
#if defined(P2E_F29_BOUNDS) && !defined(__HIP_DEVICE_COMPILE__)
    if (g.k1.w[4] | g.k1.w[5] | g.k1.w[6] | g.k1.w[7] | g.k2.w[4] | g.k2.w[5] | g.k2.w[6] | g.k2.w[7]) {
        fprintf(stderr, "point_glv_mul: |k1| or |k2| >= 2^128\n");
        abort();
    }
#endif
    const Pt t1 = A::from_aff(P);
    const Pt t2 = A::dbl(t1);              // Z = 2 y != 0: a point of odd order has y != 0
    const Pt t3 = A::add_mixed(t2, t1);    // 2 P != +-P: n > 3
    const typename FA::E beta = FA::from(glv_beta());
    const bool neg1 = g.n1 != 0, neg2 = g.n2 != 0;
    u32 d1[4], d2[4];
    P2E_UNROLL
    for (int j = 0; j < 4; j++) d1[j] = g.k1.w[j], d2[j] = g.k2.w[j];
    SignSum<CV> s = msm_neutral<CV>();
    for (int t = 0; t < GLV_WINDOWS; t++) {
        const u32 dig1 = d1[3] >> 30, dig2 = d2[3] >> 30;   // always the top two bits: the words move up two bits per window
        P2E_UNROLL
        for (int j = 3; j > 0; j--) {
            d1[j] = (d1[j] << 2) | (d1[j - 1] >> 30);
            d2[j] = (d2[j] << 2) | (d2[j - 1] >> 30);
        }
        d1[0] <<= 2;
        d2[0] <<= 2;
        s = msm_dbl<CV>(msm_dbl<CV>(s));
        s = msm_add<CV, false>(s, glv_entry<CV, false>(t1, t2, t3, dig1, neg1, beta));
        s = msm_add<CV, false>(s, glv_entry<CV, true>(t1, t2, t3, dig2, neg2, beta));
    }
    return s;
}

// k P for a checked operand; empty where k = 0 (mod n) or P is the neutral element
template <class CV, int PLAN>
P2E_HD SignSum<CV> point_var_mul(const Aff& P, bool neutral, const U256& k) {
    if (neutral || u256_is_zero(k)) return msm_neutral<CV>();
    if constexpr (PLAN == MUL_PLAN_GLV)
        return point_glv_mul<CV>(P, k);
    else
        return recover_var_mul<CV>(P, k);
}

// ---- a P + b Q: one joint (Straus) walk, one accumulator (see the header) --------------------------------------------------
// the operand `base` (Z = 1) with abscissa x (its own, or beta times it) if `take`, its opposite if `neg`
template <class CV>
P2E_HD SignSum<CV> joint_entry(const typename SignArith<CV>::Pt& base, const typename RecField<CV>::E& x, bool take, bool neg) {
    typedef SignArith<CV> A;
    typedef RecField<CV> FA;
    SignSum<CV> e;
    e.p = base;
    e.p.X = x;
    e.have = take;
    typename A::Pt m = e.p;
    m.Y = FA::sub(FA::from(u256_zero()), base.Y);
    e.p = A::select(neg, m, e.p);   // (a register select, as everywhere: no private memory)
    return e;
}
// the top bit of the WORDS-word value d, which moves up one bit
template <int WORDS>
P2E_HD u32 joint_next_bit(u32 (&d)[WORDS]) {
    const u32 bit = d[WORDS - 1] >> 31;
    P2E_UNROLL
    for (int j = WORDS - 1; j > 0; j--) d[j] = (d[j] << 1) | (d[j - 1] >> 31);
    d[0] <<= 1;
    return bit;
}
// PLAIN: 128 windows of two bits over a and b, each window two steps of (double, + P if a's bit, + Q if b's bit)
template <class CV>
P2E_HD SignSum<CV> point_joint_plain(const Aff& P, bool p_have, const U256& a, const Aff& Q, bool q_have, const U256& b) {
    typedef SignArith<CV> A;
    const typename A::Pt tp = A::from_aff(P), tq = A::from_aff(Q);
    u32 da[8], db[8];
    P2E_UNROLL
    for (int j = 0; j < 8; j++) da[j] = a.w[j], db[j] = b.w[j];
    SignSum<CV> s = msm_neutral<CV>();
    for (int t = 0; t < 2 * RECOVER_WINDOWS; t++) {
        const u32 ba = joint_next_bit<8>(da), bb = joint_next_bit<8>(db);
        s = msm_dbl<CV>(s);
        s = msm_add<CV, true>(s, joint_entry<CV>(tp, tp.X, p_have && ba != 0, false));
        s = msm_add<CV, true>(s, joint_entry<CV>(tq, tq.X, q_have && bb != 0, false));
    }
    return s;
}
P2E_HD void glv_check_halves(const GlvOut& g) {
#if defined(P2E_F29_BOUNDS) && !defined(__HIP_DEVICE_COMPILE__)
    if (g.k1.w[4] | g.k1.w[5] | g.k1.w[6] | g.k1.w[7] | g.k2.w[4] | g.k2.w[5] | g.k2.w[6] | g.k2.w[7]) {
        fprintf(stderr, "point_joint_glv: |k1| or |k2| >= 2^128\n");
        abort();
    }
#else
    (void)g;
#endif
}
// GLV (secp256k1): a = +-a1 +- a2 lambda, b = +-b1 +- b2 lambda; the four halves (< 2^128: the header) walk together, 128
// doublings in all, per step + (+-P), + (+-lambda P), + (+-Q), + (+-lambda Q) for the four bits
template <class CV>
P2E_HD SignSum<CV> point_joint_glv(const Aff& P, bool p_have, const U256& a, const Aff& Q, bool q_have, const U256& b) {
    typedef SignArith<CV> A;
    typedef RecField<CV> FA;
    const GlvOut ga = glv_decompose(a), gb = glv_decompose(b);
    glv_check_halves(ga);
    glv_check_halves(gb);
    const typename A::Pt tp = A::from_aff(P), tq = A::from_aff(Q);
    const typename FA::E beta = FA::from(glv_beta());
    const typename FA::E lpx = FA::mul(tp.X, beta), lqx = FA::mul(tq.X, beta);   // lambda (x, y) = (beta x, y)
    const bool na1 = ga.n1 != 0, na2 = ga.n2 != 0, nb1 = gb.n1 != 0, nb2 = gb.n2 != 0;
    u32 a1[4], a2[4], b1[4], b2[4];
    P2E_UNROLL
    for (int j = 0; j < 4; j++) a1[j] = ga.k1.w[j], a2[j] = ga.k2.w[j], b1[j] = gb.k1.w[j], b2[j] = gb.k2.w[j];
    SignSum<CV> s = msm_neutral<CV>();
    for (int t = 0; t < 2 * GLV_WINDOWS; t++) {
        const u32 x1 = joint_next_bit<4>(a1), x2 = joint_next_bit<4>(a2), y1 = joint_next_bit<4>(b1), y2 = joint_next_bit<4>(b2);
        s = msm_dbl<CV>(s);
        s = msm_add<CV, true>(s, joint_entry<CV>(tp, tp.X, p_have && x1 != 0, na1));
        s = msm_add<CV, true>(s, joint_entry<CV>(tp, lpx, p_have && x2 != 0, na2));
        s = msm_add<CV, true>(s, joint_entry<CV>(tq, tq.X, q_have && y1 != 0, nb1));
        s = msm_add<CV, true>(s, joint_entry<CV>(tq, lqx, q_have && y2 != 0, nb2));
    }
    return s;
}
// a P + b Q for checked operands and a, b < n; a neutral operand (`have` false) and a zero scalar add nothing
template <class CV, int PLAN>
P2E_HD SignSum<CV> point_joint_mul(const Aff& P, bool p_have, const U256& a, const Aff& Q, bool q_have, const U256& b) {
    if constexpr (PLAN == MUL_PLAN_GLV)
        return point_joint_glv<CV>(P, p_have, a, Q, q_have, b);
    else
        return point_joint_plain<CV>(P, p_have, a, Q, q_have, b);
}

// affine coordinates of `s` to element i, zeros where `e` is set or the sum is the neutral element; returns the code
template <class CV>
P2E_HD uint8_t point_finish(uint8_t e, const SignSum<CV>& s, uint8_t* outx32, uint8_t* outy32, size_t i) {
    U256 x = u256_zero(), y = u256_zero();
    if (!e && (!s.have || !sign_to_affine<CV, true>(s, x, y))) {   // (a zero Z under `have` cannot occur: see the header)
        e = WIRE_INFINITY;
        x = y = u256_zero();
    }
    store_packed(outx32, i, x);
    store_packed(outy32, i, y);
    return e;
}

// out_i = k_i P_i; returns the code of element i
// (include/p2e.h BUFFER OVERLAP relies on this body reading every input of element i before its first store)
template <class CV, int PLAN>
P2E_HD uint8_t body_point_mul(const uint8_t* k32, const uint8_t* px32, const uint8_t* py32, uint8_t* outx32, uint8_t* outy32, size_t i) {
    Aff P;
    P.x = load_packed(px32, i), P.y = load_packed(py32, i);
    bool neutral;
    const uint8_t e = point_check<CV>(P.x, P.y, neutral);
    SignSum<CV> s = msm_neutral<CV>();
    if (!e) s = point_var_mul<CV, PLAN>(P, neutral, sign_scalar<CV>(k32, i));
    return point_finish<CV>(e, s, outx32, outy32, i);
}

// out_i = a_i G + b_i P_i (T: the generator's fixed-base table of sign.hpp)
// (include/p2e.h BUFFER OVERLAP relies on this body reading every input of element i before its first store)
template <class CV, int PLAN>
P2E_HD uint8_t body_point_lincomb(const Aff* T, const uint8_t* a32, const uint8_t* b32, const uint8_t* px32, const uint8_t* py32,
                                  uint8_t* outx32, uint8_t* outy32, size_t i) {
    Aff P;
    P.x = load_packed(px32, i), P.y = load_packed(py32, i);
    bool neutral;
    const uint8_t e = point_check<CV>(P.x, P.y, neutral);
    SignSum<CV> s = msm_neutral<CV>();
    if (!e) {
        const SignSum<CV> B = point_var_mul<CV, PLAN>(P, neutral, sign_scalar<CV>(b32, i));
        const SignSum<CV> A_ = sign_base_mul<CV, SIGN_PLAN_LANE>(T, sign_scalar<CV>(a32, i), 0);   // empty for a = 0
        s = msm_add<CV, false>(A_, B);
    }
    return point_finish<CV>(e, s, outx32, outy32, i);
}

// out_i = P_i + Q_i
// (include/p2e.h BUFFER OVERLAP relies on this body reading every input of element i before its first store)
template <class CV>
P2E_HD uint8_t body_point_add(const uint8_t* px32, const uint8_t* py32, const uint8_t* qx32, const uint8_t* qy32, uint8_t* outx32,
                              uint8_t* outy32, size_t i) {
    Aff P, Q;
    P.x = load_packed(px32, i), P.y = load_packed(py32, i);
    Q.x = load_packed(qx32, i), Q.y = load_packed(qy32, i);
    bool p_neutral, q_neutral;
    uint8_t e = point_check<CV>(P.x, P.y, p_neutral);
    const uint8_t eq = point_check<CV>(Q.x, Q.y, q_neutral);
    if (!e) e = eq;
    SignSum<CV> s = msm_neutral<CV>();
    if (!e) {
        SignSum<CV> a, b;
        a.p = SignArith<CV>::from_aff(P), a.have = !p_neutral;
        b.p = SignArith<CV>::from_aff(Q), b.have = !q_neutral;
        s = msm_add<CV, true>(a, b);
    }
    return point_finish<CV>(e, s, outx32, outy32, i);
}

// out_i = a_i P_i + b_i Q_i
// (include/p2e.h BUFFER OVERLAP relies on this body reading every input of element i before its first store)
template <class CV, int PLAN>
P2E_HD uint8_t body_point_lincomb2(const uint8_t* a32, const uint8_t* b32, const uint8_t* px32, const uint8_t* py32, const uint8_t* qx32,
                                   const uint8_t* qy32, uint8_t* outx32, uint8_t* outy32, size_t i) {
    Aff P, Q;
    P.x = load_packed(px32, i), P.y = load_packed(py32, i);
    Q.x = load_packed(qx32, i), Q.y = load_packed(qy32, i);
    const U256 a = sign_scalar<CV>(a32, i), b = sign_scalar<CV>(b32, i);
    bool p_neutral, q_neutral;
    uint8_t e = point_check<CV>(P.x, P.y, p_neutral);
    const uint8_t eq = point_check<CV>(Q.x, Q.y, q_neutral);
    if (!e) e = eq;
    SignSum<CV> s = msm_neutral<CV>();
    if (!e) s = point_joint_mul<CV, PLAN>(P, !p_neutral, a, Q, !q_neutral, b);
    return point_finish<CV>(e, s, outx32, outy32, i);
}

#if defined(__HIPCC__)
// thread g owns element g
template <class CV, int PLAN>
__global__ __launch_bounds__(256) void k_point_lincomb2(const uint8_t* a32, const uint8_t* b32, const uint8_t* px32, const uint8_t* py32,
                                                        const uint8_t* qx32, const uint8_t* qy32, uint8_t* outx32, uint8_t* outy32,
                                                        size_t count, uint8_t* err, unsigned long long* counter) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    uint8_t e = 0;
    if (i < count) {
        e = body_point_lincomb2<CV, PLAN>(a32, b32, px32, py32, qx32, qy32, outx32, outy32, i);
        err[i] = e;
    }
    sign_count_err(e, counter);
}
template <class CV, int PLAN>
__global__ __launch_bounds__(256) void k_point_mul(const uint8_t* k32, const uint8_t* px32, const uint8_t* py32, uint8_t* outx32,
                                                   uint8_t* outy32, size_t n, uint8_t* err, unsigned long long* counter) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    uint8_t e = 0;
    if (i < n) {
        e = body_point_mul<CV, PLAN>(k32, px32, py32, outx32, outy32, i);
        err[i] = e;
    }
    sign_count_err(e, counter);
}
template <class CV, int PLAN>
__global__ __launch_bounds__(256) void k_point_lincomb(const Aff* T, const uint8_t* a32, const uint8_t* b32, const uint8_t* px32,
                                                       const uint8_t* py32, uint8_t* outx32, uint8_t* outy32, size_t n, uint8_t* err,
                                                       unsigned long long* counter) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    uint8_t e = 0;
    if (i < n) {
        e = body_point_lincomb<CV, PLAN>(T, a32, b32, px32, py32, outx32, outy32, i);
        err[i] = e;
    }
    sign_count_err(e, counter);
}
template <class CV>
__global__ __launch_bounds__(256) void k_point_add(const uint8_t* px32, const uint8_t* py32, const uint8_t* qx32, const uint8_t* qy32,
                                                   uint8_t* outx32, uint8_t* outy32, size_t n, uint8_t* err,
                                                   unsigned long long* counter) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    uint8_t e = 0;
    if (i < n) {
        e = body_point_add<CV>(px32, py32, qx32, qy32, outx32, outy32, i);
        err[i] = e;
    }
    sign_count_err(e, counter);
}
#endif

}  // namespace p2e

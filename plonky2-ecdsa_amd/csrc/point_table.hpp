// Point tables: the fixed-base route of sign.hpp for the CALLER'S points (include/p2e.h p2e_point_table_create and the
// three calls that consume a table).  The reference splits a multiplication the same way: mul_precompute /
// mul_with_precomputation (curve/curve_multiplication.rs:18-73) and MsmPrecomputation (curve/curve_msm.rs:19-54).
//
// Layout.  Aff[m][FB_WINDOWS = 66][16], entry [j][w][d] = d 16^w P_j in canonical affine form for d = 1 .. 15, slot 0 a
// copy of slot 1: for every point exactly the generator's table (curve_program.hpp fixed_base_table_cv), so
// sign_window_sum walks it as it is.  Rows 64 and 65 are filled like the others: sign_window_sum prefetches row 64 with
// digit 0 and drops it, so the memory must be there and hold points.  16^w P_j is a point of order n for EVERY w (n is
// prime and does not divide 16^w), so all 66 rows hold ordinary points.
//
// Build, on the device, two kernels:
//   k_table_powers  one lane per point: checks it ((0, 0) -> WIRE_INFINITY: the neutral element has no table; a coordinate
//                   >= p -> WIRE_COORD_RANGE; off the curve -> WIRE_NOT_ON_CURVE), then walks the 4 * 65 doublings and leaves
//                   B_w = 16^w P_j for w = 0 .. 65 in scratch, in the accumulator's own representation (SignArith<CV>::Pt).
//   k_table_rows    one lane per (point, window): B_w made affine (one safegcd inversion), then 2 B = dbl(B) and
//                   d B = (d - 1) B + B for d = 3 .. 15 as mixed additions; each multiple is made affine by its own
//                   inversion as soon as it exists and stored, so a lane holds ONE Jacobian accumulator and B, never the
//                   15 multiples (Montgomery's trick over a lane's 15 entries would keep 15 Jacobian points live: that
//                   is the private segment, which no kernel of this library uses).  15 inversions per lane instead of
//                   one plus 42 multiplications: the build runs once per key set, the calls below run per element.
// The host allocates, launches both on the context's stream and waits; there is no host big-int loop over m.
//
// Why the additions of the build may be incomplete.  P_j is on the curve and not the neutral element; both curves have
// cofactor 1 and prime order n, so B = 16^w P_j has order n.  Doublings: a point of odd order has y != 0, so Z3 = 2 Y Z != 0
// along the whole chain and in 2 B = dbl(B).  Additions: (d - 1) B + B for 3 <= d <= 15 adds c B and B with 2 <= c <= 14;
// c = +-1 (mod n) is impossible for n > 15, so h != 0 and the sum is not the neutral element.  Independently of the
// argument every Z is tested before it is inverted (sign_to_affine): a zero Z -- of B_w, so of any doubling before it
// (Z3 = 2 Y Z carries a zero forward), or of a multiple (Z3 = Z1 h) -- rejects the POINT (WIRE_NOT_ON_CURVE in
// point_err[j]) and the table is not built; it never becomes a silently wrong entry.
//
// The three calls, one lane per element, one kernel per call; no LDS table, nothing in the private segment:
//   mul      k T[idx]              body_base_mul on the point's table: at most 64 mixed additions, no doubling
//   lincomb  a G + b T[idx]        two window sums (the generator's table of the context, the point's table), then ONE
//                                  complete addition (pmsm.hpp msm_add: a G = b P doubles, a G = -b P is the neutral
//                                  element, either half may be empty)
//   verify   the textbook verdict of curve/ecdsa.rs:42-62: c = 1 / s, X = (msg c) G + (r c) P, valid iff X is not the
//            neutral element and X.x mod n == r (base_to_scalar: x < p < 2 n, one conditional subtraction)
// idx == nullptr is point 0 for every element; idx[i] >= m is WIRE_BAD_INDEX, zeros, and the lane reads NO table word.
// The window sums are sign.hpp's, called as they are.  Its no-exception argument (two disjoint non-empty digit ranges of
// one k < n spell u != v with u + v < n) needs a base of order n and nothing else, so it holds for T[idx] as for G.
// The two sums of lincomb / verify run one after the other: on the lazy-limb path every field multiplication is an
// out-of-line call, so two chains woven into one loop would still take turns at every call; weaving them is left unmeasured.
// secp256k1 computes on lazy 29-bit limbs, P-256 on canonical words: one text for both (SignArith<CV> / RecField<CV>).
#pragma once
#include "point_arith.hpp"

namespace p2e {

constexpr uint8_t WIRE_BAD_INDEX = 10;                            // include/p2e.h P2E_WIRE_BAD_INDEX
constexpr size_t TABLE_MAX_POINTS = 65536;                        // include/p2e.h P2E_POINT_TABLE_MAX_POINTS
constexpr size_t TABLE_POINT_ENTRIES = (size_t)FB_WINDOWS * 16;   // entries of one point's table
constexpr size_t TABLE_POW_BYTES = 108;                           // scratch per (point, window): the larger SignArith<CV>::Pt
static_assert(sizeof(Aff) == 64, "table layout");
#if !defined(P2E_F29_BOUNDS)   // (the CPU build with the limb-bound tracker carries bounds inside every limb vector)
static_assert(sizeof(JacL) <= TABLE_POW_BYTES && sizeof(Jac) <= TABLE_POW_BYTES, "scratch layout");
#endif

// checks point j and leaves 16^w P_j, w = 0 .. 65, in pow[j][w]; returns the point's code (nothing written where not 0)
template <class CV>
P2E_HD uint8_t body_table_powers(const uint8_t* px32, const uint8_t* py32, typename SignArith<CV>::Pt* pow, size_t j) {
    typedef SignArith<CV> A;
    Aff P;
    P.x = load_packed(px32, j), P.y = load_packed(py32, j);
    bool neutral;
    const uint8_t e = point_check<CV>(P.x, P.y, neutral);
    if (neutral) return WIRE_INFINITY;
    if (e) return e;
    typename A::Pt b = A::from_aff(P);
    for (int w = 0; w < FB_WINDOWS; w++) {
        pow[j * FB_WINDOWS + w] = b;
        b = A::dbl(A::dbl(A::dbl(A::dbl(b))));   // (the last four are dropped)
    }
    return WIRE_OK;
}

// row g = (point, window) of the table from pow[g]; false: a zero Z (see the header)
template <class CV>
P2E_HD bool body_table_row(const typename SignArith<CV>::Pt* pow, Aff* tab, size_t g) {
    typedef SignArith<CV> A;
    SignSum<CV> s;
    s.p = pow[g];
    s.have = true;
    Aff B;
    if (!sign_to_affine<CV, true>(s, B.x, B.y)) return false;
    Aff* row = tab + g * 16;
    row[0] = B;
    row[1] = B;
    const typename A::Pt b = A::from_aff(B);
    s.p = A::dbl(b);
    bool ok = true;
    for (int d = 2; d < 16; d++) {
        Aff e;
        if (!sign_to_affine<CV, true>(s, e.x, e.y)) {
            ok = false;
            e.x = e.y = u256_zero();
        }
        row[d] = e;
        if (d < 15) s.p = A::add_mixed(s.p, b);
    }
    return ok;
}

// the table of element i's point; WIRE_BAD_INDEX (and T untouched) where idx[i] >= m
P2E_HD uint8_t table_pick(const Aff* tab, const u32* idx, u32 m, size_t i, const Aff*& T) {
    const u32 j = idx ? idx[i] : 0u;
    if (j >= m) return WIRE_BAD_INDEX;
    T = tab + (size_t)j * TABLE_POINT_ENTRIES;
    return WIRE_OK;
}

// out_i = k_i T[idx_i]; returns the code of element i
// (include/p2e.h BUFFER OVERLAP relies on this body reading every input of element i before its first store)
template <class CV>
P2E_HD uint8_t body_table_mul(const Aff* tab, const u32* idx, u32 m, const uint8_t* k32, uint8_t* outx32, uint8_t* outy32, size_t i) {
    const Aff* T = nullptr;
    const uint8_t e = table_pick(tab, idx, m, i, T);
    SignSum<CV> s = msm_neutral<CV>();
    if (!e) s = body_base_mul<CV>(T, sign_scalar<CV>(k32, i));   // empty for k = 0 (mod n)
    return point_finish<CV>(e, s, outx32, outy32, i);
}

// out_i = a_i G + b_i T[idx_i] (G: the generator's table)
// (include/p2e.h BUFFER OVERLAP relies on this body reading every input of element i before its first store)
template <class CV>
P2E_HD uint8_t body_table_lincomb(const Aff* G, const Aff* tab, const u32* idx, u32 m, const uint8_t* a32, const uint8_t* b32,
                                  uint8_t* outx32, uint8_t* outy32, size_t i) {
    const Aff* T = nullptr;
    const uint8_t e = table_pick(tab, idx, m, i, T);
    SignSum<CV> s = msm_neutral<CV>();
    if (!e) {
        const SignSum<CV> B = body_base_mul<CV>(T, sign_scalar<CV>(b32, i));
        const SignSum<CV> A_ = body_base_mul<CV>(G, sign_scalar<CV>(a32, i));
        s = msm_add<CV, false>(A_, B);
    }
    return point_finish<CV>(e, s, outx32, outy32, i);
}

// valid[i] = verdict of signature (r_i, s_i) on msg_i under T[idx_i]; returns the code of element i
template <class CV>
P2E_HD uint8_t body_table_verify(const Aff* G, const Aff* tab, const u32* idx, u32 m, const uint8_t* msg32, const uint8_t* r32,
                                 const uint8_t* s32, uint8_t* valid, size_t i) {
    typedef typename CV::Fn Fn;
    const Aff* T = nullptr;
    uint8_t e = table_pick(tab, idx, m, i, T);
    bool ok = false;
    if (!e) {
        const U256 r = load_packed(r32, i), s = load_packed(s32, i);
        U256 c;
        if (u256_is_zero(r) || geq_mod<Fn>(r.w) || u256_is_zero(s) || geq_mod<Fn>(s.w) || !fe_inv_safegcd<Fn>(s, c)) {
            e = WIRE_SCALAR_RANGE;
        } else {
            const U256 msg = sign_scalar<CV>(msg32, i);
            const SignSum<CV> B = body_base_mul<CV>(T, fe_mul<Fn>(r, c));
            const SignSum<CV> A_ = body_base_mul<CV>(G, fe_mul<Fn>(msg, c));
            const SignSum<CV> X = msm_add<CV, false>(A_, B);
            U256 x = u256_zero(), y;
            if (X.have && sign_to_affine<CV, false>(X, x, y)) ok = u256_eq(fe_canon<Fn>(x), r);
        }
    }
    valid[i] = ok ? 1 : 0;
    return e;
}

#if defined(__HIPCC__)
// thread g owns point g
template <class CV>
__global__ __launch_bounds__(256) void k_table_powers(const uint8_t* px32, const uint8_t* py32, void* pow, size_t m, uint8_t* perr,
                                                      unsigned long long* counter) {
    const size_t j = (size_t)blockIdx.x * 256 + threadIdx.x;
    uint8_t e = 0;
    if (j < m) {
        e = body_table_powers<CV>(px32, py32, (typename SignArith<CV>::Pt*)pow, j);
        perr[j] = e;
    }
    sign_count_err(e, counter);
}
// thread g owns row g = point * 66 + window; the first failing row of a point rejects it (flag[point]: zeroed by the host)
template <class CV>
__global__ __launch_bounds__(256) void k_table_rows(const void* pow, Aff* tab, size_t rows, u32* flag, uint8_t* perr,
                                                    unsigned long long* counter) {
    const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= rows) return;
    if (body_table_row<CV>((const typename SignArith<CV>::Pt*)pow, tab, g)) return;
    const size_t j = g / FB_WINDOWS;
    if (atomicExch(&flag[j], 1u) == 0u) {
        perr[j] = WIRE_NOT_ON_CURVE;
        atomicAdd(counter, 1ull);
    }
}
// thread g owns element g
template <class CV>
__global__ __launch_bounds__(256) void k_table_mul(const Aff* tab, const u32* idx, u32 m, const uint8_t* k32, uint8_t* outx32,
                                                   uint8_t* outy32, size_t n, uint8_t* err, unsigned long long* counter) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    uint8_t e = 0;
    if (i < n) {
        e = body_table_mul<CV>(tab, idx, m, k32, outx32, outy32, i);
        err[i] = e;
    }
    sign_count_err(e, counter);
}
template <class CV>
__global__ __launch_bounds__(256) void k_table_lincomb(const Aff* G, const Aff* tab, const u32* idx, u32 m, const uint8_t* a32,
                                                       const uint8_t* b32, uint8_t* outx32, uint8_t* outy32, size_t n, uint8_t* err,
                                                       unsigned long long* counter) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    uint8_t e = 0;
    if (i < n) {
        e = body_table_lincomb<CV>(G, tab, idx, m, a32, b32, outx32, outy32, i);
        err[i] = e;
    }
    sign_count_err(e, counter);
}
template <class CV>
__global__ __launch_bounds__(256) void k_table_verify(const Aff* G, const Aff* tab, const u32* idx, u32 m, const uint8_t* msg32,
                                                      const uint8_t* r32, const uint8_t* s32, size_t n, uint8_t* err, uint8_t* valid,
                                                      unsigned long long* counter) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    uint8_t e = 0;
    if (i < n) {
        e = body_table_verify<CV>(G, tab, idx, m, msg32, r32, s32, valid, i);
        err[i] = e;
    }
    sign_count_err(e, counter);
}
#endif

}  // namespace p2e

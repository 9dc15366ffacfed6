// Test-only probe of the field and curve-formula layers (csrc/fe.hpp, fe29.hpp, ec.hpp, ec29.hpp, quad.hpp, quad29.hpp).
//
// Every function of those headers the kernels are built from is reachable here as one (op, field) entry of a table:
// `n` elements in, `n` elements out, nothing else.  The file builds twice (tests/probe/Makefile):
//   libp2e_probe.so       hipcc, the library's own flags: one kernel instantiation per (op, field), so the device
//                         branches of the headers (the inline-asm column accumulators, sqr_wide8's doubling, the DPP
//                         exchanges, the noinline calls) run as the product compiles them;
//   libp2e_probe_host.so  g++ -x c++ -DP2E_F29_BOUNDS: the same table through a plain loop, with the limb-bound tracker
//                         of fe29.hpp riding beside every lazy limb (an operand outside a function's contract aborts).
// tests/probe_inputs.py holds the vectors and the big-integer expectations; tests/test_gpu_field_probe.py and
// tests/test_field_probe_cpu.py compare every output byte.  Nothing here is linked into the product library.
//
// Element layout: u32 words, element-major.  A canonical value is 8 words (little-endian), a lazy-limb value 9 limbs.
// Lane-per-element ops: thread i handles element i.  Four-lane ops: threads 4i .. 4i+3 handle element i with role =
// thread & 3 (as k_chains_quad), and each of the four lanes writes its own copy of the whole result.
//
// One source, four translation units on the device (-DP2E_PROBE_PART=0..3, linked into one library) so the build runs
// side by side like csrc/p2e_hip.hip's; without the macro everything is one unit (the host build).
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#endif
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../plonky2-ecdsa_amd/csrc/quad.hpp"

#if defined(P2E_PROBE_PART)
#define PROBE_HAS(k) (P2E_PROBE_PART == (k))
#else
#define PROBE_HAS(k) 1
#endif

namespace probe {
using namespace p2e;

struct Entry {
    const char* name;
    int field, in_words, out_words, lanes, flag;
    long (*run)(const u32*, u32*, size_t, int);
};

P2E_HD U256 ldU(const u32* in, int k) {
    U256 r;
    P2E_UNROLL
    for (int i = 0; i < 8; i++) r.w[i] = in[8 * k + i];
    return r;
}
P2E_HD void stU(u32* out, int k, const U256& v) {
    P2E_UNROLL
    for (int i = 0; i < 8; i++) out[8 * k + i] = v.w[i];
}
// nine raw limbs; the emulation build's bound of a limb is the limb itself: the tracker then checks THIS operand against
// every precondition on its way
P2E_HD F29 ldF(const u32* in, int k) {
    F29 r;
    P2E_UNROLL
    for (int i = 0; i < 9; i++) r.l[i] = in[9 * k + i];
#if P2E_F29_TRACK
    for (int i = 0; i < 9; i++) r.ub[i] = r.l[i];
#endif
    return r;
}
P2E_HD void stF(u32* out, int k, const F29& v) {
    P2E_UNROLL
    for (int i = 0; i < 9; i++) out[9 * k + i] = v.l[i];
}
P2E_HD Jac ldJ(const u32* in, int k) {
    Jac p;
    p.X = ldU(in, k);
    p.Y = ldU(in, k + 1);
    p.Z = ldU(in, k + 2);
    return p;
}
P2E_HD JacL ldJL(const u32* in, int k) {
    JacL p;
    p.X = ldF(in, k);
    p.Y = ldF(in, k + 1);
    p.Z = ldF(in, k + 2);
    return p;
}
P2E_HD u64 ld64(const u32* in, int k) { return (u64)in[2 * k] | ((u64)in[2 * k + 1] << 32); }
P2E_HD void st64(u32* out, int k, u64 v) {
    out[2 * k] = (u32)v;
    out[2 * k + 1] = (u32)(v >> 32);
}

template <class MOD>
struct CurveOf {
    typedef Secp256k1 type;
};
template <>
struct CurveOf<ModP256> {
    typedef P256 type;
};

#if defined(__HIPCC__)
// one instantiation per (op, field): the op is a template parameter, not a switch
template <class OP>
__global__ __launch_bounds__(256) void k_probe(const u32* __restrict__ in, u32* __restrict__ out, size_t n, int flag) {
    const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t i = OP::LANES == 4 ? g >> 2 : g;   // the four lanes of a quad share i: active or inactive together
    if (i < n) {
        u32 a[OP::IN], r[OP::OUT];
        P2E_UNROLL
        for (int k = 0; k < OP::IN; k++) a[k] = in[i * OP::IN + k];
        OP::run((int)(g & 3), flag, a, r);
        u32* const o = out + g * OP::OUT;            // g < LANES * n
        P2E_UNROLL
        for (int k = 0; k < OP::OUT; k++) o[k] = r[k];
    }
}
#endif

template <class OP>
static long run_op(const u32* in, u32* out, size_t n, int flag) {
    if (n == 0) return 0;
#if defined(__HIPCC__)
    const size_t ib = n * OP::IN * sizeof(u32), ob = n * OP::LANES * OP::OUT * sizeof(u32);
    u32 *din = nullptr, *dout = nullptr;
    hipError_t e = hipMalloc((void**)&din, ib);
    if (e == hipSuccess) e = hipMalloc((void**)&dout, ob);
    if (e == hipSuccess) e = hipMemcpy(din, in, ib, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemset(dout, 0xEE, ob);   // a slot no lane wrote shows as such
    if (e == hipSuccess) {
        const size_t threads = n * OP::LANES;
        hipLaunchKernelGGL(k_probe<OP>, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, 0, din, dout, n, flag);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(out, dout, ob, hipMemcpyDeviceToHost);
    if (din) (void)hipFree(din);
    if (dout) (void)hipFree(dout);
    return (long)e;
#else
    for (size_t i = 0; i < n; i++)
        for (int role = 0; role < OP::LANES; role++) OP::run(role, flag, in + i * OP::IN, out + (i * OP::LANES + role) * OP::OUT);
    return 0;
#endif
}

// an op: words in, words out (per lane), lanes per element.  MOD is the field, P an op-specific constant.
#define PROBE_OP(NAME, INW, OUTW, LANESN)                                               \
    template <class MOD, int P>                                                         \
    struct NAME {                                                                       \
        static constexpr int IN = INW, OUT = OUTW, LANES = LANESN;                      \
        P2E_HD static void run(int role, int flag, const u32* in, u32* out) {           \
            (void)role;                                                                 \
            (void)flag;
#define PROBE_END \
    }             \
    }             \
    ;

#define PROBE_E(NAME, OPT, P, MODT, FIELD, FLAG) \
    v.push_back(Entry{NAME, FIELD, OPT<MODT, P>::IN, OPT<MODT, P>::OUT, OPT<MODT, P>::LANES, FLAG, &run_op<OPT<MODT, P>>});
#define PROBE_E4(NAME, OPT, P)          \
    PROBE_E(NAME, OPT, P, ModP, 0, 0)   \
    PROBE_E(NAME, OPT, P, ModN, 1, 0)   \
    PROBE_E(NAME, OPT, P, ModP256, 2, 0) \
    PROBE_E(NAME, OPT, P, ModN256, 3, 0)
// the two base fields (the formulas: field 0 = secp256k1, field 2 = P-256)
#define PROBE_E2(NAME, OPT, P, FLAG)       \
    PROBE_E(NAME, OPT, P, ModP, 0, FLAG)   \
    PROBE_E(NAME, OPT, P, ModP256, 2, FLAG)

// ---- part 0: canonical words, raw products and reductions, Goldilocks --------------------------------------------------
#if PROBE_HAS(0)
PROBE_OP(OpFeMul, 16, 8, 1) stU(out, 0, fe_mul<MOD>(ldU(in, 0), ldU(in, 1))); PROBE_END
PROBE_OP(OpFeSqr, 8, 8, 1) stU(out, 0, fe_sqr<MOD>(ldU(in, 0))); PROBE_END
PROBE_OP(OpFeAdd, 16, 8, 1) stU(out, 0, fe_add<MOD>(ldU(in, 0), ldU(in, 1))); PROBE_END
PROBE_OP(OpFeSub, 16, 8, 1) stU(out, 0, fe_sub<MOD>(ldU(in, 0), ldU(in, 1))); PROBE_END
PROBE_OP(OpFeNeg, 8, 8, 1) stU(out, 0, fe_neg<MOD>(ldU(in, 0))); PROBE_END
PROBE_OP(OpFeCanon, 8, 8, 1) stU(out, 0, fe_canon<MOD>(ldU(in, 0))); PROBE_END
PROBE_OP(OpFeMulSmall, 9, 8, 1) stU(out, 0, fe_mul_small<MOD>(ldU(in, 0), in[8])); PROBE_END
PROBE_OP(OpMulWide, 16, 16, 1) mul_wide<8, 8>(in, in + 8, out); PROBE_END
PROBE_OP(OpSqrWide8, 8, 16, 1) sqr_wide8(in, out); PROBE_END
PROBE_OP(OpReduce16R, 16, 8, 1) reduce16<MOD, false>(in, out, nullptr); PROBE_END
PROBE_OP(OpReduce16RQ, 16, 17, 1) reduce16<MOD, true>(in, out, out + 8); PROBE_END
PROBE_OP(OpBarrettWide, 18, 17, 1) reduce_barrett_wide<MOD, 10, true>(in, out, out + 8); PROBE_END
PROBE_OP(OpGlMul, 4, 2, 1) st64(out, 0, gl_mul(ld64(in, 0), ld64(in, 1))); PROBE_END
PROBE_OP(OpGlAdd, 4, 2, 1) st64(out, 0, gl_add(ld64(in, 0), ld64(in, 1))); PROBE_END
PROBE_OP(OpGlReduce128, 4, 2, 1) st64(out, 0, gl_reduce128(ld64(in, 0), ld64(in, 1))); PROBE_END

void part0(std::vector<Entry>& v) {
    PROBE_E4("fe_mul", OpFeMul, 0)
    PROBE_E4("fe_sqr", OpFeSqr, 0)
    PROBE_E4("fe_add", OpFeAdd, 0)
    PROBE_E4("fe_sub", OpFeSub, 0)
    PROBE_E4("fe_neg", OpFeNeg, 0)
    PROBE_E4("fe_canon", OpFeCanon, 0)
    PROBE_E4("fe_mul_small", OpFeMulSmall, 0)
    PROBE_E("mul_wide", OpMulWide, 0, ModP, 0, 0)
    PROBE_E("sqr_wide8", OpSqrWide8, 0, ModP, 0, 0)
    PROBE_E4("reduce16_r", OpReduce16R, 0)
    PROBE_E4("reduce16_rq", OpReduce16RQ, 0)
    PROBE_E("reduce_barrett_wide", OpBarrettWide, 0, ModP256, 2, 0)
    PROBE_E("reduce_barrett_wide", OpBarrettWide, 0, ModN256, 3, 0)
    PROBE_E("gl_mul", OpGlMul, 0, ModP, 0, 0)
    PROBE_E("gl_add", OpGlAdd, 0, ModP, 0, 0)
    PROBE_E("gl_reduce128", OpGlReduce128, 0, ModP, 0, 0)
}
#else
void part0(std::vector<Entry>& v);
#endif

// ---- part 1: inversion -----------------------------------------------------------------------------------------------
#if PROBE_HAS(1)
PROBE_OP(OpInvSafegcd, 8, 9, 1)
    U256 r;
    const bool ok = fe_inv_safegcd<MOD>(ldU(in, 0), r);
    stU(out, 0, r);
    out[8] = ok ? 1u : 0u;
PROBE_END
PROBE_OP(OpInvBingcd, 8, 9, 1)
    U256 r;
    const bool ok = fe_inv_bingcd<MOD>(ldU(in, 0), r);
    stU(out, 0, r);
    out[8] = ok ? 1u : 0u;
PROBE_END
PROBE_OP(OpInv, 8, 8, 1) stU(out, 0, fe_inv<MOD>(ldU(in, 0))); PROBE_END
PROBE_OP(OpInvFermat, 8, 8, 1) stU(out, 0, fe_inv_fermat<MOD>(ldU(in, 0))); PROBE_END
PROBE_OP(OpInvP, 8, 8, 1) stU(out, 0, fe_inv_p(ldU(in, 0))); PROBE_END
PROBE_OP(OpInvN, 8, 8, 1) stU(out, 0, fe_inv_n(ldU(in, 0))); PROBE_END

void part1(std::vector<Entry>& v) {
    PROBE_E4("fe_inv_safegcd", OpInvSafegcd, 0)
    PROBE_E4("fe_inv_bingcd", OpInvBingcd, 0)
    PROBE_E4("fe_inv", OpInv, 0)
    PROBE_E4("fe_inv_fermat", OpInvFermat, 0)
    PROBE_E("fe_inv_p", OpInvP, 0, ModP, 0, 0)
    PROBE_E("fe_inv_n", OpInvN, 0, ModN, 1, 0)
}
#else
void part1(std::vector<Entry>& v);
#endif

// ---- part 2: lazy limbs (secp256k1 p) and the lane-per-signature formulas ----------------------------------------------
#if PROBE_HAS(2)
PROBE_OP(OpF29From, 8, 9, 1) stF(out, 0, f29_from_u256(ldU(in, 0))); PROBE_END
PROBE_OP(OpF29Norm, 9, 9, 1) stF(out, 0, f29_norm(ldF(in, 0))); PROBE_END
PROBE_OP(OpF29Add, 18, 9, 1) stF(out, 0, f29_add(ldF(in, 0), ldF(in, 1))); PROBE_END
PROBE_OP(OpF29Sub, 18, 9, 1) stF(out, 0, f29_sub<P>(ldF(in, 0), ldF(in, 1))); PROBE_END
PROBE_OP(OpF29Times, 9, 9, 1) stF(out, 0, f29_times<(u32)P>(ldF(in, 0))); PROBE_END
PROBE_OP(OpF29Mul, 18, 9, 1) stF(out, 0, f29_mul(ldF(in, 0), ldF(in, 1))); PROBE_END
PROBE_OP(OpF29MulCall, 18, 9, 1) stF(out, 0, f29_mul_call(ldF(in, 0), ldF(in, 1))); PROBE_END
PROBE_OP(OpF29Sqr, 9, 9, 1) stF(out, 0, f29_sqr(ldF(in, 0))); PROBE_END
PROBE_OP(OpF29SqrCall, 9, 9, 1) stF(out, 0, f29_sqr_call(ldF(in, 0))); PROBE_END
PROBE_OP(OpF29Canon, 9, 8, 1) stU(out, 0, f29_canon(ldF(in, 0))); PROBE_END
PROBE_OP(OpF29CanonCall, 9, 8, 1) stU(out, 0, f29_canon_call(ldF(in, 0))); PROBE_END
PROBE_OP(OpF29IsZero, 9, 1, 1) out[0] = f29_is_zero(ldF(in, 0)) ? 1u : 0u; PROBE_END

// in: X, Y, Z.  out: X3, Y3, Z3, W
PROBE_OP(OpJacDbl, 24, 32, 1)
    const JacW o = jac_dbl_cv<typename CurveOf<MOD>::type>(ldJ(in, 0));
    stU(out, 0, o.p.X);
    stU(out, 1, o.p.Y);
    stU(out, 2, o.p.Z);
    stU(out, 3, o.W);
PROBE_END
// in: X1, Y1, Z1, X2, Y2, Z2.  P = 2 Z1ONE + Z2ONE
PROBE_OP(OpJacAdd, 48, 32, 1)
    const JacW o = jac_add_cv<typename CurveOf<MOD>::type, (P & 2) != 0, (P & 1) != 0>(ldJ(in, 0), ldJ(in, 3));
    stU(out, 0, o.p.X);
    stU(out, 1, o.p.Y);
    stU(out, 2, o.p.Z);
    stU(out, 3, o.W);
PROBE_END
PROBE_OP(OpJacDbl29, 27, 36, 1)
    const JacWL o = jac_dbl29(ldJL(in, 0));
    stF(out, 0, o.p.X);
    stF(out, 1, o.p.Y);
    stF(out, 2, o.p.Z);
    stF(out, 3, o.W);
PROBE_END
PROBE_OP(OpJacAdd29, 54, 36, 1)
    const JacWL o = jac_add29<(P & 2) != 0, (P & 1) != 0>(ldJL(in, 0), ldJL(in, 3));
    stF(out, 0, o.p.X);
    stF(out, 1, o.p.Y);
    stF(out, 2, o.p.Z);
    stF(out, 3, o.W);
PROBE_END

void part2(std::vector<Entry>& v) {
    PROBE_E("f29_from_u256", OpF29From, 0, ModP, 0, 0)
    PROBE_E("f29_norm", OpF29Norm, 0, ModP, 0, 0)
    PROBE_E("f29_add", OpF29Add, 0, ModP, 0, 0)
    PROBE_E("f29_sub1", OpF29Sub, 1, ModP, 0, 0)
    PROBE_E("f29_sub2", OpF29Sub, 2, ModP, 0, 0)
    PROBE_E("f29_sub3", OpF29Sub, 3, ModP, 0, 0)
    PROBE_E("f29_sub4", OpF29Sub, 4, ModP, 0, 0)
    PROBE_E("f29_times2", OpF29Times, 2, ModP, 0, 0)
    PROBE_E("f29_times3", OpF29Times, 3, ModP, 0, 0)
    PROBE_E("f29_times4", OpF29Times, 4, ModP, 0, 0)
    PROBE_E("f29_mul", OpF29Mul, 0, ModP, 0, 0)
    PROBE_E("f29_mul_call", OpF29MulCall, 0, ModP, 0, 0)
    PROBE_E("f29_sqr", OpF29Sqr, 0, ModP, 0, 0)
    PROBE_E("f29_sqr_call", OpF29SqrCall, 0, ModP, 0, 0)
    PROBE_E("f29_canon", OpF29Canon, 0, ModP, 0, 0)
    PROBE_E("f29_canon_call", OpF29CanonCall, 0, ModP, 0, 0)
    PROBE_E("f29_is_zero", OpF29IsZero, 0, ModP, 0, 0)
    PROBE_E2("jac_dbl", OpJacDbl, 0, 0)
    PROBE_E2("jac_add_z00", OpJacAdd, 0, 0)
    PROBE_E2("jac_add_z01", OpJacAdd, 1, 0)
    PROBE_E2("jac_add_z10", OpJacAdd, 2, 0)
    PROBE_E2("jac_add_z11", OpJacAdd, 3, 0)
    PROBE_E("jac_dbl29", OpJacDbl29, 0, ModP, 0, 0)
    PROBE_E("jac_add29_z00", OpJacAdd29, 0, ModP, 0, 0)
    PROBE_E("jac_add29_z01", OpJacAdd29, 1, ModP, 0, 0)
    PROBE_E("jac_add29_z10", OpJacAdd29, 2, ModP, 0, 0)
    PROBE_E("jac_add29_z11", OpJacAdd29, 3, ModP, 0, 0)
}
#else
void part2(std::vector<Entry>& v);
#endif

// ---- part 3: the four-lane formulas ----------------------------------------------------------------------------------
#if PROBE_HAS(3)
P2E_HD void st_quad(u32* out, const QuadRes& q) {
    stU(out, 0, q.res.p.X);
    stU(out, 1, q.res.p.Y);
    stU(out, 2, q.res.p.Z);
    stU(out, 3, q.res.W);
    stU(out, 4, q.zz3);
    stU(out, 5, q.zz1);
    stU(out, 6, q.acc);
    out[56] = q.z3_zero ? 1u : 0u;
}
P2E_HD void st_quad29(u32* out, const QuadRes29& q) {
    stF(out, 0, q.p.X);
    stF(out, 1, q.p.Y);
    stF(out, 2, q.p.Z);
    stF(out, 3, q.zz3);
    stF(out, 4, q.zz1);
    stF(out, 5, q.acc);
    P2E_UNROLL
    for (int i = 0; i < 8; i++) out[54 + i] = q.mine.w[i];
    out[62] = q.z3_zero ? 1u : 0u;
}
// in: X, Y, Z, acc.  out (every lane): X3, Y3, Z3, W, Z3^2, Z1^2, acc', z3_zero
PROBE_OP(OpJacDblQuad, 32, 57, 4)
    st_quad(out, jac_dbl_quad_cv<typename CurveOf<MOD>::type>(role, ldJ(in, 0), ldU(in, 3)));
PROBE_END
// in: X1, Y1, Z1, X2, Y2, Z2, zz1_in, acc.  flag = have_zz1
PROBE_OP(OpJacAddQuad, 64, 57, 4)
    st_quad(out, jac_add_quad_cv<typename CurveOf<MOD>::type, (P & 2) != 0, (P & 1) != 0>(role, ldJ(in, 0), flag != 0, ldU(in, 6), ldJ(in, 3),
                                                                                         ldU(in, 7)));
PROBE_END
// lazy limbs.  in: X, Y, Z, acc.  out (every lane): X3, Y3, Z3, Z3^2, Z1^2, acc' (limbs), mine (words), z3_zero.  flag = no_affine
PROBE_OP(OpJacDblQuad29, 36, 63, 4)
    st_quad29(out, jac_dbl_quad29(role, (flag & 1) != 0, ldJL(in, 0), ldF(in, 3)));
PROBE_END
// in: X1, Y1, Z1, X2, Y2, Z2, zz1_in, acc.  flag = no_affine | have_zz1 << 1
PROBE_OP(OpJacAddQuad29, 72, 63, 4)
    st_quad29(out, jac_add_quad29<(P & 2) != 0, (P & 1) != 0>(role, (flag & 1) != 0, ldJL(in, 0), (flag & 2) != 0, ldF(in, 6), ldJL(in, 3),
                                                              ldF(in, 7)));
PROBE_END

void part3(std::vector<Entry>& v) {
    PROBE_E2("jac_dbl_quad", OpJacDblQuad, 0, 0)
    PROBE_E2("jac_add_quad_z00_have0", OpJacAddQuad, 0, 0)
    PROBE_E2("jac_add_quad_z00_have1", OpJacAddQuad, 0, 1)
    PROBE_E2("jac_add_quad_z01_have0", OpJacAddQuad, 1, 0)
    PROBE_E2("jac_add_quad_z01_have1", OpJacAddQuad, 1, 1)
    PROBE_E2("jac_add_quad_z10_have0", OpJacAddQuad, 2, 0)
    PROBE_E2("jac_add_quad_z10_have1", OpJacAddQuad, 2, 1)
    PROBE_E2("jac_add_quad_z11_have0", OpJacAddQuad, 3, 0)
    PROBE_E2("jac_add_quad_z11_have1", OpJacAddQuad, 3, 1)
    PROBE_E("jac_dbl_quad29_na0", OpJacDblQuad29, 0, ModP, 0, 0)
    PROBE_E("jac_dbl_quad29_na1", OpJacDblQuad29, 0, ModP, 0, 1)
    PROBE_E("jac_add_quad29_z00_na0_have0", OpJacAddQuad29, 0, ModP, 0, 0)
    PROBE_E("jac_add_quad29_z00_na1_have0", OpJacAddQuad29, 0, ModP, 0, 1)
    PROBE_E("jac_add_quad29_z00_na0_have1", OpJacAddQuad29, 0, ModP, 0, 2)
    PROBE_E("jac_add_quad29_z00_na1_have1", OpJacAddQuad29, 0, ModP, 0, 3)
    PROBE_E("jac_add_quad29_z01_na0_have0", OpJacAddQuad29, 1, ModP, 0, 0)
    PROBE_E("jac_add_quad29_z01_na1_have0", OpJacAddQuad29, 1, ModP, 0, 1)
    PROBE_E("jac_add_quad29_z01_na0_have1", OpJacAddQuad29, 1, ModP, 0, 2)
    PROBE_E("jac_add_quad29_z01_na1_have1", OpJacAddQuad29, 1, ModP, 0, 3)
    PROBE_E("jac_add_quad29_z10_na0_have0", OpJacAddQuad29, 2, ModP, 0, 0)
    PROBE_E("jac_add_quad29_z10_na1_have0", OpJacAddQuad29, 2, ModP, 0, 1)
    PROBE_E("jac_add_quad29_z10_na0_have1", OpJacAddQuad29, 2, ModP, 0, 2)
    PROBE_E("jac_add_quad29_z10_na1_have1", OpJacAddQuad29, 2, ModP, 0, 3)
    PROBE_E("jac_add_quad29_z11_na0_have0", OpJacAddQuad29, 3, ModP, 0, 0)
    PROBE_E("jac_add_quad29_z11_na1_have0", OpJacAddQuad29, 3, ModP, 0, 1)
    PROBE_E("jac_add_quad29_z11_na0_have1", OpJacAddQuad29, 3, ModP, 0, 2)
    PROBE_E("jac_add_quad29_z11_na1_have1", OpJacAddQuad29, 3, ModP, 0, 3)
}
#else
void part3(std::vector<Entry>& v);
#endif

}  // namespace probe

// ---- the C interface (lives in part 0) -------------------------------------------------------------------------------
#if PROBE_HAS(0)
namespace probe {
struct Table {
    std::vector<Entry> e;
    std::vector<int> op;   // op id of entry k: the index of the first entry with the same name
    Table() {
        part0(e);
        part1(e);
        part2(e);
        part3(e);
        int next = 0;
        for (size_t k = 0; k < e.size(); k++) {
            int id = -1;
            for (size_t j = 0; j < k && id < 0; j++)
                if (std::strcmp(e[j].name, e[k].name) == 0) id = op[j];
            op.push_back(id < 0 ? next++ : id);
        }
    }
};
static const Table& table() {
    static const Table t;
    return t;
}
}  // namespace probe

extern "C" {
// Entry `index` of the table: its name (NUL-terminated, cut to name_cap), op id, field (0 secp256k1 p, 1 secp256k1 n,
// 2 P-256 p, 3 P-256 n), bytes per element in and out (all lanes) and lanes per element.  Returns the number of entries,
// or -1 for an index outside the table.
long probe_ops(long index, char* name, size_t name_cap, int* op, int* field, int* in_bytes, int* out_bytes, int* lanes) {
    const probe::Table& t = probe::table();
    if (index < 0 || (size_t)index >= t.e.size()) return -1;
    const probe::Entry& e = t.e[(size_t)index];
    if (name && name_cap) {
        std::strncpy(name, e.name, name_cap - 1);
        name[name_cap - 1] = 0;
    }
    if (op) *op = t.op[(size_t)index];
    if (field) *field = e.field;
    if (in_bytes) *in_bytes = e.in_words * 4;
    if (out_bytes) *out_bytes = e.out_words * e.lanes * 4;
    if (lanes) *lanes = e.lanes;
    return (long)t.e.size();
}
// `n` elements of (op, field) from host memory to host memory.  The device build allocates, copies, launches and
// synchronises by itself and returns the HIP status (0 = success); -1 unknown (op, field), -2 element sizes that are not
// the table's, -3 null pointer.
long probe_run(int op, int field, const uint8_t* in, size_t in_bytes_per_elem, uint8_t* out, size_t out_bytes_per_elem, size_t n) {
    const probe::Table& t = probe::table();
    for (size_t k = 0; k < t.e.size(); k++) {
        const probe::Entry& e = t.e[k];
        if (t.op[k] != op || e.field != field) continue;
        if (in_bytes_per_elem != (size_t)e.in_words * 4 || out_bytes_per_elem != (size_t)e.out_words * e.lanes * 4) return -2;
        if (n && (!in || !out)) return -3;
        return e.run((const p2e::u32*)in, (p2e::u32*)out, n, e.flag);
    }
    return -1;
}
// 1 for the device build, 0 for the host build
int probe_is_device(void) {
#if defined(__HIPCC__)
    return 1;
#else
    return 0;
#endif
}
}
#endif

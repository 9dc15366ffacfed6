// CPU emulation harness -- TEST INFRASTRUCTURE ONLY (never loaded by the product path).
// Compiles the very same per-lane bodies the HIP kernels run (pipeline.hpp / prims.hpp) with g++ and
// drives them with plain loops, phase by phase, so kernel logic can be debugged in the GPU-less dev
// container.  tests/ compare its output with the oracle; the GPU tests then compare the real kernels.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../plonky2-ecdsa_amd/csrc/consts.hpp"
#include "../../plonky2-ecdsa_amd/csrc/pipeline.hpp"
#include "../../plonky2-ecdsa_amd/csrc/prims.hpp"
#include "../../plonky2-ecdsa_amd/csrc/fe29.hpp"
#include "../../plonky2-ecdsa_amd/csrc/quad.hpp"
#include "../../plonky2-ecdsa_amd/csrc/schedule.hpp"
#include "../../plonky2-ecdsa_amd/csrc/curve_program.hpp"
#include "../../plonky2-ecdsa_amd/csrc/knobs.hpp"
#include "../../plonky2-ecdsa_amd/csrc/launch_plan.hpp"

using namespace p2e;

// The per-lane bodies behind the steps of a launch plan (csrc/launch_plan.hpp), for the built-in programs and for the
// curve programs.  E = Emit (u64 column matrix) or CompactEmit (narrow / wide matrices of the compact container).
template <class E>
struct BuiltinBodies {
    static void scalar(const Program& G, const Buffers& B, size_t i) { body_scalar<E>(G, B, i); }
    static void chain_lane(const Program& G, const Buffers& B, size_t i, int lo, int hi, bool affine, bool cont) {
        body_chain_range(G, B, i, lo, hi, affine, cont);
    }
    // every role walks the whole range (the host form of a level computes all four products) and writes only its own
    // share of the scratch outputs
    static void chain_quad(const Program& G, const Buffers& B, size_t i, int lo, int hi, bool affine, bool cont) {
        for (int role = 0; role < 4; role++) body_chain_range_quad(G, B, i, role, lo, hi, affine, cont);
    }
    static void chain_rows(const Program& G, const Buffers& B, size_t i, int lo, int nrows, int count) {
        for (int r = 0; r < nrows; r++) body_chain_rows(G, B, i, lo, nrows, r, count);
    }
    static void binv(const Program& G, const Buffers& B, size_t i, int lo, int hi, bool have_prefix) { body_batch_inv(G, B, i, lo, hi, have_prefix); }
    static void binv_split(const Program& G, const Buffers& B, size_t i, int lo, int hi, bool have_prefix, int q, int split) {
        body_batch_inv_split(G, B, i, lo, hi, have_prefix, q, split);
    }
    static void expand(const Program& G, const Buffers& B, size_t i, int t) { body_expand<E>(G, B, i, t); }
    static void expand_run(const Program& G, const Buffers& B, size_t i, int it0, int it1) { body_expand_run<E>(G, B, i, it0, it1); }
    static void expand_fb_run(const Program& G, const Buffers& B, size_t i, int t_after) { body_expand_fb_run<E>(G, B, i, t_after); }
};
template <class CV, class E>
struct CurveBodies {
    static void scalar(const Program& G, const Buffers& B, size_t i) { body_cscalar<CV, E>(G, B, i); }
    static void chain_lane(const Program& G, const Buffers& B, size_t i, int lo, int hi, bool affine, bool) {
        body_chain_range<CV, true>(G, B, i, lo, hi, affine, false);
    }
    // body_chain_range_quad_cv with the four roles in lock step, op by op, as the four lanes of a quad run: the generic walker
    // reads most first operands back from scratch (X, Y, Z, W each stored by ONE role), so one role cannot walk the whole
    // range before the others have started
    static void chain_quad(const Program& G, const Buffers& B, size_t i, int lo, int hi, bool affine, bool) {
        ChainStateQ st[4];
        for (ChainStateQ& q : st) {
            q.out_id = q.p1_id = q.dyn_idx = q.dyn_val = 0xFFFF;
            q.out.X = q.out.Y = q.out.Z = q.p1.X = q.p1.Y = q.p1.Z = q.out_zz = q.p1_zz = u256_zero();
            q.acc = u256_small(1);
        }
        for (int t = lo; t < hi; t++) {
            const OpDesc op = load_op(B.ops, t);
            P1Sel s1[4];
            for (int role = 0; role < 4; role++) s1[role] = quad_first_operand(G, B, i, op, st[role]);
            for (int role = 0; role < 4; role++) body_chain_op_quad_cv<CV>(G, B, i, role, t, op, affine, s1[role], st[role]);
        }
    }
    static void chain_rows(const Program&, const Buffers&, size_t, int, int, int) { abort(); }   // no curve plan has rows
    static void binv(const Program& G, const Buffers& B, size_t i, int lo, int hi, bool have_prefix) { body_batch_inv<CV>(G, B, i, lo, hi, have_prefix); }
    static void binv_split(const Program& G, const Buffers& B, size_t i, int lo, int hi, bool have_prefix, int q, int split) {
        body_batch_inv_split<CV>(G, B, i, lo, hi, have_prefix, q, split);
    }
    static void expand(const Program& G, const Buffers& B, size_t i, int t) { body_expand<E, CV>(G, B, i, t); }
    static void expand_run(const Program& G, const Buffers& B, size_t i, int it0, int it1) {
        if (G.loop_dbls == 2)   // kc_expand_runs2
            body_expand_run<E, CV, 2>(G, B, i, it0, it1);
        else                    // kc_expand_runs
            body_expand_run<E, CV, 4>(G, B, i, it0, it1);
    }
    static void expand_fb_run(const Program& G, const Buffers& B, size_t i, int t_after) { body_expand_fb_run<E, CV>(G, B, i, t_after); }
};

// Executes the compute steps of a plan one after the other: in list order, or (order != nullptr) the steps order[0 ..
// n_order) in that order.  RECORD and WAIT are ignored: list order is a valid execution order because every wait names
// an event recorded earlier in the list (tests/test_knobs_cpu.py); which OTHER orders the waits permit is worked out by
// tests/test_plan_order_cpu.py, which runs them here.
// How a BINV step is executed is a local matter (arbitrary batching must not change any output):
//   split > 0          : the batch cut into `split` sub-ranges, whatever the step says (any count, not only 2^k)
//   0 < chunk < hi - lo: the forward pass re-run inside phase B, `chunk` ops at a time
//   otherwise          : what the step says (2^split_log2 sub-ranges, or one batch on phase A's prefix products)
template <class K>
static void exec_plan(const plan::Plan& pl, const Program& G, const Buffers& B, int chunk, int split, const int32_t* order = nullptr,
                      size_t n_order = 0) {
    const long long n = (long long)B.n;
    const size_t count = order ? n_order : (size_t)pl.n_steps;
    for (size_t at = 0; at < count; at++) {
        const int k = order ? (int)order[at] : (int)at;
        if (k < 0 || k >= pl.n_steps) continue;
        const plan::Step& s = pl.steps[k];
        switch (s.kind) {
        case plan::RECORD:
        case plan::WAIT:
        case plan::FINALIZE: break;
        case plan::SCALAR:
#pragma omp parallel for
            for (long long i = 0; i < n; i++) K::scalar(G, B, (size_t)i);
            break;
        case plan::CHAIN:
#pragma omp parallel for
            for (long long i = 0; i < n; i++) {
                if (s.form == plan::ROWS)
                    K::chain_rows(G, B, (size_t)i, s.a, s.b, s.c);
                else if (s.form == plan::QUAD)
                    K::chain_quad(G, B, (size_t)i, s.a, s.b, s.c != 0, s.d != 0);
                else
                    K::chain_lane(G, B, (size_t)i, s.a, s.b, s.c != 0, s.d != 0);
            }
            break;
        case plan::BINV: {
            const int parts = split > 0 ? split : s.d > 0 ? 1 << s.d : 0;
            if (parts > 0) {
#pragma omp parallel for
                for (long long i = 0; i < n; i++)
                    for (int q = 0; q < parts; q++) K::binv_split(G, B, (size_t)i, s.a, s.b, s.c != 0, q, parts);
            } else if (chunk <= 0 || chunk >= s.b - s.a) {
#pragma omp parallel for
                for (long long i = 0; i < n; i++) K::binv(G, B, (size_t)i, s.a, s.b, s.c != 0);
            } else {
                for (int t0 = s.a; t0 < s.b; t0 += chunk) {
                    const int t1 = t0 + chunk < s.b ? t0 + chunk : s.b;
#pragma omp parallel for
                    for (long long i = 0; i < n; i++) K::binv(G, B, (size_t)i, t0, t1, false);
                }
            }
            break;
        }
        case plan::EXPAND_OPS:
#pragma omp parallel for
            for (long long i = 0; i < n; i++)
                for (int t = s.a; t < s.b; t++) K::expand(G, B, (size_t)i, t);
            break;
        case plan::EXPAND_RUNS:
            for (int a = s.a; a < s.b; a += s.c) {   // one run per workgroup row of the launch
                const int b = a + s.c < s.b ? a + s.c : s.b;
#pragma omp parallel for
                for (long long i = 0; i < n; i++) K::expand_run(G, B, (size_t)i, a, b);
            }
            break;
        case plan::EXPAND_FB_RUN:
#pragma omp parallel for
            for (long long i = 0; i < n; i++) K::expand_fb_run(G, B, (size_t)i, s.a);
            break;
        }
    }
}

// the scratch of one emulated call, bound to B (everything but the inputs, the sink and the tables)
struct Scratch {
    std::vector<U256> PX, PY, PZ, PW, PREF, AX, AY;
    std::vector<uint8_t> dig4, dig2, valid8;
    std::vector<uint16_t> dyn, src, msrc;
    std::vector<u32> err32;
    Scratch(const Program& G, size_t n, Buffers& B)
        : PX((size_t)G.num_slots * n), PY(PX.size()), PZ(PX.size()), PW((size_t)G.num_ops * n), PREF(PW.size()), AX(PX.size()), AY(PX.size()),
          dig4((size_t)FB_WINDOWS * n), dig2((size_t)(G.cp_rows > MSM_DIGITS ? G.cp_rows : MSM_DIGITS) * n), valid8(n),
          dyn((size_t)G.num_cadd * n + 1), src((size_t)G.num_ops * 2 * n), msrc(dig2.size()), err32(n) {
        B.n = n;
        B.err = err32.data(); B.valid = valid8.data();
        B.PX = PX.data(); B.PY = PY.data(); B.PZ = PZ.data(); B.PW = PW.data(); B.PREF = PREF.data();
        B.AX = AX.data(); B.AY = AY.data();
        B.dig4 = dig4.data(); B.dig2 = dig2.data(); B.dyn = dyn.data(); B.src = src.data(); B.msrc = msrc.data();
    }
    // Every array holds a value no step of the call wrote: a step that runs before the step it reads from then computes
    // on these and its columns come out wrong.  The values are ones the bodies accept from any input -- field elements
    // below every modulus (canonical, non-zero; any 256-bit value passes the limb-bound tracker of f29_from_u256), digits
    // below 16, source ids that name slot 2 -- so that a premature read never leaves an array or aborts.
    void poison() {
        U256 v;
        for (int k = 0; k < 8; k++) v.w[k] = 0x01010101u * (u32)(k + 1);
        for (auto* a : {&PX, &PY, &PZ, &PW, &PREF, &AX, &AY}) std::fill(a->begin(), a->end(), v);
        std::fill(dig4.begin(), dig4.end(), (uint8_t)3);
        std::fill(dig2.begin(), dig2.end(), (uint8_t)3);
        std::fill(valid8.begin(), valid8.end(), (uint8_t)0xAA);
        for (auto* a : {&dyn, &src, &msrc}) std::fill(a->begin(), a->end(), (uint16_t)2);
        std::fill(err32.begin(), err32.end(), 0x40000000u);
    }
    // what k_finalize leaves: the flagged count
    long finalize(uint8_t* err, uint8_t* valid) const {
        long bad = 0;
        for (size_t i = 0; i < err32.size(); i++) {
            err[i] = (uint8_t)err32[i];
            if (valid) valid[i] = err32[i] ? 0 : valid8[i];
            bad += err32[i] != 0;
        }
        return bad;
    }
};

// A built-in program under the plan build_builtin makes of `P` (chunk, split: exec_plan); cols != nullptr: the u64 column
// matrix, otherwise the compact container.  -2: the record asks for a plan that build refuses.
static long run(int program, const plan::BuiltinParams& P, const uint8_t* msg, const uint8_t* r, const uint8_t* s, const uint8_t* pkx,
                const uint8_t* pky, uint64_t* cols, size_t n, size_t ld, uint8_t* err, uint8_t* valid, int chunk, int split,
                uint32_t* narrow = nullptr, size_t ldn = 0, uint64_t* wide = nullptr, size_t ldw = 0) {
    host::ScheduleBuilder sb;
    if (program == 0)
        sb.verify_secp256k1_message_circuit();
    else
        sb.glv_mul_circuit();
    sb.mark_runs(P.run_iters, P.fb_run);   // (as p2e_ctx_create marks the op tables: the fixed-base windows only with the fixed-base run)
    const Program& G = sb.prog;
    const host::Consts& C = host::consts();
    plan::Plan pl;
    pl.max_seg = plan::PIECES_CAP;   // no events here: any piece count the record asks for
    if (!plan::build_builtin(G, P, pl)) return -2;
    Buffers B{};
    Scratch scratch(G, n, B);
    B.msg = msg; B.r = r; B.s = s; B.pkx = pkx; B.pky = pky;
    // wide_before[c] = check_sum / carry columns (33 per mul generator, after its r and q limbs) before column c
    std::vector<u32> wide_before((size_t)G.num_cols + 1, 0);
    for (const auto& g : sb.gens)
        for (u32 k = 0; k < g.ncols; k++) wide_before[g.col + k + 1] = (g.kind == host::GEN_MUL && k >= 2 * NL) ? 1u : 0u;
    for (size_t c2 = 1; c2 < wide_before.size(); c2++) wide_before[c2] += wide_before[c2 - 1];
    B.sink = Sink{cols, ld, narrow, ldn, wide, ldw, wide_before.data()};
    B.cpts = C.cpts; B.fbtab = C.fbtab.data(); B.ops = sb.ops.data();
    if (cols)
        exec_plan<BuiltinBodies<Emit>>(pl, G, B, chunk, split);
    else
        exec_plan<BuiltinBodies<CompactEmit>>(pl, G, B, chunk, split);
    return scratch.finalize(err, valid);
}
// the record of the emu_verify / emu_glv_mul family: the loop in 3 pieces of runs of `run_iters` iterations (0: op by
// op), the fixed-base chain as one piece (with runs: its windows as one run per signature); chunk < 0: the four-lane
// plan with every inversion batch cut into -chunk sub-ranges
static long run_legacy(int program, const uint8_t* msg, const uint8_t* r, const uint8_t* s, const uint8_t* pkx, const uint8_t* pky,
                       uint64_t* cols, size_t n, size_t ld, uint8_t* err, uint8_t* valid, int chunk, int run_iters, uint32_t* narrow = nullptr,
                       size_t ldn = 0, uint64_t* wide = nullptr, size_t ldw = 0) {
    plan::BuiltinParams P;
    P.quad = P.alt_b = chunk < 0;
    P.run_iters = run_iters;
    P.ops = run_iters > 0 ? plan::OPS_RUNS : plan::OPS_PLAIN;
    P.msm_pieces = 4;
    P.fb_run = run_iters > 0 && !P.quad && program == 0;
    return run(program, P, msg, r, s, pkx, pky, cols, n, ld, err, valid, chunk, chunk < 0 ? -chunk : 0, narrow, ldn, wide, ldw);
}

// ---- fe29.hpp (lazy 29-bit limbs) against fe.hpp (canonical words): every operation on patterned and random values,
// with operands pushed through the lazy forms the chains use (sums, differences, small multiples) before they are used
static U256 f29_test_value(host::SplitMix64& rng) {
    U256 x;
    const unsigned long long sel = rng.next();
    for (int k = 0; k < 4; k++) {
        unsigned long long w = rng.next();
        const unsigned pat = (unsigned)(sel >> (8 * k)) & 7;
        if (pat == 0) w = 0;
        if (pat == 1) w = ~0ull;
        if (pat == 2) w &= 0xFFFFFFFFull;
        x.w[2 * k] = (u32)w;
        x.w[2 * k + 1] = (u32)(w >> 32);
    }
    const unsigned kind = (unsigned)(sel >> 40) & 15;
    if (kind == 0) x = u256_zero();
    if (kind == 1) x = u256_small(1);
    if (kind == 2 || kind == 3) {   // p - 1, p - small
        x = u256_zero();
        x = fe_sub<ModP>(x, u256_small(kind == 2 ? 1 : (u32)(sel >> 48) & 0xFFF));
    }
    return fe_canon<ModP>(fe_canon<ModP>(x));   // (two conditional subtractions: any 256-bit pattern -> canonical)
}
extern "C" long emu_f29_selftest(unsigned long long seed, size_t n) {
    long fails = 0;
#pragma omp parallel for reduction(+ : fails)
    for (long long i = 0; i < (long long)n; i++) {
        host::SplitMix64 rng{seed ^ (0x9E3779B97F4A7C15ull * (unsigned long long)(i + 1))};
        const U256 a = f29_test_value(rng), b = f29_test_value(rng), c = f29_test_value(rng);
        const F29 fa = f29_from_u256(a), fb = f29_from_u256(b), fc = f29_from_u256(c);
        auto same = [&](const F29& got, const U256& want) { fails += !u256_eq(f29_canon(f29_norm(got)), want); };
        auto same_direct = [&](const F29& got, const U256& want) { fails += !u256_eq(f29_canon(got), want); };   // limbs < 2^31
        typedef ModP F;
        same(fa, a);
        same_direct(fa, a);
        same_direct(f29_mul(fa, fb), fe_mul<F>(a, b));
        same_direct(f29_sub<1>(fa, fb), fe_sub<F>(a, b));
        same_direct(f29_add(f29_add(fa, fb), fc), fe_add<F>(fe_add<F>(a, b), c));
        same(f29_mul(fa, fb), fe_mul<F>(a, b));
        same(f29_sqr(fa), fe_sqr<F>(a));
        same(f29_add(fa, fb), fe_add<F>(a, b));
        same(f29_sub<1>(fa, fb), fe_sub<F>(a, b));
        same(f29_norm(f29_sub<1>(fa, fb)), fe_sub<F>(a, b));
        same(f29_times<3>(fa), fe_add<F>(fe_add<F>(a, a), a));
        // lazy operands: (a + b) (2 c), (a - b)(c - a), (a + b)^2, (a - b - c)^2 normalised first, 4 (a - 2 b)
        const U256 apb = fe_add<F>(a, b), amb = fe_sub<F>(a, b), cma = fe_sub<F>(c, a), c2 = fe_add<F>(c, c);
        same(f29_mul(f29_add(fa, fb), f29_times<2>(fc)), fe_mul<F>(apb, c2));
        same(f29_mul(f29_norm(f29_sub<1>(fa, fb)), f29_sub<1>(fc, fa)), fe_mul<F>(amb, cma));
        same(f29_sqr(f29_add(fa, fb)), fe_sqr<F>(apb));
        same(f29_sqr(f29_norm(f29_sub<1>(f29_sub<1>(fa, fb), fc))), fe_sqr<F>(fe_sub<F>(amb, c)));
        const U256 b2 = fe_add<F>(b, b), am2b = fe_sub<F>(a, b2), am2b2 = fe_add<F>(am2b, am2b);
        same(f29_times<4>(f29_norm(f29_sub<2>(fa, f29_times<2>(fb)))), fe_add<F>(am2b2, am2b2));
        same(f29_sub<3>(fa, f29_times<3>(fb)), fe_sub<F>(a, fe_add<F>(b2, b)));
        same(f29_sub<4>(fa, f29_add(f29_times<3>(fb), fc)), fe_sub<F>(fe_sub<F>(a, fe_add<F>(b2, b)), c));
        // a chain of dependent operations on lazy values
        F29 x = fa;
        U256 y = a;
        for (int k = 0; k < 6; k++) {
            x = f29_mul(f29_add(x, fb), f29_sub<1>(x, fc));
            y = fe_mul<F>(fe_add<F>(y, b), fe_sub<F>(y, c));
            x = f29_sqr(f29_norm(f29_sub<1>(f29_times<2>(x), fa)));
            y = fe_sqr<F>(fe_sub<F>(fe_add<F>(y, y), a));
        }
        same(x, y);
        fails += f29_is_zero(f29_sub<1>(fa, fa)) ? 0 : 1;
        fails += f29_is_zero(f29_mul(f29_sub<1>(fa, fb), f29_norm(f29_sub<1>(fb, fa)))) != u256_eq(a, b) ? 1 : 0;
    }
    return fails;
}

// f29_canon on caller-supplied limb forms (nine limbs each below 2^31, any value): the canonical 256-bit value,
// little-endian.  The walks above never hand it a value in [p, 2^256) -- the one range in which only its final conditional
// subtraction makes the result canonical -- so tests/test_adversarial_cpu.py builds such forms directly.
extern "C" long emu_f29_canon(const uint32_t* limbs, size_t n, uint8_t* out) {
    for (size_t i = 0; i < n; i++) {
        F29 a;
        for (int k = 0; k < 9; k++) {
            a.l[k] = limbs[9 * i + k];
            if (a.l[k] >> 31) return -1;
#if P2E_F29_TRACK
            a.ub[k] = a.l[k];
#endif
        }
        const U256 x = f29_canon_call(a);
        memcpy(out + 32 * i, x.w, 32);
    }
    return (long)n;
}

// the same stress loop for fe_inv_safegcd (csrc/fe.hpp), over all four moduli of the crate (field: 0 p, 1 n of secp256k1,
// 2 p, 3 n of P-256): x * inv(x) == 1, the result is canonical and equal to fe_inv_bingcd's; zero is reported as not invertible
template <class MOD>
static long safegcd_one(const U256& raw) {
    const U256 x = fe_canon<MOD>(fe_canon<MOD>(raw));
    U256 r, r2;
    const bool ok = fe_inv_safegcd<MOD>(x, r);
    if (u256_is_zero(x)) return ok ? 1 : 0;
    const bool ok2 = fe_inv_bingcd<MOD>(x, r2);
    return (ok && ok2 && u256_eq(r, r2) && !geq_mod<MOD>(r.w) && u256_eq(fe_mul<MOD>(x, r), u256_small(1))) ? 0 : 1;
}
// ---- ec29.hpp / quad29.hpp against ec.hpp / quad.hpp: every variant of the addition and the doubling, lane per signature and
// four-lane form, on arbitrary coordinates (the formulas never use the curve equation), under the limb-bound tracking
template <bool Z1ONE, bool Z2ONE>
static long ec29_add_case(const Jac& p1, const Jac& p2, const U256& acc, const U256& zz1) {
    long fails = 0;
    Jac a = p1, b = p2;
    if (Z1ONE) a.Z = u256_small(1);
    if (Z2ONE) b.Z = u256_small(1);
    const JacW want = jac_add<Z1ONE, Z2ONE>(a, b);
    const JacWL got = jac_add29<Z1ONE, Z2ONE>(jacl_from(a), jacl_from(b));
    fails += !u256_eq(f29_canon(got.p.X), want.p.X) + !u256_eq(f29_canon(got.p.Y), want.p.Y) + !u256_eq(f29_canon(got.p.Z), want.p.Z) +
             !u256_eq(f29_canon(got.W), want.W);
    for (int have = 0; have < 2; have++) {
        const U256 z1sq = fe_sqr<ModP>(a.Z);
        const QuadRes wq = jac_add_quad<Z1ONE, Z2ONE>(0, a, have != 0, have ? z1sq : zz1, b, acc);
        for (int role = 0; role < 4; role++) {
            const QuadRes29 q = jac_add_quad29<Z1ONE, Z2ONE>(role, false, jacl_from(a), have != 0, f29_from_u256(have ? z1sq : zz1), jacl_from(b),
                                                             f29_from_u256(acc));
            const U256 mine = role == 0 ? wq.res.p.X : role == 1 ? acc : role == 2 ? wq.res.p.Z : wq.res.W;
            fails += !u256_eq(f29_canon(q.p.X), wq.res.p.X) + !u256_eq(f29_canon(q.p.Y), wq.res.p.Y) + !u256_eq(f29_canon(q.p.Z), wq.res.p.Z) +
                     !u256_eq(f29_canon(q.acc), wq.acc) + !u256_eq(f29_canon(q.zz3), wq.zz3) + !u256_eq(q.mine, mine) + (q.z3_zero != wq.z3_zero);
            if (!Z1ONE) fails += !u256_eq(f29_canon(q.zz1), wq.zz1);
        }
    }
    return fails;
}
extern "C" long emu_ec29_selftest(unsigned long long seed, size_t n) {
    long fails = 0;
#pragma omp parallel for reduction(+ : fails)
    for (long long i = 0; i < (long long)n; i++) {
        host::SplitMix64 rng{seed ^ (0x9E3779B97F4A7C15ull * (unsigned long long)(i + 1))};
        Jac p1, p2;
        p1.X = f29_test_value(rng); p1.Y = f29_test_value(rng); p1.Z = f29_test_value(rng);
        p2.X = f29_test_value(rng); p2.Y = f29_test_value(rng); p2.Z = f29_test_value(rng);
        const U256 acc = f29_test_value(rng), zz1 = f29_test_value(rng);
        if ((i & 15) == 0) p2 = p1;                       // equal operands: H = 0, Z3 = 0 (the reference's inverse-of-zero case)
        fails += ec29_add_case<false, false>(p1, p2, acc, zz1) + ec29_add_case<false, true>(p1, p2, acc, zz1) +
                 ec29_add_case<true, false>(p1, p2, acc, zz1) + ec29_add_case<true, true>(p1, p2, acc, zz1);
        const JacW wd = jac_dbl(p1);
        const JacWL gd = jac_dbl29(jacl_from(p1));
        fails += !u256_eq(f29_canon(gd.p.X), wd.p.X) + !u256_eq(f29_canon(gd.p.Y), wd.p.Y) + !u256_eq(f29_canon(gd.p.Z), wd.p.Z) +
                 !u256_eq(f29_canon(gd.W), wd.W);
        const QuadRes wq = jac_dbl_quad(0, p1, acc);
        for (int role = 0; role < 4; role++)
            for (int na = 0; na < 2; na++) {
                const QuadRes29 q = jac_dbl_quad29(role, na != 0, jacl_from(p1), f29_from_u256(acc));
                const U256 mine = role == 1 ? acc : role == 3 ? wq.res.W : (role == 0 && !na) ? wq.res.p.X : wq.res.p.Z;
                fails += !u256_eq(f29_canon(q.p.X), wq.res.p.X) + !u256_eq(f29_canon(q.p.Y), wq.res.p.Y) + !u256_eq(f29_canon(q.p.Z), wq.res.p.Z) +
                         !u256_eq(f29_canon(q.acc), wq.acc) + !u256_eq(f29_canon(q.zz3), wq.zz3) + !u256_eq(f29_canon(q.zz1), wq.zz1) +
                         !u256_eq(q.mine, mine) + (q.z3_zero != wq.z3_zero);
            }
    }
    return fails;
}

extern "C" {
// raw access to the binary-GCD inversion (csrc/fe.hpp) for the stress test: ok[i] = round bound held
long emu_bingcd(int field, const uint8_t* x32, uint8_t* inv32, uint8_t* ok, size_t n) {
    long fails = 0;
#pragma omp parallel for reduction(+ : fails)
    for (long long i = 0; i < (long long)n; i++) {
        U256 x, r;
        std::memcpy(x.w, x32 + 32 * i, 32);
        bool good = field ? fe_inv_bingcd<ModN>(x, r) : fe_inv_bingcd<ModP>(x, r);
        std::memcpy(inv32 + 32 * i, r.w, 32);
        ok[i] = good;
        fails += !good;
    }
    return fails;
}
// self-checking stress loop: x from splitmix64 with assorted bit lengths / word patterns, x * inv(x) == 1
long emu_bingcd_selfcheck(int field, unsigned long long seed, size_t n) {
    long fails = 0;
#pragma omp parallel for reduction(+ : fails)
    for (long long i = 0; i < (long long)n; i++) {
        host::SplitMix64 rng{seed ^ (0x9E3779B97F4A7C15ull * (unsigned long long)(i + 1))};
        U256 x;
        unsigned long long sel = rng.next();
        for (int k = 0; k < 4; k++) {
            unsigned long long w = rng.next();
            unsigned pat = (unsigned)(sel >> (8 * k)) & 7;
            if (pat == 0) w = 0;
            if (pat == 1) w = ~0ull;
            if (pat == 2) w &= 0xFFFFFFFFull;
            x.w[2 * k] = (u32)w;
            x.w[2 * k + 1] = (u32)(w >> 32);
        }
        int bits = 1 + (int)((sel >> 40) % 256);
        for (int b = bits; b < 256; b++) x.w[b >> 5] &= ~(1u << (b & 31));
        x = field ? fe_canon<ModN>(x) : fe_canon<ModP>(x);
        if (u256_is_zero(x)) continue;
        U256 r;
        bool ok = field ? fe_inv_bingcd<ModN>(x, r) : fe_inv_bingcd<ModP>(x, r);
        U256 one = field ? fe_mul<ModN>(x, r) : fe_mul<ModP>(x, r);
        if (!ok || !u256_eq(one, u256_small(1))) fails++;
    }
    return fails;
}
long emu_safegcd_selfcheck(int field, unsigned long long seed, size_t n) {
    long fails = 0;
#pragma omp parallel for reduction(+ : fails)
    for (long long i = 0; i < (long long)n; i++) {
        host::SplitMix64 rng{seed ^ (0x9E3779B97F4A7C15ull * (unsigned long long)(i + 1))};
        U256 x;
        unsigned long long sel = rng.next();
        for (int k = 0; k < 4; k++) {
            unsigned long long w = rng.next();
            unsigned pat = (unsigned)(sel >> (8 * k)) & 7;
            if (pat == 0) w = 0;
            if (pat == 1) w = ~0ull;
            if (pat == 2) w &= 0xFFFFFFFFull;
            x.w[2 * k] = (u32)w;
            x.w[2 * k + 1] = (u32)(w >> 32);
        }
        int bits = 1 + (int)((sel >> 40) % 256);
        if ((sel >> 50) & 1)
            for (int b = bits; b < 256; b++) x.w[b >> 5] &= ~(1u << (b & 31));
        if (((sel >> 52) & 63) == 0) {   // m - small
            x = u256_zero();
            x.w[0] = (u32)(sel >> 58) + 1u;
            x = field == 0 ? fe_neg<ModP>(x) : field == 1 ? fe_neg<ModN>(x) : field == 2 ? fe_neg<ModP256>(x) : fe_neg<ModN256>(x);
        }
        fails += field == 0 ? safegcd_one<ModP>(x) : field == 1 ? safegcd_one<ModN>(x) : field == 2 ? safegcd_one<ModP256>(x) : safegcd_one<ModN256>(x);
    }
    return fails;
}
// the knob table (csrc/knobs.hpp) read from `count` (name, value) pairs instead of the environment: out[0..21] = the
// scalar fields in the order below, out[22..38] = small_takes
long emu_tuning(const char* const* names, const char* const* values, size_t count, long long* out) {
    Tuning t;
    read_tuning(t, [&](const char* name) -> const char* {
        for (size_t k = 0; k < count; k++)
            if (!std::strcmp(names[k], name)) return values[k];
        return nullptr;
    });
    const long long scalars[] = {t.run_iters, t.run_iters_mid, t.run_iters_small, t.fb_run, (long long)t.runs_min_n, (long long)t.quad_max_n,
                                 (long long)t.cp_quad_max_n, (long long)t.binv_alt_max_n, (long long)t.cp_runs_min_n, t.msm_pieces,
                                 t.msm_pieces_mid, t.msm_pieces_small, t.fixed_pieces, t.fixed_pieces_small, t.binv_mid_split_log2,
                                 t.binv_split_log2, t.binv_split_log2_last, t.binv_split_log2_fixed, t.quad_b_first_on_fixed,
                                 t.quad_few_waits, t.expand_lds_small, t.expand_lds};
    long k = 0;
    for (long long v : scalars) out[k++] = v;
    for (int v : t.small_takes) out[k++] = v;
    return k;
}
long emu_verify(const uint8_t* msg, const uint8_t* r, const uint8_t* s, const uint8_t* pkx, const uint8_t* pky,
                uint64_t* cols, size_t n, size_t ld, uint8_t* err, uint8_t* valid, int chunk, int run_iters) {
    return run_legacy(0, msg, r, s, pkx, pky, cols, n, ld, err, valid, chunk, run_iters);
}
// verdict only (p2e_ecdsa_verify_batch): scalar phase without emission, Jacobian chains, r == x on the Jacobian result
long emu_verify_only(const uint8_t* msg, const uint8_t* r, const uint8_t* s, const uint8_t* pkx, const uint8_t* pky, size_t n,
                     uint8_t* err, uint8_t* valid) {
    host::ScheduleBuilder sb;
    sb.verify_secp256k1_message_circuit();
    const Program& G = sb.prog;
    const host::Consts& C = host::consts();
    Buffers B{};
    Scratch scratch(G, n, B);
    B.msg = msg; B.r = r; B.s = s; B.pkx = pkx; B.pky = pky;
    B.cpts = C.cpts; B.fbtab = C.fbtab.data(); B.ops = sb.ops.data();
#pragma omp parallel for
    for (long long i = 0; i < (long long)n; i++) {
        body_scalar<NullEmit>(G, B, (size_t)i);
        body_chain_range(G, B, (size_t)i, G.chain_begin[1], G.chain_end[1], false, false);
        body_chain_range(G, B, (size_t)i, G.chain_begin[0], G.chain_end[0], false, false);
        body_chain_range(G, B, (size_t)i, G.chain_begin[2], G.chain_end[2], false, false);
        body_verify_check(G, B, (size_t)i);
    }
    return scratch.finalize(err, valid);
}
// the same walk writing the compact container directly (CompactEmit: what the compact kernels' ragged tail runs)
long emu_verify_compact(const uint8_t* msg, const uint8_t* r, const uint8_t* s, const uint8_t* pkx, const uint8_t* pky,
                        uint32_t* narrow, size_t ldn, uint64_t* wide, size_t ldw, size_t n, uint8_t* err, uint8_t* valid,
                        int run_iters) {
    return run_legacy(0, msg, r, s, pkx, pky, nullptr, n, 0, err, valid, 512, run_iters, narrow, ldn, wide, ldw);
}
long emu_glv_mul_compact(const uint8_t* px, const uint8_t* py, const uint8_t* k, uint32_t* narrow, size_t ldn, uint64_t* wide,
                         size_t ldw, size_t n, uint8_t* err, uint8_t* valid, int run_iters) {
    return run_legacy(1, k, k, k, px, py, nullptr, n, 0, err, valid, 512, run_iters, narrow, ldn, wide, ldw);
}
long emu_glv_mul(const uint8_t* px, const uint8_t* py, const uint8_t* k, uint64_t* cols, size_t n, size_t ld,
                 uint8_t* err, uint8_t* valid, int chunk, int run_iters) {
    return run_legacy(1, k, k, k, px, py, cols, n, ld, err, valid, chunk, run_iters);
}
// built-in-generator columns from a finished witness matrix (aux.hpp: the body k_aux runs)
long emu_aux(int program, const uint8_t* pky, const uint64_t* cols, size_t ld, uint64_t* aux, size_t ald, size_t n,
             uint8_t* err) {
    host::ScheduleBuilder sb;
    if (program == 0)
        sb.verify_secp256k1_message_circuit();
    else
        sb.glv_mul_circuit();
    const host::Consts& C = host::consts();
    std::vector<u32> err32(n);
    AuxArgs A{cols, ld, aux, ald, n, pky, C.cpts, C.fbtab.data(), sb.aux_items.data(), &sb.aux_tab, err32.data(),
              nullptr, 0, nullptr};
    for (int item = 0; item < (int)sb.aux_items.size(); item++) {
#pragma omp parallel for
        for (long long i = 0; i < (long long)n; i++) body_aux<Emit>(A, item, (size_t)i);
    }
    long bad = 0;
    for (size_t i = 0; i < n; i++) {
        err[i] = (uint8_t)err32[i];
        bad += err32[i] != 0;
    }
    return bad;
}
// the same pass inside the compact container: narrow u32 matrix in, u32 aux matrix out
long emu_aux_compact(int program, const uint8_t* pky, const uint32_t* narrow, size_t ldn, uint32_t* aux32, size_t ald, size_t n,
                     uint8_t* err) {
    host::ScheduleBuilder sb;
    if (program == 0)
        sb.verify_secp256k1_message_circuit();
    else
        sb.glv_mul_circuit();
    const host::Consts& C = host::consts();
    std::vector<u32> wide_before((size_t)sb.prog.num_cols + 1, 0);
    for (const auto& g : sb.gens)
        for (u32 k = 0; k < g.ncols; k++) wide_before[g.col + k + 1] = (g.kind == host::GEN_MUL && k >= 2 * NL) ? 1u : 0u;
    for (size_t c2 = 1; c2 < wide_before.size(); c2++) wide_before[c2] += wide_before[c2 - 1];
    std::vector<u32> err32(n);
    AuxArgs A{nullptr, 0, aux32, ald, n, pky, C.cpts, C.fbtab.data(), sb.aux_items.data(), &sb.aux_tab, err32.data(),
              narrow, ldn, wide_before.data()};
    for (int item = 0; item < (int)sb.aux_items.size(); item++) {
#pragma omp parallel for
        for (long long i = 0; i < (long long)n; i++) body_aux<Emit32>(A, item, (size_t)i);
    }
    long bad = 0;
    for (size_t i = 0; i < n; i++) {
        err[i] = (uint8_t)err32[i];
        bad += err32[i] != 0;
    }
    return bad;
}
// constraint-block columns from finished matrices (ux.hpp: the body k_ux runs); inputs by INPUT_* slot
long emu_ux(int program, const uint8_t* msg, const uint8_t* r, const uint8_t* s, const uint8_t* pkx, const uint8_t* pky,
            const uint64_t* cols, size_t ld, const uint64_t* aux, size_t ald, uint64_t* ux, size_t uld, size_t n, uint8_t* err) {
    host::ScheduleBuilder sb;
    if (program == 0)
        sb.verify_secp256k1_message_circuit();
    else
        sb.glv_mul_circuit();
    U256 cv[NUM_CONSTV];
    for (u32 id = 0; id < NUM_CONSTV; id++) cv[id] = host::ScheduleBuilder::const_value(id);
    std::vector<u32> err32(n);
    UxArgs A{};
    A.cols = cols; A.ld = ld; A.aux = aux; A.ald = ald; A.ux = ux; A.uld = uld; A.n = n;
    A.in[INPUT_PY] = pky; A.in[INPUT_PX] = pkx; A.in[INPUT_MSG] = msg; A.in[INPUT_R] = r ? r : msg; A.in[INPUT_S] = s ? s : msg;
    A.consts = cv; A.items = sb.ux_items.data(); A.err = err32.data();
    for (int item = 0; item < (int)sb.ux_items.size(); item++) {
#pragma omp parallel for
        for (long long i = 0; i < (long long)n; i++) body_ux<Emit>(A, item, (size_t)i);
    }
    long bad = 0;
    for (size_t i = 0; i < n; i++) {
        err[i] = (uint8_t)err32[i];
        bad += err32[i] != 0;
    }
    return (long)sb.num_ux_cols + 0 * bad;
}
// gate-internal values from an aux matrix (aux.hpp body_gate)
long emu_gate(int program, const uint64_t* aux, size_t ald, uint64_t* gate, size_t gld, size_t n) {
    host::ScheduleBuilder sb;
    if (program == 0)
        sb.verify_secp256k1_message_circuit();
    else
        sb.glv_mul_circuit();
    GateArgs A{};
    A.aux = aux; A.ald = ald; A.gate = gate; A.gld = gld; A.n = n; A.items = sb.gate_items.data();
    A.inv16[0] = 0;
    for (u64 d = 1; d < 16; d++) {
        u64 r = 1, a = d, e = P_GL - 2;
        while (e) {
            if (e & 1) r = gl_mul(r, a);
            a = gl_mul(a, a);
            e >>= 1;
        }
        A.inv16[d] = r;
    }
    for (int item = 0; item < (int)sb.gate_items.size(); item++)
        for (size_t i = 0; i < n; i++) body_gate<Emit>(A, item, i);
    return (long)sb.num_gate_cols;
}
long emu_aux_num_cols(int program) {
    host::ScheduleBuilder sb;
    if (program == 0)
        sb.verify_secp256k1_message_circuit();
    else
        sb.glv_mul_circuit();
    return (long)sb.aux_tab.num_aux_cols;
}
#define LOOP(expr)                                  \
    long bad = 0;                                   \
    for (size_t i = 0; i < n; i++) {                \
        uint8_t e = (expr);                         \
        err[i] = e;                                 \
        bad += e != 0;                              \
    }                                               \
    return bad;
long emu_mul(int field, const u64* x, const u64* y, u64* r, u64* q, u64* cs, u64* b, size_t n, size_t ld, uint8_t* err) {
    LOOP(field == 3   ? prim_mul<ModN256>(x, y, r, q, cs, b, ld, i)
         : field == 2 ? prim_mul<ModP256>(x, y, r, q, cs, b, ld, i)
         : field      ? prim_mul<ModN>(x, y, r, q, cs, b, ld, i)
                      : prim_mul<ModP>(x, y, r, q, cs, b, ld, i))
}
long emu_checksum(const u64* a, u64* b, size_t n, size_t ld, uint8_t* err) { LOOP(prim_checksum(a, b, ld, i)) }
long emu_add(int field, const u64* a, const u64* b, u64* out, u64* ov, size_t n, size_t ld, uint8_t* err) {
    LOOP(field == 3   ? (prim_addsub<ModN256, false>(a, b, out, ov, ld, i))
         : field == 2 ? (prim_addsub<ModP256, false>(a, b, out, ov, ld, i))
         : field      ? (prim_addsub<ModN, false>(a, b, out, ov, ld, i))
                      : (prim_addsub<ModP, false>(a, b, out, ov, ld, i)))
}
long emu_sub(int field, const u64* a, const u64* b, u64* out, u64* ov, size_t n, size_t ld, uint8_t* err) {
    LOOP(field == 3   ? (prim_addsub<ModN256, true>(a, b, out, ov, ld, i))
         : field == 2 ? (prim_addsub<ModP256, true>(a, b, out, ov, ld, i))
         : field      ? (prim_addsub<ModN, true>(a, b, out, ov, ld, i))
                      : (prim_addsub<ModP, true>(a, b, out, ov, ld, i)))
}
long emu_add_many(int field, const u64* s, int k, u64* out, u64* ov, size_t n, size_t ld, uint8_t* err) {
    LOOP(field == 3   ? prim_add_many<ModN256>(s, k, out, ov, ld, i)
         : field == 2 ? prim_add_many<ModP256>(s, k, out, ov, ld, i)
         : field      ? prim_add_many<ModN>(s, k, out, ov, ld, i)
                      : prim_add_many<ModP>(s, k, out, ov, ld, i))
}
long emu_inv(int field, const u64* x, u64* inv, u64* div, size_t n, size_t ld, uint8_t* err) {
    LOOP(field == 3   ? prim_inv<ModN256>(x, inv, div, ld, i)
         : field == 2 ? prim_inv<ModP256>(x, inv, div, ld, i)
         : field      ? prim_inv<ModN>(x, inv, div, ld, i)
                      : prim_inv<ModP>(x, inv, div, ld, i))
}
long emu_div_rem(const u64* a, int na, const u64* b, int nb, u64* div, u64* rem, size_t n, size_t ld, uint8_t* err) {
    LOOP(prim_div_rem(a, na, b, nb, div, rem, ld, i))
}
long emu_glv(const u64* k, u64* k1, u64* k2, u64* n1, u64* n2, size_t n, size_t ld, uint8_t* err) {
    LOOP(prim_glv(k, k1, k2, n1, n2, ld, i))
}
long emu_split(const uint8_t* packed, u64* limbs, size_t n, size_t ld) {
    for (size_t i = 0; i < n; i++) prim_split(packed, limbs, ld, i);
    return 0;
}
long emu_pack(const u64* limbs, uint8_t* packed, size_t n, size_t ld, uint8_t* err) { LOOP(prim_pack(limbs, packed, ld, i)) }
}

// ---- curve programs (curves.hpp): the bodies kc_scalar / kc_chains / kc_batch_inv / kc_expand run, under the plan
// build_curve makes of `P` (csrc/launch_plan.hpp).  -2: the record asks for a plan that build refuses. ----------------
template <class CV>
static long run_curve(const host::CurveProgramHost& H, const plan::CurveParams& P, const uint8_t* msg, const uint8_t* r, const uint8_t* s,
                      const uint8_t* pkx, const uint8_t* pky, uint64_t* cols, size_t n, size_t ld, uint8_t* err, uint8_t* valid,
                      const uint8_t* qx = nullptr, const uint8_t* qy = nullptr) {
    const host::ScheduleBuilder& sb = H.sb;
    const Program& G = sb.prog;
    plan::Plan pl;
    pl.max_seg = plan::PIECES_CAP;   // no events here: any piece count the record asks for
    if (!plan::build_curve(G, P, pl)) return -2;
    if (P.runs && G.msm_loop_iters > 0 && G.loop_dbls != 2 && G.loop_dbls != 4) return -2;
    Buffers B{};
    Scratch scratch(G, n, B);
    B.msg = msg; B.r = r; B.s = s; B.pkx = pkx; B.pky = pky;
    B.qx = qx; B.qy = qy;   // the MSM program's second point (null for every other program)
    B.sink = Sink{cols, ld, nullptr, 0, nullptr, 0, nullptr};
    B.cpts = sb.gpts.data(); B.fbtab = sb.gfbtab.data(); B.ops = sb.ops.data();
    host::ScheduleBuilder marked;
    if (pl.ops == plan::OPS_RUNS) {   // the op table with the run marks
        marked = sb;
        marked.mark_runs(P.run_iters);
        B.ops = marked.ops.data();
    }
    exec_plan<CurveBodies<CV, Emit>>(pl, G, B, 0, 0);
    return scratch.finalize(err, valid);
}
// the record of emu_curve_program / emu_curve_msm: pieces of `piece` ops expanded op by op on one chain stream, or
// (piece < 0) the run plan with -piece loop iterations per run
static plan::CurveParams curve_legacy_params(int piece) {
    plan::CurveParams P;
    if (piece == 0) piece = 32;
    P.runs = piece < 0;
    P.run_iters = piece < 0 ? -piece : 0;
    P.piece_ops = piece > 0 ? piece : plan::CP_PIECE_OPS;
    return P;
}
extern "C" {
// kind / curve: include/p2e.h P2E_CP_* / P2E_CURVE_*; blind: the gadget's rand() point.  Returns the flagged count, or
// -1 for an unknown program; *num_cols receives the program's column count (call with n = 0 to query it).
long emu_curve_program(int kind, int curve, const uint8_t* blind_x, const uint8_t* blind_y, const uint8_t* msg, const uint8_t* r,
                       const uint8_t* s, const uint8_t* pkx, const uint8_t* pky, uint64_t* cols, size_t n, size_t ld, uint8_t* err,
                       uint8_t* valid, int piece, long* num_cols, long* num_gens, long* num_aux) {
    Aff blind;
    memcpy(blind.x.w, blind_x, 32);
    memcpy(blind.y.w, blind_y, 32);
    host::CurveProgramHost H;
    if (!host::make_curve_program(H, kind, curve, blind)) return -1;
    if (num_cols) *num_cols = H.sb.prog.num_cols;
    if (num_gens) *num_gens = (long)H.sb.gens.size();
    if (num_aux) *num_aux = (long)H.sb.aux_tab.num_aux_cols;
    if (n == 0) return 0;
    const plan::CurveParams P = curve_legacy_params(piece);   // piece < 0: the run plan with -piece windows per run
    if (curve == 1) return run_curve<P256>(H, P, msg, r, s, pkx, pky, cols, n, ld, err, valid);
    return run_curve<Secp256k1>(H, P, msg, r, s, pkx, pky, cols, n, ld, err, valid);
}
// a program, the op table its plan binds (the run marks of the plan's record), and the plan
struct PlanCase {
    int family = 0, prog = 0, curve = 0, loop_stride = 3;
    host::CurveProgramHost H;
    plan::Plan pl;
    const Program& G() const { return H.sb.prog; }
};
// choose + build with the knobs and per-call switches read from `count` (name, value) pairs instead of the environment
// (P2E_STREAM_LAYOUT and P2E_QUAD_EXPAND_CUS as p2e_ctx_create reads them), for a call of n elements.  family 0: built-in
// program `prog`; family 1: curve program of kind `prog` on `curve` (blind: the gadget's rand() point).  *error: 0, or
// -(plan::Error) where build refuses (the case is returned all the same, for its program), or -100 for an unknown program
// (null).
static PlanCase* make_case(int family, int prog, int curve, const uint8_t* blind_x, const uint8_t* blind_y, size_t n, const char* const* names,
                           const char* const* values, size_t count, int timing, long* error) {
    auto env = [&](const char* name) -> const char* {
        for (size_t k = 0; k < count; k++)
            if (!std::strcmp(names[k], name)) return values[k];
        return nullptr;
    };
    Tuning t;
    read_tuning(t, env);
    const char* layout = env("P2E_STREAM_LAYOUT");
    if (!layout || !*layout) layout = "M1FB2";
    const char* cus = env("P2E_QUAD_EXPAND_CUS");
    const plan::Layout L{std::strchr(layout, '1') != nullptr, cus && atoi(cus) > 0};
    PlanCase* pc = new PlanCase;
    pc->family = family;
    pc->prog = prog;
    pc->curve = curve;
    host::ScheduleBuilder& sb = pc->H.sb;
    long err = 0;
    if (family == 0) {
        if (prog == 0)
            sb.verify_secp256k1_message_circuit();
        else
            sb.glv_mul_circuit();
        const plan::BuiltinParams P = plan::choose_builtin(sb.prog, t, n, L, timing != 0);
        sb.mark_runs(P.run_iters, P.fb_run);   // (as p2e_ctx_create marks the op table this plan binds)
        if (!plan::build_builtin(sb.prog, P, pc->pl)) err = -(long)pc->pl.error;
        pc->loop_stride = 3;
    } else {
        Aff blind;
        memcpy(blind.x.w, blind_x, 32);
        memcpy(blind.y.w, blind_y, 32);
        if (!host::make_curve_program(pc->H, prog, curve, blind)) {
            err = -100;
        } else {
            const Program& G = sb.prog;
            const plan::CurveParams P = plan::choose_curve(G, t, n, G.msm_loop_iters > 0 || prog == CP_FIXED_BASE_MUL, L, timing != 0,
                                                           read_call_switches(env));
            if (!plan::build_curve(G, P, pc->pl))
                err = -(long)pc->pl.error;
            else if (pc->pl.ops == plan::OPS_RUNS)
                sb.mark_runs(P.run_iters);
            pc->loop_stride = G.loop_dbls + 1;
        }
    }
    *error = err;
    if (err == -100) {
        delete pc;
        return nullptr;
    }
    return pc;
}
// ---- launch plans (csrc/launch_plan.hpp) ------------------------------------------------------------------------------
// choose + build with the knobs and per-call switches read from `count` (name, value) pairs instead of the environment
// (P2E_STREAM_LAYOUT and P2E_QUAD_EXPAND_CUS as p2e_ctx_create reads them), for a call of n elements: the plan's text
// form in out[0..cap), its length returned; -(plan::Error) where build refuses.  family 0: built-in program `prog`;
// family 1: curve program of kind `prog` on `curve` (blind: the gadget's rand() point).  shape (optional) receives
// num_ops, fb_begin, fb_windows, msm_loop_begin, msm_loop_iters, ops per loop iteration, plan::MAX_SEG, plan::MAX_EXPAND.
long emu_plan_dump(int family, int prog, int curve, const uint8_t* blind_x, const uint8_t* blind_y, size_t n, const char* const* names,
                   const char* const* values, size_t count, int timing, char* out, size_t cap, int32_t* shape) {
    long err = 0;
    PlanCase* pc = make_case(family, prog, curve, blind_x, blind_y, n, names, values, count, timing, &err);
    if (!pc) return err;
    const Program& G = pc->G();
    if (shape) {
        const int32_t v[8] = {G.num_ops, G.fb_begin, G.fb_windows, G.msm_loop_begin, G.msm_loop_iters, pc->loop_stride, plan::MAX_SEG, plan::MAX_EXPAND};
        memcpy(shape, v, sizeof v);
    }
    const long len = err ? err : (long)plan::dump(pc->pl, out, cap);
    delete pc;
    return len;
}
// ---- one plan case held open (tests/test_plan_order_cpu.py): the program, the op table the plan binds and the plan, as
// emu_plan_dump makes them; then its text form, its column blocks, its op table, and any number of executions in orders of
// the caller's choosing.  drop_step >= 0: the plan WITHOUT that step (a mutation for the tests: never issued on a device).
// *error receives -(plan::Error) where build refuses, -100 for an unknown program, -101 for a step the plan does not have;
// the handle is then null.
void* emu_case_open(int family, int prog, int curve, const uint8_t* blind_x, const uint8_t* blind_y, size_t n, const char* const* names,
                    const char* const* values, size_t count, int timing, int drop_step, long* error) {
    long err = 0;
    PlanCase* pc = make_case(family, prog, curve, blind_x, blind_y, n, names, values, count, timing, &err);
    if (pc && !err && drop_step >= 0) {
        if (drop_step >= pc->pl.n_steps) {
            err = -101;
        } else {
            for (int k = drop_step; k + 1 < pc->pl.n_steps; k++) pc->pl.steps[k] = pc->pl.steps[k + 1];
            pc->pl.n_steps--;
        }
    }
    if (error) *error = err;
    if (err) {
        delete pc;
        return nullptr;
    }
    return pc;
}
void emu_case_close(void* h) { delete (PlanCase*)h; }
long emu_case_dump(void* h, char* out, size_t cap) { return (long)plan::dump(((PlanCase*)h)->pl, out, cap); }
// plan::column_blocks of the case: (first_col, num_cols, event) per block; returns the number of blocks
long emu_case_blocks(void* h, int32_t* out, size_t cap) {
    const PlanCase& pc = *(PlanCase*)h;
    const std::vector<plan::ColumnBlock> b = plan::column_blocks(pc.G(), pc.H.sb.ops, pc.pl, pc.loop_stride);
    for (size_t k = 0; k < b.size() && k < cap; k++) {
        out[3 * k] = (int32_t)b[k].first_col;
        out[3 * k + 1] = (int32_t)b[k].num_cols;
        out[3 * k + 2] = b[k].event;
    }
    return (long)b.size();
}
// the host op table the plan binds: (kind, flags, ref1, ref2, col, number of columns, cadd_idx) per op; returns num_ops.
// shape (optional): num_ops, num_slots, slot_p, slot_sp, num_cols, num_chains, chain_begin[4], chain_end[4], msm_loop_begin,
// msm_loop_iters, ops per loop iteration, fb_begin, fb_windows, cp_table_ops, msm_tab[16]
long emu_case_ops(void* h, uint32_t* out, size_t cap, int64_t* shape) {
    const PlanCase& pc = *(PlanCase*)h;
    const std::vector<OpDesc>& ops = pc.H.sb.ops;
    for (size_t t = 0; t < ops.size() && t < cap; t++) {
        const uint32_t v[7] = {ops[t].kind, ops[t].flags, ops[t].ref1, ops[t].ref2, ops[t].col, plan::op_cols(ops[t]), ops[t].cadd_idx};
        memcpy(out + 7 * t, v, sizeof v);
    }
    if (shape) {
        const Program& G = pc.G();
        int k = 0;
        for (int64_t v : {(int64_t)G.num_ops, (int64_t)G.num_slots, (int64_t)G.slot_p, (int64_t)G.slot_sp, (int64_t)G.num_cols, (int64_t)G.num_chains})
            shape[k++] = v;
        for (int c = 0; c < 4; c++) shape[k++] = G.chain_begin[c];
        for (int c = 0; c < 4; c++) shape[k++] = G.chain_end[c];
        for (int64_t v : {(int64_t)G.msm_loop_begin, (int64_t)G.msm_loop_iters, (int64_t)pc.loop_stride, (int64_t)G.fb_begin, (int64_t)G.fb_windows,
                          (int64_t)G.cp_table_ops})
            shape[k++] = v;
        for (int c = 0; c < 16; c++) shape[k++] = G.msm_tab[c];
    }
    return (long)ops.size();
}
// The case's plan executed on n elements into the u64 column matrix: steps order[0 .. n_order) in that order (null: list
// order; inputs as emu_curve_program / emu_curve_msm).  poison != 0: every scratch array and the output start from Scratch::poison / a fixed pattern.  Returns the
// flagged count.
long emu_case_exec(void* h, const uint8_t* msg, const uint8_t* r, const uint8_t* s, const uint8_t* pkx, const uint8_t* pky, const uint8_t* qx,
                   const uint8_t* qy, uint64_t* cols, size_t n, size_t ld, uint8_t* err, uint8_t* valid, const int32_t* order, size_t n_order, int poison) {
    const PlanCase& pc = *(PlanCase*)h;
    const host::ScheduleBuilder& sb = pc.H.sb;
    const Program& G = sb.prog;
    Buffers B{};
    Scratch scratch(G, n, B);
    if (poison) {
        scratch.poison();
        for (size_t c = 0; c < (size_t)G.num_cols; c++)
            for (size_t i = 0; i < n; i++) cols[c * ld + i] = 0xA5A5A5A5A5A5A5A5ull;
    }
    B.msg = msg; B.r = r; B.s = s; B.pkx = pkx; B.pky = pky;
    B.qx = qx; B.qy = qy;   // the MSM program's second point (null for every other program)
    B.sink = Sink{cols, ld, nullptr, 0, nullptr, 0, nullptr};
    B.ops = sb.ops.data();
    if (pc.family == 0) {
        const host::Consts& C = host::consts();
        B.cpts = C.cpts; B.fbtab = C.fbtab.data();
        exec_plan<BuiltinBodies<Emit>>(pc.pl, G, B, 0, 0, order, n_order);
    } else {
        B.cpts = sb.gpts.data(); B.fbtab = sb.gfbtab.data();
        if (pc.curve == 1)
            exec_plan<CurveBodies<P256, Emit>>(pc.pl, G, B, 0, 0, order, n_order);
        else
            exec_plan<CurveBodies<Secp256k1, Emit>>(pc.pl, G, B, 0, 0, order, n_order);
    }
    return scratch.finalize(err, valid);
}
// The plan a call of `nominal` elements launches under the default knobs (default stream layout), executed on the n
// elements given: what lets a CPU test run the plan of a 2^16 call on a few signatures.
// cols != nullptr: the u64 column matrix, otherwise the compact container.
long emu_builtin_nominal(int program, const uint8_t* msg, const uint8_t* r, const uint8_t* s, const uint8_t* pkx, const uint8_t* pky,
                         uint64_t* cols, size_t ld, uint32_t* narrow, size_t ldn, uint64_t* wide, size_t ldw, size_t n, uint8_t* err,
                         uint8_t* valid, size_t nominal) {
    host::ScheduleBuilder sb;
    if (program == 0)
        sb.verify_secp256k1_message_circuit();
    else
        sb.glv_mul_circuit();
    const plan::BuiltinParams P = plan::choose_builtin(sb.prog, Tuning{}, nominal, plan::Layout{true, false}, false);
    return run(program, P, msg, r, s, pkx, pky, cols, n, ld, err, valid, 0, 0, narrow, ldn, wide, ldw);
}
long emu_curve_program_nominal(int kind, int curve, const uint8_t* blind_x, const uint8_t* blind_y, const uint8_t* msg, const uint8_t* r,
                               const uint8_t* s, const uint8_t* pkx, const uint8_t* pky, uint64_t* cols, size_t n, size_t ld, uint8_t* err,
                               uint8_t* valid, size_t nominal) {
    Aff blind;
    memcpy(blind.x.w, blind_x, 32);
    memcpy(blind.y.w, blind_y, 32);
    host::CurveProgramHost H;
    if (!host::make_curve_program(H, kind, curve, blind)) return -1;
    const Program& G = H.sb.prog;
    const plan::CurveParams P = plan::choose_curve(G, Tuning{}, nominal, G.msm_loop_iters > 0 || kind == CP_FIXED_BASE_MUL,
                                                   plan::Layout{true, false}, false, CallSwitches{});
    if (curve == 1) return run_curve<P256>(H, P, msg, r, s, pkx, pky, cols, n, ld, err, valid);
    return run_curve<Secp256k1>(H, P, msg, r, s, pkx, pky, cols, n, ld, err, valid);
}
// P2E_CP_MSM: curve_msm_circuit(p, q, n, m); as emu_curve_program with the second point (the program takes no blinding point)
long emu_curve_msm(int curve, const uint8_t* px, const uint8_t* py, const uint8_t* qx, const uint8_t* qy, const uint8_t* n_scalar,
                   const uint8_t* m_scalar, uint64_t* cols, size_t n, size_t ld, uint8_t* err, uint8_t* valid, int piece) {
    host::CurveProgramHost H;
    if (!host::make_curve_program(H, CP_MSM, curve, Aff{})) return -1;
    if (n == 0) return 0;
    const plan::CurveParams P = curve_legacy_params(piece);
    if (curve == 1) return run_curve<P256>(H, P, n_scalar, m_scalar, n_scalar, px, py, cols, n, ld, err, valid, qx, qy);
    return run_curve<Secp256k1>(H, P, n_scalar, m_scalar, n_scalar, px, py, cols, n, ld, err, valid, qx, qy);
}
// generator table (kind, field, first column, column count) and operand wiring of a curve program, for the host tests
long emu_curve_program_gens(int kind, int curve, const uint8_t* blind_x, const uint8_t* blind_y, int32_t* kinds, int32_t* fields,
                            uint32_t* first, uint32_t* ncols, uint32_t* src /*[4 per gen]*/, uint8_t* nl /*[4 per gen]*/, size_t cap) {
    Aff blind;
    memcpy(blind.x.w, blind_x, 32);
    memcpy(blind.y.w, blind_y, 32);
    host::CurveProgramHost H;
    if (!host::make_curve_program(H, kind, curve, blind)) return -1;
    const auto& g = H.sb.gens;
    for (size_t k = 0; k < g.size() && k < cap; k++) {
        kinds[k] = g[k].kind;
        fields[k] = g[k].field;
        first[k] = g[k].col;
        ncols[k] = g[k].ncols;
        for (int j = 0; j < 4; j++) {
            src[4 * k + j] = g[k].src[j];
            nl[4 * k + j] = g[k].nl[j];
        }
    }
    return (long)g.size();
}
// value of constant `id` of a curve program (source code AUX_SRC_CONST | id); 0, or -1 for an unknown id
int emu_curve_program_const(int kind, int curve, const uint8_t* blind_x, const uint8_t* blind_y, uint32_t id, uint8_t* out32) {
    Aff blind;
    memcpy(blind.x.w, blind_x, 32);
    memcpy(blind.y.w, blind_y, 32);
    host::CurveProgramHost H;
    if (!host::make_curve_program(H, kind, curve, blind)) return -1;
    id &= 0xFFFFu;
    if (id >= AUX_GCONST_BASE ? id - AUX_GCONST_BASE >= H.sb.gvals.size() : (id >> 1) >= H.sb.gpts.size()) return -1;
    const U256 v = H.sb.cval(id);
    memcpy(out32, v.w, 32);
    return 0;
}
// built-in-generator / gate-internal / constraint-block values of a curve program from finished matrices (the bodies
// kc_aux / k_gate / kc_ux run); each returns the matrix' column count (call with n = 0 to query it)
long emu_curve_aux(int kind, int curve, const uint8_t* blind_x, const uint8_t* blind_y, const uint8_t* msg, const uint8_t* r,
                   const uint8_t* s, const uint8_t* pkx, const uint8_t* pky, const uint64_t* cols, size_t ld, uint64_t* aux, size_t ald,
                   size_t n, uint8_t* err) {
    Aff blind;
    memcpy(blind.x.w, blind_x, 32);
    memcpy(blind.y.w, blind_y, 32);
    host::CurveProgramHost H;
    if (!host::make_curve_program(H, kind, curve, blind)) return -1;
    const host::ScheduleBuilder& sb = H.sb;
    if (n == 0) return (long)sb.aux_tab.num_aux_cols;
    std::vector<u32> err32(n);
    AuxArgs A{cols, ld, aux, ald, n, pky, sb.gpts.data(), sb.gfbtab.data(), sb.aux_items.data(), &sb.aux_tab, err32.data(), nullptr, 0, nullptr, {}};
    A.in[INPUT_PY] = pky;
    A.in[INPUT_PX] = pkx;
    A.in[INPUT_MSG] = msg;
    A.in[INPUT_R] = r ? r : msg;
    A.in[INPUT_S] = s ? s : msg;
    for (int item = 0; item < (int)sb.aux_items.size(); item++) {
#pragma omp parallel for
        for (long long i = 0; i < (long long)n; i++) body_aux_cv<Emit>(A, item, (size_t)i);
    }
    for (size_t i = 0; i < n; i++) err[i] = (uint8_t)err32[i];
    return (long)sb.aux_tab.num_aux_cols;
}
long emu_curve_gate(int kind, int curve, const uint8_t* blind_x, const uint8_t* blind_y, const uint64_t* aux, size_t ald, uint64_t* gate,
                    size_t gld, size_t n) {
    Aff blind;
    memcpy(blind.x.w, blind_x, 32);
    memcpy(blind.y.w, blind_y, 32);
    host::CurveProgramHost H;
    if (!host::make_curve_program(H, kind, curve, blind)) return -1;
    const host::ScheduleBuilder& sb = H.sb;
    if (n == 0) return (long)sb.num_gate_cols;
    GateArgs A{};
    A.aux = aux;
    A.ald = ald;
    A.gate = gate;
    A.gld = gld;
    A.n = n;
    A.items = sb.gate_items.data();
    A.inv16[0] = 0;
    for (u64 d = 1; d < 16; d++) {   // d^(p-2) in Goldilocks
        u64 acc = 1, base = d, e = P_GL - 2;
        while (e) {
            if (e & 1) acc = gl_mul(acc, base);
            base = gl_mul(base, base);
            e >>= 1;
        }
        A.inv16[d] = acc;
    }
    for (int item = 0; item < (int)sb.gate_items.size(); item++)
        for (size_t i = 0; i < n; i++) body_gate<Emit>(A, item, i);
    return (long)sb.num_gate_cols;
}
long emu_curve_ux(int kind, int curve, const uint8_t* blind_x, const uint8_t* blind_y, const uint8_t* msg, const uint8_t* r,
                  const uint8_t* s, const uint8_t* pkx, const uint8_t* pky, const uint64_t* cols, size_t ld, const uint64_t* aux,
                  size_t ald, uint64_t* ux, size_t uld, size_t n, uint8_t* err) {
    Aff blind;
    memcpy(blind.x.w, blind_x, 32);
    memcpy(blind.y.w, blind_y, 32);
    host::CurveProgramHost H;
    if (!host::make_curve_program(H, kind, curve, blind)) return -1;
    const host::ScheduleBuilder& sb = H.sb;
    if (n == 0) return (long)sb.num_ux_cols;
    std::vector<U256> cv(AUX_GCONST_BASE + sb.gvals.size(), u256_zero());
    for (size_t k = 0; k < sb.gpts.size(); k++) {
        cv[2 * k] = sb.gpts[k].x;
        cv[2 * k + 1] = sb.gpts[k].y;
    }
    for (size_t j = 0; j < sb.gvals.size(); j++) cv[AUX_GCONST_BASE + j] = sb.gvals[j];
    std::vector<u32> err32(n);
    UxArgs A{};
    A.cols = cols;
    A.ld = ld;
    A.aux = aux;
    A.ald = ald;
    A.ux = ux;
    A.uld = uld;
    A.n = n;
    A.in[INPUT_PY] = pky;
    A.in[INPUT_PX] = pkx;
    A.in[INPUT_MSG] = msg;
    A.in[INPUT_R] = r ? r : msg;
    A.in[INPUT_S] = s ? s : msg;
    A.consts = cv.data();
    A.items = sb.ux_items.data();
    A.err = err32.data();
#pragma omp parallel for
    for (long long item = 0; item < (long long)sb.ux_items.size(); item++)
        for (size_t i = 0; i < n; i++) body_ux_cv<Emit>(A, (int)item, i);
    for (size_t i = 0; i < n; i++) err[i] = (uint8_t)err32[i];
    return (long)sb.num_ux_cols;
}
// P-256 base field: the multiplication-free reduction of the chains (reduce_p256_solinas) against the Barrett reduction
// of the witness generators on `count` products of random and structured operands and on raw 512-bit values; returns
// the number of mismatches
long emu_p256_reduce_selfcheck(long count, uint64_t seed) {
    host::SplitMix64 rng{seed};
    long bad = 0;
    const u32 edge[6] = {0u, 1u, 0xFFFFFFFFu, 0xFFFFFFFEu, 0x80000000u, 0x7FFFFFFFu};
    for (long it = 0; it < count; it++) {
        u32 prod[16];
        if (it % 3 == 0) {   // a raw 512-bit value built from edge words and random words
            for (int k = 0; k < 16; k++) prod[k] = (rng.next() & 1) ? edge[rng.next() % 6] : (u32)rng.next();
        } else {             // a product of two field elements (canonical, or structured near 0 / p)
            U256 a, b;
            for (int k = 0; k < 8; k++) {
                a.w[k] = (it % 3 == 1) ? (u32)rng.next() : edge[rng.next() % 6];
                b.w[k] = (u32)rng.next();
            }
            a = fe_canon<ModP256>(a);
            b = fe_canon<ModP256>(b);
            if (it % 7 == 2)
                for (int k = 0; k < 8; k++) b.w[k] = ModP256::m(k) - (k == 0 ? 1u + (u32)(it & 3) : 0u);   // p - 1 .. p - 4
            mul_wide<8, 8>(a.w, b.w, prod);
        }
        u32 r1[8], r2[8];
        reduce_p256_solinas(prod, r1);
        reduce_barrett<ModP256, 8, false>(prod, r2, nullptr);
        for (int k = 0; k < 8; k++)
            if (r1[k] != r2[k]) {
                bad++;
                break;
            }
    }
    return bad;
}
// verdict only of the P-256 verifier program (p2e_p256_verify_batch): scalar phase without emission, the chains in
// Jacobian coordinates (table left Jacobian), r == x on the Jacobian result of the final add
long emu_p256_verify_only(const uint8_t* blind_x, const uint8_t* blind_y, const uint8_t* msg, const uint8_t* r, const uint8_t* s,
                          const uint8_t* pkx, const uint8_t* pky, size_t n, uint8_t* err, uint8_t* valid) {
    Aff blind;
    memcpy(blind.x.w, blind_x, 32);
    memcpy(blind.y.w, blind_y, 32);
    host::CurveProgramHost H;
    if (!host::make_curve_program(H, CP_VERIFY, 1, blind)) return -1;
    const host::ScheduleBuilder& sb = H.sb;
    const Program& G = sb.prog;
    Buffers B{};
    Scratch scratch(G, n, B);
    B.msg = msg; B.r = r; B.s = s; B.pkx = pkx; B.pky = pky;
    B.cpts = sb.gpts.data(); B.fbtab = sb.gfbtab.data(); B.ops = sb.ops.data();
    const int fb_end = G.fb_begin + G.fb_windows + 1;
#pragma omp parallel for
    for (long long i = 0; i < (long long)n; i++) {
        body_cscalar<P256, NullEmit>(G, B, (size_t)i);
        body_chain_range<P256, true>(G, B, (size_t)i, G.fb_begin, fb_end, false, false);
        body_chain_range<P256, true>(G, B, (size_t)i, fb_end, G.num_ops - 1, false, false);
        body_chain_range<P256, true>(G, B, (size_t)i, G.num_ops - 1, G.num_ops, false, false);
        body_verify_check<P256>(G, B, (size_t)i, G.num_ops - 1);
    }
    return scratch.finalize(err, valid);
}
int emu_synth_signatures_curve(int curve, uint64_t seed, size_t first, size_t n, uint8_t* msg32, uint8_t* r32, uint8_t* s32,
                               uint8_t* pkx32, uint8_t* pky32) {
#pragma omp parallel for
    for (long long i = 0; i < (long long)n; i++) {
        U256 msg, r, s;
        Aff pk;
        if (curve == 1)
            host::synth_signature_cv<P256>(seed, first + (u64)i, msg, r, s, pk);
        else
            host::synth_signature_cv<Secp256k1>(seed, first + (u64)i, msg, r, s, pk);
        memcpy(msg32 + 32 * i, msg.w, 32);
        memcpy(r32 + 32 * i, r.w, 32);
        memcpy(s32 + 32 * i, s.w, 32);
        memcpy(pkx32 + 32 * i, pk.x.w, 32);
        memcpy(pky32 + 32 * i, pk.y.w, 32);
    }
    return 0;
}
}

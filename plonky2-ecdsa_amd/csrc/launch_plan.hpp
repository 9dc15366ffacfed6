// Launch plans of the fused calls as data: WHICH chain piece runs on which stream, which inversion batch follows it,
// which expansion waits for which event, and in what order all of it is issued.  Host only, no HIP (like knobs.hpp):
// the library builds a plan per call and walks it with issue_plan (p2e_hip.hip), tests/emu builds the same plan with
// g++ and executes its compute steps in list order.
//
// A plan is made in two pure steps per family (built-in programs: run_program; curve programs: run_curve_program):
//   choose_*  (Program, Tuning, n, stream layout, timing, per-call switches) -> a small parameter record
//   build_*   (Program, parameter record)                                    -> the step list
// build takes the record and not Tuning, so that a test may ask for values no environment variable can set (a piece of
// 7 ops, say).
//
// The plan in words:
//   chains (latency-bound, sequential) : their own high-priority streams, cut into pieces
//   phase B of a piece                 : an inversion batch once the piece's chain kernel is done
//   phase C of a piece                 : the expansion stream(s), after its phase B (HBM-bound)
// so that the HBM-bound expansion of finished pieces hides the chains and inversions of later ones.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <algorithm>
#include <utility>
#include <vector>

#include "knobs.hpp"
#include "pipeline.hpp"

namespace p2e {
namespace plan {

constexpr int MAX_PIECES = Tuning::MAX_PIECES;
constexpr int MAX_SEG = 2 * MAX_PIECES + 2;   // pieces of one call: the context has an event pair for each
constexpr int MAX_EXPAND = 2 * MAX_SEG;       // expansion launches of one call (one event pair each)
constexpr int PIECES_CAP = 160;               // what Plan::max_seg may be raised to by a walker that needs no events (tests/emu)
constexpr int MAX_STEPS = 2560;               // (the one-wait-per-earlier-piece form of the four-lane plan is quadratic in the pieces)

// Streams and events by name; the issuer resolves them to the context's handles.
// ST_C1 is only ever named by a plan whose record says the layout has an own first expansion stream (otherwise the
// expansions go to ST_CALLER); Plan::masked_expand turns ST_C1 / ST_C2 into the CU-masked pair of the four-lane plan.
enum Stream : uint8_t { ST_CALLER, ST_M, ST_F, ST_B, ST_C1, ST_C2 };
enum EventKind : uint8_t { EV_FORK, EV_FIXED, EV_PIECE, EV_BINV, EV_C0, EV_C1, EV_C2, EV_C1JOIN, EV_T0, EV_T1, EV_T5 };
struct Event {
    EventKind kind;
    uint16_t idx;  // EV_PIECE / EV_BINV: the piece; EV_C0 / EV_C1: the expansion launch
};
enum StepKind : uint8_t { SCALAR, CHAIN, BINV, EXPAND_OPS, EXPAND_RUNS, EXPAND_FB_RUN, RECORD, WAIT, FINALIZE };
enum ChainForm : uint8_t { LANE, QUAD, ROWS };
// the op table a call binds: every op expanded on its own, or with the run marks of the large / mid-size / four-lane plan
// (curve programs have the first two)
enum OpTable : uint8_t { OPS_PLAIN, OPS_RUNS, OPS_MID, OPS_SMALL };

struct Step {
    StepKind kind;
    Stream stream;
    Event ev;         // RECORD / WAIT
    ChainForm form;   // CHAIN
    // CHAIN lane / quad: lo, hi, table_affine, continue_prefix;  CHAIN rows: lo, row count, count
    // BINV: lo, hi, have_prefix, split_log2
    // EXPAND_OPS: s_lo, s_hi;  EXPAND_RUNS: it0, it1, run_iters;  EXPAND_FB_RUN: t_after;  all three: d = expansion launch e
    int a, b, c, d;
};

enum Error { OK = 0, TOO_MANY_PIECES, BAD_SHAPE, BAD_ORDER, TOO_MANY_STEPS };

struct Plan {
    Step steps[MAX_STEPS];
    int n_steps = 0, n_seg = 0, n_expand = 0;
    int max_seg = MAX_SEG;        // pieces build may cut (at most PIECES_CAP), with two expansion launches each
    OpTable ops = OPS_PLAIN;
    unsigned expand_lds = 0;      // dynamic LDS of the expansion launches (the scalar phase launches with none)
    bool masked_expand = false;   // ST_C1 / ST_C2 are the CU-masked expansion streams (P2E_QUAD_EXPAND_CUS)
    Error error = OK;

    void push(const Step& s) {
        if (n_steps < MAX_STEPS)
            steps[n_steps++] = s;
        else
            error = TOO_MANY_STEPS;
    }
    void record(Event e, Stream st) { push(Step{RECORD, st, e, LANE, 0, 0, 0, 0}); }
    void wait(Stream st, Event e) { push(Step{WAIT, st, e, LANE, 0, 0, 0, 0}); }
    void compute(StepKind k, Stream st) { push(Step{k, st, Event{EV_FORK, 0}, LANE, 0, 0, 0, 0}); }
    void chain(Stream st, ChainForm form, int lo, int hi, int table_affine, int continue_prefix) {
        push(Step{CHAIN, st, Event{EV_FORK, 0}, form, lo, hi, table_affine, continue_prefix});
    }
    void binv(Stream st, int lo, int hi, int have_prefix, int split_log2) {
        push(Step{BINV, st, Event{EV_FORK, 0}, LANE, lo, hi, have_prefix, split_log2});
    }
    // one expansion launch with its event pair (the first of the pair only with P2E_CTX_PHASE_TIMING)
    void expand(StepKind k, Stream st, int a, int b, int c, bool timing) {
        if (n_expand >= 2 * max_seg) {
            error = TOO_MANY_STEPS;
            return;
        }
        const int e = n_expand++;
        if (timing) record(Event{EV_C0, (uint16_t)e}, st);
        push(Step{k, st, Event{EV_FORK, 0}, LANE, a, b, c, e});
        record(Event{EV_C1, (uint16_t)e}, st);
    }
};

// what the context's stream layout offers beyond the streams every plan needs (M, F, B, C2)
struct Layout {
    bool own_c1 = false;    // the library's OWN first expansion stream (P2E_STREAM_LAYOUT with a '1')
    bool masked = false;    // CU-masked expansion streams for the four-lane plan (P2E_QUAD_EXPAND_CUS)
};

// a piece of the op list: one chain kernel + one inversion batch + the expansion launches
struct Piece {
    int lo, hi;          // ops of phases A and B
    int order;           // built-in programs: readiness estimate (ops walked on its chain before it completes)
    Stream chain;        // chain stream
    bool final_after;    // built-in verify: append the final add (needs the fixed-base chain) to this piece
    bool table, wait_fb; // curve programs: the per-signature window table; needs the fixed-base chain (the final add)
    bool fb_run;         // phase C: the fixed-base windows as one run per signature (k_expand_fb_run) ...
    int it0, it1;        // ... loop iterations as runs (k_expand_runs) ...
    int s_lo, s_hi;      // ... ops one by one (k_expand)
};

// ====================================================================================================
// built-in programs (verify, glv_mul)
// ====================================================================================================
struct BuiltinParams {
    // three regimes: four lanes per signature (n <= quad_max_n), lane per signature with phase B on two streams and longer
    // runs in fewer pieces (below binv_alt_max_n), and the large-batch plan
    bool quad = false, mid = false;
    int run_iters = 0;   // MSM-loop iterations per expansion run (0: op by op)
    OpTable ops = OPS_PLAIN;
    int msm_pieces = 1, fixed_pieces = 1;
    int takes[MAX_PIECES + 1] = {0};   // four-lane plan: runs per loop piece, 0-terminated (empty: equal pieces)
    bool fb_run = false;   // the fixed-base windows as one run per signature
    bool alt_b = false;    // phase B of consecutive pieces on two streams
    // sub-ranges (log2) of an inversion batch: of the last piece, of a fixed-base piece, of every other one
    int split_last = 0, split_fixed = 0, split = 0;
    bool b_first_on_fixed = true, few_waits = true;
    Layout layout;
    bool timing = false;
    unsigned expand_lds = 0;
};

inline BuiltinParams choose_builtin(const Program& G, const Tuning& t, size_t n, Layout layout, bool timing) {
    BuiltinParams P;
    P.mid = n > t.quad_max_n && n < t.binv_alt_max_n;
    // small batches: four lanes per signature in phase A, split inversion batches in phase B (quad.hpp)
    P.quad = n <= t.quad_max_n;
    if (n >= t.runs_min_n) {
        P.run_iters = P.mid ? t.run_iters_mid : t.run_iters;
        if (P.run_iters > 0) P.ops = P.mid ? OPS_MID : OPS_RUNS;
    } else if (P.quad && t.run_iters_small > 0) {
        P.run_iters = t.run_iters_small;
        P.ops = OPS_SMALL;
    }
    const bool verify = G.num_chains == 3;
    P.msm_pieces = P.quad ? t.msm_pieces_small : P.mid ? t.msm_pieces_mid : t.msm_pieces;
    // with run expansion the fixed-base chain is ONE piece: its windows keep no X, Y / affine form in memory
    // (F_NO_AFFINE), so nothing could resume the chain from scratch in the middle
    P.fb_run = P.run_iters > 0 && verify && t.fb_run && G.fb_begin == G.chain_begin[1];
    P.fixed_pieces = P.fb_run ? 1 : P.quad ? t.fixed_pieces_small : t.fixed_pieces;
    // small-batch plan: an explicit list of runs per piece (the list is used while it fits; the last piece takes the rest)
    // default list for the runs of 4 iterations (19 runs): 6, 5, 5, 2 and the last run alone -- the last piece's inversion
    // batch and expansion are the exposed tail of the call (2.27 / 2.92 against 2.32 / 2.98 ms at 2^13 / 12 288 with
    // equal pieces, profiles/r03_quad_plan_piece_sizes_sweep.txt)
    static const int takes_r4[MAX_PIECES + 1] = {6, 5, 5, 2, 0};
    const int* takes = t.small_takes[0] > 0 ? t.small_takes
                       : (P.quad && P.run_iters == 4 && G.msm_loop_iters == MSM_DIGITS) ? takes_r4 : t.small_takes;
    if (P.quad)
        for (int k = 0; k < MAX_PIECES && takes[k] > 0; k++) P.takes[k] = takes[k];
    P.alt_b = P.quad || n < t.binv_alt_max_n;
    if (P.quad) {
        P.split = t.binv_split_log2;
        P.split_last = t.binv_split_log2_last;
        P.split_fixed = t.binv_split_log2_fixed;
    } else {
        P.split = P.split_last = P.split_fixed = P.alt_b ? t.binv_mid_split_log2 : 0;
    }
    P.b_first_on_fixed = t.quad_b_first_on_fixed;
    P.few_waits = t.quad_few_waits;
    // first expansion stream: the library's own if the layout has one (the caller's stream then waits for it at the end)
    P.layout.masked = P.quad && layout.masked;
    P.layout.own_c1 = layout.own_c1 || P.layout.masked;
    P.timing = timing;
    P.expand_lds = P.quad ? t.expand_lds_small : t.expand_lds;   // (only ever non-zero for the small-batch plan by default)
    return P;
}

inline bool build_builtin(const Program& G, const BuiltinParams& P, Plan& pl) {
    if (pl.max_seg > PIECES_CAP) pl.max_seg = PIECES_CAP;
    pl.n_steps = pl.n_seg = pl.n_expand = 0;
    pl.error = OK;
    pl.ops = P.ops;
    pl.expand_lds = P.expand_lds;
    pl.masked_expand = P.layout.masked;
    Piece segs[PIECES_CAP];
    int ns = 0;
    bool overflow = false;   // more pieces than the plan holds: the call fails (never a silently shorter op list)
    auto add = [&](const Piece& pc) {
        if (ns < pl.max_seg)
            segs[ns++] = pc;
        else
            overflow = true;
    };
    const bool verify = G.num_chains == 3, quad = P.quad;
    const int run_iters = P.run_iters;
    auto cut = [&](int lo, int hi, int pieces, Stream st) {
        if (pieces > hi - lo) pieces = hi - lo;
        int a = lo;
        for (int k = 0; k < pieces; k++) {
            int rem = pieces - k;
            int len = (hi - a + rem - 1) / rem;
            add(Piece{a, a + len, a + len - lo, st, false, false, false, false, 0, 0, a, a + len});
            a += len;
        }
    };
    if (verify) cut(G.chain_begin[1], G.chain_end[1], P.fixed_pieces, ST_F);
    if (P.fb_run && ns > 0) {   // windows as one run, then the unblinding add op by op
        segs[0].fb_run = true;
        segs[0].s_lo = G.fb_begin + G.fb_windows;
    }
    const int first_msm = ns;
    {
        // MSM chain = window table (its own piece: inverted first, read in affine form by everything after) +
        // the loop, cut at run boundaries into msm_pieces - 1 groups + the trailing unblinding add
        const int lo0 = G.chain_begin[0], hi0 = G.chain_end[0];
        const int lb = G.msm_loop_begin, iters = G.msm_loop_iters, le = lb + 3 * iters;
        const int R = run_iters > 0 ? run_iters : 1;
        const int nruns = (iters + R - 1) / R;
        int groups = P.msm_pieces > 1 ? P.msm_pieces - 1 : 1;
        if (groups > nruns) groups = nruns;
        int listed = 0;
        if (quad && P.takes[0] > 0) {
            int sum = 0;
            while (listed < MAX_PIECES - 1 && P.takes[listed] > 0 && sum + P.takes[listed] < nruns) sum += P.takes[listed++];
            groups = listed + 1;
        }
        add(Piece{lo0, lb, lb - lo0, ST_M, false, false, false, false, 0, 0, lo0, lb});
        int run = 0;
        for (int g = 0; g < groups; g++) {
            int rem = groups - g;
            int take = (nruns - run + rem - 1) / rem;
            if (listed) take = g < listed ? P.takes[g] : nruns - run;
            int it0 = run * R, it1 = (run + take) * R < iters ? (run + take) * R : iters;
            Piece sg{lb + 3 * it0, lb + 3 * it1, lb + 3 * it1 - lo0, ST_M, false, false, false, false, it0, it1, 0, 0};
            if (run_iters == 0) {   // no run expansion: op by op
                sg.s_lo = sg.lo;
                sg.s_hi = sg.hi;
                sg.it0 = sg.it1 = 0;
            }
            if (g == groups - 1) {     // trailing ops of the chain (the unblinding add)
                sg.hi = hi0;
                if (run_iters == 0) sg.s_hi = hi0; else { sg.s_lo = le; sg.s_hi = hi0; }
                sg.order = hi0 - lo0;
            }
            add(sg);
            run += take;
        }
    }
    if (overflow) {
        pl.error = TOO_MANY_PIECES;
        return false;
    }
    if (verify) segs[ns - 1].final_after = true;
    pl.n_seg = ns;

    const bool alt_b = P.alt_b;
    auto binv = [&](Stream st, int lo, int hi, int have_prefix, bool last_piece = false, bool fixed_piece = false) {
        pl.binv(st, lo, hi, have_prefix, last_piece ? P.split_last : fixed_piece ? P.split_fixed : P.split);
    };
    auto piece_ev = [](int k) { return Event{EV_PIECE, (uint16_t)k}; };
    auto binv_ev = [](int k) { return Event{EV_BINV, (uint16_t)k}; };
    const Event fork{EV_FORK, 0}, fixed{EV_FIXED, 0};
    if (P.timing) pl.record(Event{EV_T0, 0}, ST_CALLER);
    pl.compute(SCALAR, ST_CALLER);
    pl.record(Event{EV_T1, 0}, ST_CALLER);
    pl.record(fork, ST_CALLER);
    pl.wait(ST_M, fork);
    pl.wait(ST_F, fork);
    if (alt_b) pl.wait(ST_B, fork);
    const Stream st_c1 = P.layout.own_c1 ? ST_C1 : ST_CALLER, st_c2 = ST_C2;
    if (P.layout.own_c1) pl.wait(st_c1, fork);
    // chains
    for (int k = 0; k < ns; k++) {
        Piece& sg = segs[k];
        // once the table piece has been inverted on this stream (below), later pieces read the table affine
        // (small-batch plan: the FIRST loop piece does not wait for the table's inversion -- it reads the table in
        // Jacobian form, one level more per addition, and starts ~0.15 ms earlier; the table's phase B runs beside it)
        const int table_affine = (sg.chain == ST_M && k > first_msm + (quad ? 1 : 0)) ? 1 : 0;
        if (quad && k == first_msm + 2) pl.wait(ST_M, binv_ev(first_msm));
        // glv_mul alone: the window table as 2 chains of 4 adds, then 6 and 9 independent adds (body_chain_rows):
        // -6 % at 2^10, -4 % at 2^16.  Not in the verify program: there the fixed-base chain runs beside it, three
        // 186-VGPR waves do not fit a SIMD and the rows only queue (+0.6...1 % measured).
        const bool table_rows = (!verify || quad) && k == first_msm && sg.hi - sg.lo == MSM_TABLE_OPS;
        if (table_rows) {
            pl.chain(sg.chain, ROWS, sg.lo, 2, 4, 0);
            pl.chain(sg.chain, ROWS, sg.lo + 8, 6, 1, 0);
            pl.chain(sg.chain, ROWS, sg.lo + 14, 9, 1, 0);
        } else {
            pl.chain(sg.chain, quad ? QUAD : LANE, sg.lo, sg.hi, table_affine, 0);
        }
        if (verify && k == first_msm - 1) pl.record(fixed, ST_F);
        if (sg.final_after) {
            pl.wait(ST_M, fixed);
            // the final add joins the inversion batch of the last MSM piece
            pl.chain(ST_M, quad ? QUAD : LANE, G.chain_begin[2], G.chain_end[2], 0, 1);
            sg.hi = G.chain_end[2];
            sg.s_hi = G.chain_end[2];
        }
        pl.record(piece_ev(k), sg.chain);
        if (k == first_msm) {
            // The first MSM piece is the 23-op table build.  Its phase B runs right here on the chain's own
            // stream (the rest of the chain is not on the critical path: it ends long before the expansion
            // does), so that the first k_expand can start ~0.8 ms earlier than if it queued behind the
            // fixed-base chain on the other stream.
            const Stream st_tab = quad ? ST_B : ST_M;
            if (quad) pl.wait(st_tab, piece_ev(k));
            binv(st_tab, sg.lo, sg.hi, table_rows ? 0 : 1);
            pl.record(binv_ev(k), st_tab);
        }
    }
    // order of phases B / C: by readiness
    int order[PIECES_CAP];
    for (int k = 0; k < ns; k++) order[k] = k;
    for (int a = 1; a < ns; a++)
        for (int b = a; b > 0 && segs[order[b]].order < segs[order[b - 1]].order; b--) {
            int t = order[b];
            order[b] = order[b - 1];
            order[b - 1] = t;
        }
    bool used_c2 = false;
    int last_b[2] = {-1, quad ? first_msm : -1};   // most recent inversion batch on ST_F / ST_B (the table's: above)
    for (int q = 0; q < ns; q++) {
        const int k = order[q];
        const Piece& sg = segs[k];
        // HIP multiplexes streams onto a few hardware queues (4 by default) and kernels of one queue run
        // in order: a dedicated inversion stream ended up sharing the caller's queue and serialised B
        // with C.  The fixed-base chain's stream is idle after its first ~1 ms, so phase B lives there.
        // (small-batch plan: phase B of consecutive pieces alternates between two streams, so that an inversion batch
        // does not queue behind the previous one -- there the chains are no slower than phase B)
        const bool b_odd = (q & 1) != (quad && P.b_first_on_fixed ? 1 : 0);
        const Stream st_b = (alt_b && b_odd) ? ST_B : ST_F;
        if (k != first_msm) {
            pl.wait(st_b, piece_ev(k));
            binv(st_b, sg.lo, sg.hi, 1, k == ns - 1, k < first_msm);
            pl.record(binv_ev(k), st_b);
            last_b[st_b == ST_B ? 1 : 0] = k;
        }
        // (small-batch plan: phase C alternates between the caller's stream and a second one, so that an expansion
        // waiting for its inversion batch does not hold up the expansions queued behind it)
        const Stream st_c = (quad && (q & 1)) ? st_c2 : st_c1;
        used_c2 = used_c2 || st_c == st_c2;
        pl.wait(st_c, binv_ev(k));
        // an expansion also reads affine results of EARLIER pieces (the first operand of its first op, the window
        // table, the fixed-base result under the final add): with one expansion stream the queue order implied
        // their inversion batches, with two it has to be said
        // (the inversion batches sit on two in-order streams: the most recent one of each implies every earlier one, so
        // two waits say what q of them used to -- 28 barrier packets less on the expansion streams of a verify call;
        // tests/test_plan_order_cpu.py drops each of them in turn: from the second loop piece on the wait on the OTHER
        // inversion stream's batch is needed, the rest of the many-waits list is implied -- DESIGN.md section 5)
        if (quad) {
            if (P.few_waits) {
                for (int sb = 0; sb < 2; sb++)
                    if (last_b[sb] >= 0 && last_b[sb] != k) pl.wait(st_c, binv_ev(last_b[sb]));
            } else {
                for (int q2 = 0; q2 < q; q2++) pl.wait(st_c, binv_ev(order[q2]));
            }
        }
        if (sg.it1 > sg.it0) pl.expand(EXPAND_RUNS, st_c, sg.it0, sg.it1, run_iters, P.timing);
        if (sg.fb_run) pl.expand(EXPAND_FB_RUN, st_c, G.fb_begin + G.fb_windows, 0, 0, P.timing);
        if (sg.s_hi > sg.s_lo) pl.expand(EXPAND_OPS, st_c, sg.s_lo, sg.s_hi, 0, P.timing);
    }
    if (used_c2) {   // join the second expansion stream
        pl.record(Event{EV_C2, 0}, st_c2);
        pl.wait(ST_CALLER, Event{EV_C2, 0});
    }
    if (P.layout.own_c1) {
        pl.record(Event{EV_C1JOIN, 0}, st_c1);
        pl.wait(ST_CALLER, Event{EV_C1JOIN, 0});
    }
    if (P.timing) pl.record(Event{EV_T5, 0}, ST_CALLER);
    pl.compute(FINALIZE, ST_CALLER);
    return pl.error == OK;
}

// ====================================================================================================
// curve programs (curves.hpp, curve_program.hpp)
// ====================================================================================================
constexpr int CP_PIECE_OPS = 32;
constexpr int CP_PIECE_OPS_QUAD = 45;   // four-lane plan: 9 windows of the windowed loop per piece
constexpr int CP_TAIL_OPS_QUAD = 17;    // ... and a last piece of 3 windows + the trailing adds
constexpr int CP_RUN_OPS = 30;   // ops per expansion run of a loop: 6 windows of the windowed loop, 10 digits of the MSM
// loop iterations per expansion run (the op stride of an iteration is its doublings + the conditional add)
inline int cp_run_iters(const Program& G) { return CP_RUN_OPS / (G.loop_dbls + 1); }

// the per-signature window table = the ops the msm_tab slots refer to ([-1, -1): the program has none)
inline void cp_table_range(const Program& G, int& tb, int& te) {
    tb = te = -1;
    if (G.cp_table_ops > 0) {
        te = 0;
        for (int k = 1; k < 16; k++) {
            const int t = (int)ref_id(G.msm_tab[k]) + 1;
            if (t > te) te = t;
        }
        tb = te - G.cp_table_ops;
    }
}

struct CurveParams {
    // large batches: the windowed loop as runs and the fixed-base windows as one run (a run is walked by ONE lane, so
    // below cp_runs_min_n the SIMDs are better filled op by op, as in the built-in programs); the verifier's fixed-base
    // chain then runs beside the windowed chain on its own stream
    bool runs = false;
    // small batches: the chains are pure latency (429 dependent ops in the P-256 verifier): four lanes per signature walk
    // them, every inversion batch is cut into 2^binv_split_log2 sub-ranges, and the expansion kernels ask for dynamic LDS
    // they do not use so that one workgroup per CU leaves the register file to the chain waves (as the built-in programs'
    // four-lane plan)
    bool quad = false;
    int run_iters = 0;   // loop iterations per expansion run (runs plan)
    // ops per piece: the expansions are nowhere near the critical path of a small batch (the chain is), so its pieces are
    // longer: fewer launches and inversion batches on the chain's way
    int piece_ops = CP_PIECE_OPS;
    int tail_ops = 0;    // four-lane plan: a SHORT last piece -- its inversion batch and expansion are the exposed tail of the call
    // the verifier's fixed-base chain (67 ops) does not depend on the windowed chain: its pieces go to the second
    // chain stream and run beside the table / loop pieces; only the final add needs both (P2E_CP_FB_SERIAL=1: one
    // chain stream, as in round 2)
    bool fb_beside = false;
    // (op-by-op plan: the inversion batches of consecutive pieces alternate between two streams, as in the mid-size plan
    // of the built-in programs -- they are latency-bound and would otherwise queue behind each other)
    bool alt_b = false;
    int split = 0;       // sub-ranges (log2) of every inversion batch
    bool own_c1 = false, timing = false;
    unsigned expand_lds = 0;
};

inline CurveParams choose_curve(const Program& G, const Tuning& t, size_t n, bool has_runs_table, Layout layout, bool timing,
                                const CallSwitches& sw) {
    CurveParams P;
    P.runs = has_runs_table && n >= t.cp_runs_min_n && !sw.cp_no_runs;
    P.quad = !P.runs && n <= t.cp_quad_max_n && !sw.cp_no_quad;
    P.run_iters = cp_run_iters(G);
    P.piece_ops = P.quad ? CP_PIECE_OPS_QUAD : CP_PIECE_OPS;
    int tail_ops_quad = CP_TAIL_OPS_QUAD;
    // tuning knobs (tools/bench_curve_programs.py sweeps)
    if (sw.cp_piece_ops_quad_set && P.quad && sw.cp_piece_ops_quad >= 8 && sw.cp_piece_ops_quad <= 200) P.piece_ops = sw.cp_piece_ops_quad;
    if (sw.cp_tail_ops_quad_set && sw.cp_tail_ops_quad >= 0 && sw.cp_tail_ops_quad <= 100) tail_ops_quad = sw.cp_tail_ops_quad;
    P.tail_ops = P.quad ? tail_ops_quad : 0;
    int tb, te;
    cp_table_range(G, tb, te);
    P.fb_beside = !P.runs && tb >= 0 && G.fb_begin == 0 && tb == G.fb_begin + G.fb_windows + 1 && !sw.cp_fb_serial;
    P.alt_b = !P.runs && n < t.binv_alt_max_n && !sw.cp_no_alt_b;
    P.split = P.quad ? t.binv_split_log2 : 0;
    // the expansions run on the library's own first expansion stream when the stream layout has one (p2e_ctx_create)
    P.own_c1 = layout.own_c1;
    P.timing = timing;
    P.expand_lds = P.quad ? t.expand_lds_small : 0;
    return P;
}

inline bool build_curve(const Program& G, const CurveParams& P, Plan& pl) {
    if (pl.max_seg > PIECES_CAP) pl.max_seg = PIECES_CAP;
    pl.n_steps = pl.n_seg = pl.n_expand = 0;
    pl.error = OK;
    pl.ops = P.runs ? OPS_RUNS : OPS_PLAIN;
    pl.expand_lds = P.expand_lds;
    pl.masked_expand = false;
    Piece pieces[PIECES_CAP];
    int np = 0;
    int tb, te;
    cp_table_range(G, tb, te);
    bool overflow = false;   // more pieces than the plan holds: the call fails (never a silently shorter op list)
    auto add = [&](const Piece& pc) {
        if (pc.hi <= pc.lo) return;
        if (np < pl.max_seg)
            pieces[np++] = pc;
        else
            overflow = true;
    };
    const bool runs = P.runs, quad = P.quad, fb_beside = P.fb_beside;
    const int piece_ops = P.piece_ops > 0 ? P.piece_ops : 1;
    auto cut = [&](int lo, int hi) {   // chunks of <= piece_ops ops, expanded op by op
        if (hi <= lo) return;
        const int chunks = (hi - lo + piece_ops - 1) / piece_ops;
        for (int k = 0; k < chunks; k++) {
            const int a = lo + (int)((long long)(hi - lo) * k / chunks), b = lo + (int)((long long)(hi - lo) * (k + 1) / chunks);
            add(Piece{a, b, 0, ST_M, false, false, false, false, 0, 0, a, b});
        }
    };
    const int stride = G.loop_dbls + 1, run_iters = P.run_iters;   // ops per loop iteration, iterations per run
    if (runs && G.msm_loop_iters == 0) {
        // the fixed-base program: its windows as one run per signature, then the unblinding add (one piece)
        add(Piece{G.fb_begin, G.num_ops, 0, ST_M, false, false, false, true, 0, 0, G.fb_begin + G.fb_windows, G.num_ops});
        if (overflow || G.fb_begin != 0 || np != 1) {
            pl.error = BAD_SHAPE;
            return false;
        }
    } else if (runs) {
        const int lb = G.msm_loop_begin, iters = G.msm_loop_iters, le = lb + stride * iters;
        int fb_end = 0;
        if (G.fb_begin >= 0) {   // verifier: fixed-base windows + unblinding add, one piece on the second chain stream
            fb_end = G.fb_begin + G.fb_windows + 1;
            add(Piece{G.fb_begin, fb_end, 0, ST_F, false, false, false, true, 0, 0, G.fb_begin + G.fb_windows, fb_end});
        }
        add(Piece{tb, te, 0, ST_M, false, true, false, false, 0, 0, tb, te});
        if (run_iters <= 0) {
            pl.error = BAD_SHAPE;
            return false;
        }
        for (int it = 0; it < iters; it += run_iters) {
            const int it1 = it + run_iters < iters ? it + run_iters : iters;
            Piece pc{lb + stride * it, lb + stride * it1, 0, ST_M, false, false, false, false, it, it1, 0, 0};
            if (it1 == iters) {   // the last run takes the trailing ops (unblinding add, the verifier's final add)
                pc.hi = G.num_ops;
                pc.s_lo = le;
                pc.s_hi = G.num_ops;
                pc.wait_fb = G.fb_begin >= 0;
            }
            add(pc);
        }
        if (overflow || tb != fb_end || np == 0 || pieces[np - 1].hi != G.num_ops) {
            pl.error = BAD_SHAPE;
            return false;
        }
    } else {
        if (tb >= 0) {
            const int first_fb = np;
            cut(0, tb);
            if (fb_beside)
                for (int k = first_fb; k < np; k++) pieces[k].chain = ST_F;
            add(Piece{tb, te, 0, ST_M, false, true, false, false, 0, 0, tb, te});
            const int tail_ops = G.num_ops - te > 2 * P.tail_ops ? P.tail_ops : 0;
            cut(te, G.num_ops - tail_ops);
            cut(G.num_ops - tail_ops, G.num_ops);
            if (fb_beside && np > 0) pieces[np - 1].wait_fb = true;
        } else {
            cut(0, G.num_ops);
        }
        if (overflow || np == 0 || pieces[np - 1].hi != G.num_ops) {
            pl.error = TOO_MANY_PIECES;
            return false;
        }
    }
    pl.n_seg = np;
    auto piece_ev = [](int k) { return Event{EV_PIECE, (uint16_t)k}; };
    auto binv_ev = [](int k) { return Event{EV_BINV, (uint16_t)k}; };
    const Event fork{EV_FORK, 0}, fixed{EV_FIXED, 0};
    if (P.timing) pl.record(Event{EV_T0, 0}, ST_CALLER);
    pl.compute(SCALAR, ST_CALLER);
    pl.record(Event{EV_T1, 0}, ST_CALLER);
    pl.record(fork, ST_CALLER);
    pl.wait(ST_M, fork);
    pl.wait(ST_F, fork);
    pl.wait(ST_B, fork);
    if (fb_beside || quad) pl.wait(ST_C2, fork);
    // phases A and B of every piece
    bool table_done = false;
    int table_piece = -1, pieces_after_table = 0;
    for (int k = 0; k < np; k++) {
        const Piece& pc = pieces[k];
        // four-lane plan: the table's inversion batch runs OFF the chain stream and the first piece after the table reads
        // the table in Jacobian form (one level more per window addition) instead of waiting 0.3 ms for it; from the
        // second piece on the chain waits for the inversion (long done) and reads the table in affine form
        if (quad && table_piece >= 0 && pc.chain == ST_M && !pc.table) {
            if (pieces_after_table == 1) {
                pl.wait(ST_M, binv_ev(table_piece));
                table_done = true;
            }
            pieces_after_table++;
        }
        if (pc.wait_fb) pl.wait(pc.chain, fixed);
        pl.chain(pc.chain, quad ? QUAD : LANE, pc.lo, pc.hi, (table_done && pc.chain == ST_M) ? 1 : 0, 0);
        pl.record(piece_ev(k), pc.chain);
        if (pc.chain == ST_F) pl.record(fixed, ST_F);
        // the table's inversion runs on the chain stream itself (everything after it reads the table affine), the
        // fixed-base piece's behind its own chain, the others on the inversion stream (on the fixed-base stream a
        // verifier's first windowed pieces would queue behind that 67-op chain)
        // (fixed-base chain beside the windowed one: ST_F carries chain pieces, so the inversion batches alternate
        // between the inversion stream and the otherwise idle second expansion stream)
        // (four-lane plan: the table's batch goes to the second expansion stream, which has nothing queued yet -- the first
        // piece after the table's successor waits for it --, the fixed-base pieces' batches to the inversion stream)
        const Stream st_b = pc.table ? (quad ? ST_C2 : ST_M)
                            : (fb_beside && quad && pc.chain == ST_F) ? ST_B
                            : fb_beside ? ((k & 1) ? ST_B : ST_C2)
                            : !runs ? ((P.alt_b && (k & 1)) ? ST_B : ST_F)
                            : pc.chain == ST_F ? ST_F : ST_B;
        if (st_b != pc.chain) pl.wait(st_b, piece_ev(k));
        pl.binv(st_b, pc.lo, pc.hi, 1, quad && P.split > 0 ? P.split : 0);
        pl.record(binv_ev(k), st_b);
        if (pc.table) {
            table_piece = k;
            if (!quad) table_done = true;
        }
    }
    const Stream st_x = P.own_c1 ? ST_C1 : ST_CALLER;
    if (P.own_c1) pl.wait(ST_C1, fork);
    // phase C by readiness: the table first, the fixed-base run after the first loop piece (its chain is 67 ops long)
    int order[PIECES_CAP];
    int no = 0;
    if (runs && G.fb_begin >= 0 && G.msm_loop_iters > 0) {   // (the verifier; the fixed-base program is one piece)
        order[no++] = 1;
        if (np > 2) order[no++] = 2;
        order[no++] = 0;
        for (int k = 3; k < np; k++) order[no++] = k;
    } else {
        for (int k = 0; k < np; k++) order[no++] = k;
    }
    for (int q = 0; q < no; q++) {
        const int k = order[q];
        if (k >= np) {
            pl.error = BAD_ORDER;
            return false;
        }
        const Piece& pc = pieces[k];
        pl.wait(st_x, binv_ev(k));
        // an expansion also reads affine results of earlier pieces: with the inversions on two streams say so
        if (runs && q > 0) pl.wait(st_x, binv_ev(k > 0 ? k - 1 : 0));
        if (pc.wait_fb) pl.wait(st_x, binv_ev(0));
        if (pc.fb_run) pl.expand(EXPAND_FB_RUN, st_x, G.fb_begin + G.fb_windows, 0, 0, P.timing);
        if (pc.it1 > pc.it0) pl.expand(EXPAND_RUNS, st_x, pc.it0, pc.it1, run_iters, P.timing);
        if (pc.s_hi > pc.s_lo) pl.expand(EXPAND_OPS, st_x, pc.s_lo, pc.s_hi, 0, P.timing);
    }
    if (P.own_c1) {
        pl.record(Event{EV_C1JOIN, 0}, ST_C1);
        pl.wait(ST_CALLER, Event{EV_C1JOIN, 0});
    }
    if (P.timing) pl.record(Event{EV_T5, 0}, ST_CALLER);
    pl.compute(FINALIZE, ST_CALLER);
    return pl.error == OK;
}

// ====================================================================================================
// column blocks of a call (include/p2e.h p2e_segments_describe): a pure function of the program, its op table and the plan
// ====================================================================================================
// event: -1 = the scalar phase (EV_T1), otherwise the expansion launch e whose EV_C1[e] says the block is final
struct ColumnBlock {
    uint32_t first_col, num_cols;
    int event;
};
inline uint32_t op_cols(const OpDesc& op) { return op.kind == OP_DBL ? COLS_DBL : op.kind == OP_CADD ? COLS_CADD : COLS_ADD; }
// the ops an expansion step completes: [lo, hi)
inline void expand_ops(const Program& G, const Step& s, int loop_stride, int& lo, int& hi) {
    lo = hi = 0;
    if (s.kind == EXPAND_OPS) {
        lo = s.a;
        hi = s.b;
    } else if (s.kind == EXPAND_RUNS) {
        lo = G.msm_loop_begin + loop_stride * s.a;
        hi = G.msm_loop_begin + loop_stride * s.b;
    } else if (s.kind == EXPAND_FB_RUN) {
        lo = G.fb_begin;
        hi = G.fb_begin + G.fb_windows;
    }
}
// Disjoint blocks that cover every column of the program once.  First the columns no curve op owns (the scalar phase writes
// them: the complement of the ops' column ranges), then, in issue order, the columns of every expansion launch -- one
// block per contiguous run of columns, because consecutive ops of a launch are NOT always consecutive generators (the
// curve programs place a 10-column scalar generator between their last ops); every block of a launch carries its event.
// loop_stride: ops per iteration of the loop at G.msm_loop_begin (3 in the built-in programs, G.loop_dbls + 1 otherwise).
inline std::vector<ColumnBlock> column_blocks(const Program& G, const std::vector<OpDesc>& ops, const Plan& pl, int loop_stride) {
    std::vector<ColumnBlock> out;
    std::vector<std::pair<uint32_t, uint32_t>> r;
    auto runs_of = [&](int event) {   // r -> one block per maximal run of touching ranges
        std::sort(r.begin(), r.end());
        for (size_t k = 0; k < r.size();) {
            uint32_t c0 = r[k].first, c1 = r[k].second;
            for (k++; k < r.size() && r[k].first <= c1; k++) c1 = std::max(c1, r[k].second);
            out.push_back({c0, c1 - c0, event});
        }
    };
    r.reserve(ops.size());
    for (const OpDesc& op : ops) r.push_back({op.col, op.col + op_cols(op)});
    std::sort(r.begin(), r.end());
    uint32_t at = 0;
    for (const auto& x : r) {
        if (x.first > at) out.push_back({at, x.first - at, -1});
        at = std::max(at, x.second);
    }
    if (at < (uint32_t)G.num_cols) out.push_back({at, (uint32_t)G.num_cols - at, -1});
    for (int k = 0; k < pl.n_steps; k++) {
        const Step& s = pl.steps[k];
        if (s.kind != EXPAND_OPS && s.kind != EXPAND_RUNS && s.kind != EXPAND_FB_RUN) continue;
        int lo, hi;
        expand_ops(G, s, loop_stride, lo, hi);
        r.clear();
        for (int t = lo; t < hi; t++) r.push_back({ops[(size_t)t].col, ops[(size_t)t].col + op_cols(ops[(size_t)t])});
        runs_of(s.d);
    }
    return out;
}

// ====================================================================================================
// text form: one line per step, then one line of what the plan binds (tests/golden/launch_plans.txt.gz)
// ====================================================================================================
inline const char* stream_name(Stream s) {
    static const char* const names[] = {"caller", "M", "F", "B", "C1", "C2"};
    return names[s];
}
inline int event_name(Event e, char* out, size_t cap) {
    static const char* const names[] = {"fork", "fixed", "piece", "binv", "c0", "c1", "c2", "c1join", "t0", "t1", "t5"};
    const bool indexed = e.kind == EV_PIECE || e.kind == EV_BINV || e.kind == EV_C0 || e.kind == EV_C1;
    return indexed ? snprintf(out, cap, "%s[%d]", names[e.kind], (int)e.idx) : snprintf(out, cap, "%s", names[e.kind]);
}
// returns the length of the text (as snprintf: the text is cut at cap - 1)
inline size_t dump(const Plan& pl, char* out, size_t cap) {
    size_t len = 0;
    char ev[24];
    auto line = [&](const char* fmt, auto... args) {
        const int k = snprintf(len < cap ? out + len : nullptr, len < cap ? cap - len : 0, fmt, args...);
        if (k > 0) len += (size_t)k;
    };
    static const char* const ops_names[] = {"plain", "runs", "mid", "small"};
    for (int i = 0; i < pl.n_steps; i++) {
        const Step& s = pl.steps[i];
        const char* st = stream_name(s.stream);
        switch (s.kind) {
        case SCALAR: line("SCALAR st=%s\n", st); break;
        case CHAIN:
            if (s.form == ROWS)
                line("CHAIN st=%s form=rows lo=%d rows=%d count=%d\n", st, s.a, s.b, s.c);
            else
                line("CHAIN st=%s form=%s lo=%d hi=%d affine=%d cont=%d\n", st, s.form == QUAD ? "quad" : "lane", s.a, s.b, s.c, s.d);
            break;
        case BINV: line("BINV st=%s lo=%d hi=%d prefix=%d split=%d\n", st, s.a, s.b, s.c, s.d); break;
        case EXPAND_OPS: line("EXPAND_OPS st=%s s_lo=%d s_hi=%d\n", st, s.a, s.b); break;
        case EXPAND_RUNS: line("EXPAND_RUNS st=%s it0=%d it1=%d run_iters=%d\n", st, s.a, s.b, s.c); break;
        case EXPAND_FB_RUN: line("EXPAND_FB_RUN st=%s t_after=%d\n", st, s.a); break;
        case RECORD:
            event_name(s.ev, ev, sizeof ev);
            line("RECORD ev=%s st=%s\n", ev, st);
            break;
        case WAIT:
            event_name(s.ev, ev, sizeof ev);
            line("WAIT st=%s ev=%s\n", st, ev);
            break;
        case FINALIZE: line("FINALIZE st=%s\n", st); break;
        }
    }
    line("END ops=%s lds=%u n_seg=%d\n", ops_names[pl.ops], pl.expand_lds, pl.n_seg);
    return len;
}

}  // namespace plan
}  // namespace p2e

// Tuning knobs of a context: the values the launch plans (launch_plan.hpp choose_builtin / choose_curve) read, their
// defaults with the measurements behind them, and the ONE table that fills them from the environment when a context is
// created (p2e_ctx_create).  Host only, no HIP: tests/emu drives read_tuning with a getenv of its own.
//
// Read on every call instead (CallSwitches, read_call_switches below): P2E_NARROW_STORES and the curve-program switches
// P2E_CP_NO_RUNS, P2E_CP_NO_QUAD, P2E_CP_NO_ALT_B, P2E_CP_FB_SERIAL, P2E_CP_PIECE_OPS_QUAD and P2E_CP_TAIL_OPS_QUAD: a test
// may toggle them between two calls on one context.  The two launchers (run_program, run_curve_program) read them once, in
// their first lines, and hand them to the plan; nothing below the launchers looks at the environment.
// P2E_STREAM_LAYOUT, P2E_TOUCH_STREAMS, P2E_QUAD_EXPAND_CUS and P2E_QUAD_EXPAND_CU_PATTERN belong to the stream setup
// of p2e_ctx_create.
#pragma once
#include <cstddef>
#include <cstdlib>

namespace p2e {

struct Tuning {
    static constexpr int MAX_PIECES = 16;
    static constexpr int MAX_RUN_ITERS = 73;   // = MSM_DIGITS (pipeline.hpp), asserted in p2e_hip.hip
    int msm_pieces = 8, fixed_pieces = 2;   // one Montgomery inversion batch per piece
    int msm_pieces_small = 5, fixed_pieces_small = 1;   // ... of the small-batch plan (fewer launches and inversions)
    int run_iters = 9;                      // MSM-loop iterations per expansion run (0: expand op by op)
    // with runs: the fixed-base windows as one run per signature (k_expand_fb_run).  OFF by default in the built-in
    // verifier: measured 11.43 / 11.05 ms against 10.86 / 11.28 ms per 2^16 batch (alternating processes on one box) --
    // the single run has one wave per SIMD and lands in the window where the chains and inversions contend with it
    // (0.40-0.42 of peak against 0.43-0.47 for the same columns through k_expand); P2E_FB_RUN=1 turns it on.  The
    // P-256 verifier program uses it (curve_api.inc), where it sits beside a longer windowed chain.
    bool fb_run = false;
    // A run is walked by ONE lane, so a launch of r runs has only r * n/64 waves: below this batch size the
    // 1024 SIMDs are better filled by one workgroup row per op (2^10 glv_mul fills: 3.0 ms against 9.5 ms)
    size_t runs_min_n = 21505;              // (= every batch the four-lane plan does not take, see quad_max_n)
    size_t cp_runs_min_n = 49152;           // the same threshold for the curve programs (curve_api.inc), measured there only at 2^13 / 2^16
    // Below this batch size phases A and B are latency, not throughput: four lanes per signature walk the chains
    // (k_chains_quad) and every inversion batch is cut into 2^binv_split_log2 sub-ranges (k_batch_inv_split)
    // (24 576 until phase B of the lane-per-signature plan went onto two streams below binv_alt_max_n: since then that plan
    // wins from 2^14 up -- 3.94 against 4.60 ms at 16 384, 4.96 against 6.46 ms at 24 576, 3.81 against 3.62 ms at 12 288)
    // (round 3, with short expansion runs and front-loaded pieces: 3.56-3.76 against 4.10-4.15 ms at 16 384, 4.73 against
    // 4.5 ms at 20 480, profiles/r03_plan_threshold_resweep.txt -- the threshold moved up from 14 336 and now takes 2^14)
    // (with the chains on lazy limbs and the safegcd inversion: 3.44-3.52 against 3.96-4.03 ms at 16 384, 4.05-4.28 against
    // 4.25-4.35 at 20 480, 5.01-5.04 against 4.72-4.73 at 24 576, profiles/r03_plan_threshold_lazy_limbs.txt: 17 408 -> 21 504)
    size_t quad_max_n = 21504;
    size_t cp_quad_max_n = 17408;   // the curve programs' own threshold (P-256 keeps canonical words: measured with those)
    // Between the two plans (lane per signature, but fewer than one chain wave per SIMD) phase B is the serial resource:
    // its kernels are latency-bound (half a wave per SIMD at 2^15) and queue on one stream from the first piece to the
    // last, with every expansion waiting behind them.  Below this batch size the inversion batches of consecutive pieces
    // alternate between two streams -- and are cut into 2^binv_mid_split_log2 sub-ranges each -- so that they overlap.
    size_t binv_alt_max_n = 49152;
    // ... and the loop is cut into fewer pieces of longer runs there (5 pieces of 12-iteration runs instead of 8 of 9:
    // 5.96 against 6.45 ms at 2^15, 7.65 against 7.95 ms at 40 960, 9.15 against 9.53 ms at 48 896)
    int msm_pieces_mid = 5, run_iters_mid = 12;
    // four-lane plan: the loop expanded as SHORT runs (4 iterations = 12 ops, two of them keep their affine form): phase B
    // then does 3 instead of 8 multiplications for the other ten, and a piece of 5 runs still launches 5 * n/64 waves.
    // 2.35 / 2.27 against 2.42 ms at 2^13, 2.88 / 2.96 against 3.05 ms at 12 288 (profiles/r03_quad_plan_run_expansion_sweep.txt;
    // R = 2, 3, 6 and 7 pieces are slower).  0: every op expanded on its own, as in round 2.
    int run_iters_small = 4;
    int binv_mid_split_log2 = 1;   // 2^15 per call: 7.03-7.08 ms on one stream, 6.76-6.83 alternating, 6.68-6.72 alternating and split in two
    int binv_split_log2 = 2;
    // small-batch plan: dynamic LDS bytes requested by the expansion kernels (they do not use it): caps how many of
    // their workgroups share a CU, so that the register file keeps room for the chain waves queued behind them
    // small-batch plan: runs per loop piece (front-loaded: the LAST piece's inversion batch and expansion are the
    // exposed tail of the call, so it is the shortest), 0-terminated; empty = equal pieces.  And the split of the last
    // piece's inversion batch (latency matters there; the earlier ones only need throughput: fewer inversions).
    int small_takes[MAX_PIECES + 1] = {0};
    int binv_split_log2_last = 3;
    // the fixed-base chain's batch: 67 ops that all keep their affine form, the longest walk, and its expansion is the largest
    // single launch of the call -- eight sub-ranges: 1.89 against 1.95 ms at 2^13, level at 2^14 (profiles/r03_fixed_base_batch_split.txt)
    int binv_split_log2_fixed = 3;
    // small-batch plan: which of the two phase-B streams takes the FIRST batch after the window table's (the fixed-base
    // chain's).  1: the fixed-base chain's own stream -- the table's batch occupies the other one until ~0.7 ms, and the
    // fixed-base batch (67 ops that all keep their affine form: the longest) queued behind it used to hold up the second
    // loop piece's batch in turn.  0: the round-2 order.
    bool quad_b_first_on_fixed = true;
    bool quad_few_waits = true;   // P2E_QUAD_FEW_WAITS=0: one wait per earlier piece, as before
    unsigned expand_lds_small = 54000;   // (160 000 -- one expansion workgroup per CU -- while the chains were the bottleneck; with lazy-limb chains 54 000 is 3-4 % faster at 2^13, profiles/r03_quad_plan_lazy_limbs_sweeps.txt)
    unsigned expand_lds = 0;   // the same knob for the large-batch plan
    // p2e_ecdsa_public_key_batch / p2e_ecdsa_sign_batch with P2E_SIGN_PLAN_AUTO: four lanes per scalar up to this batch
    // size, one lane per scalar above it (MEASUREMENTS.md, "Batch key derivation and signing")
    size_t sign_quad_max_n = 65536;   // (no environment variable)
};

// One environment variable each.  RANGED: atoi, a value outside [lo, hi] is ignored (not clamped); FLAG: atoi != 0;
// SIZE: strtoull, unchecked, `size2` takes the same value; UINT: strtoul, unchecked (p2e_ctx_create clamps the two LDS
// sizes to the device's limit afterwards).
struct Knob {
    const char* name;
    int Tuning::*ranged;
    int lo, hi;
    bool Tuning::*flag;
    size_t Tuning::*size, Tuning::*size2;
    unsigned Tuning::*uint;
};
// a row is only ever made by one of these four, so exactly one of its member pointers is set and it has the field's type
constexpr Knob knob_ranged(const char* name, int Tuning::*f, int lo, int hi) {
    return {name, f, lo, hi, nullptr, nullptr, nullptr, nullptr};
}
constexpr Knob knob_flag(const char* name, bool Tuning::*f) { return {name, nullptr, 0, 0, f, nullptr, nullptr, nullptr}; }
constexpr Knob knob_size(const char* name, size_t Tuning::*f, size_t Tuning::*f2 = nullptr) {
    return {name, nullptr, 0, 0, nullptr, f, f2, nullptr};
}
constexpr Knob knob_uint(const char* name, unsigned Tuning::*f) { return {name, nullptr, 0, 0, nullptr, nullptr, nullptr, f}; }
inline constexpr Knob KNOBS[] = {
    knob_ranged("P2E_RUN_ITERS", &Tuning::run_iters, 0, Tuning::MAX_RUN_ITERS),
    knob_ranged("P2E_RUN_ITERS_MID", &Tuning::run_iters_mid, 0, Tuning::MAX_RUN_ITERS),
    knob_ranged("P2E_RUN_ITERS_SMALL", &Tuning::run_iters_small, 0, Tuning::MAX_RUN_ITERS),
    knob_flag("P2E_FB_RUN", &Tuning::fb_run),
    knob_size("P2E_RUNS_MIN_N", &Tuning::runs_min_n),
    knob_size("P2E_QUAD_MAX_N", &Tuning::quad_max_n, &Tuning::cp_quad_max_n),
    knob_size("P2E_BINV_ALT_MAX_N", &Tuning::binv_alt_max_n),
    knob_size("P2E_CP_RUNS_MIN_N", &Tuning::cp_runs_min_n),
    knob_ranged("P2E_MSM_PIECES", &Tuning::msm_pieces, 1, Tuning::MAX_PIECES),
    knob_ranged("P2E_MSM_PIECES_MID", &Tuning::msm_pieces_mid, 1, Tuning::MAX_PIECES),
    knob_ranged("P2E_MSM_PIECES_SMALL", &Tuning::msm_pieces_small, 1, Tuning::MAX_PIECES),
    knob_ranged("P2E_FIXED_PIECES", &Tuning::fixed_pieces, 1, Tuning::MAX_PIECES),
    knob_ranged("P2E_FIXED_PIECES_SMALL", &Tuning::fixed_pieces_small, 1, Tuning::MAX_PIECES),
    knob_ranged("P2E_BINV_MID_SPLIT_LOG2", &Tuning::binv_mid_split_log2, 0, 3),
    knob_ranged("P2E_BINV_SPLIT_LOG2", &Tuning::binv_split_log2, 0, 4),
    knob_ranged("P2E_BINV_SPLIT_LOG2_LAST", &Tuning::binv_split_log2_last, 0, 4),
    knob_ranged("P2E_BINV_SPLIT_LOG2_FIXED", &Tuning::binv_split_log2_fixed, 0, 4),
    knob_flag("P2E_QUAD_B_FIRST_ON_FIXED", &Tuning::quad_b_first_on_fixed),
    knob_flag("P2E_QUAD_FEW_WAITS", &Tuning::quad_few_waits),
    knob_uint("P2E_EXPAND_LDS_SMALL", &Tuning::expand_lds_small),
    knob_uint("P2E_EXPAND_LDS", &Tuning::expand_lds),
};

// env: const char* (const char* name), null where the variable is not set (getenv)
template <class Env>
inline void read_tuning(Tuning& t, Env env) {
    for (const Knob& k : KNOBS) {
        const char* v = env(k.name);
        if (!v) continue;
        if (k.ranged) {
            const int x = atoi(v);
            if (x >= k.lo && x <= k.hi) t.*k.ranged = x;
        } else if (k.flag) {
            t.*k.flag = atoi(v) != 0;
        } else if (k.size) {
            t.*k.size = (size_t)strtoull(v, nullptr, 10);
            if (k.size2) t.*k.size2 = t.*k.size;
        } else {
            t.*k.uint = (unsigned)strtoul(v, nullptr, 10);
        }
    }
    if (const char* v = env("P2E_SMALL_TAKES")) {   // e.g. "24,20,16,9,4": loop iterations per piece (op-by-op expansion: any cut)
        int k = 0;
        for (const char* p = v; *p && k < Tuning::MAX_PIECES; k++) {
            t.small_takes[k] = atoi(p);
            while (*p && *p != ',') p++;
            if (*p == ',') p++;
        }
        t.small_takes[k] = 0;
    }
}

// P2E_NARROW_STORES alone, for the streaming passes (aux, gate, constraint-block), which have no launch plan
inline bool narrow_stores_forced() { return getenv("P2E_NARROW_STORES") != nullptr; }

// The per-call switches.  The five flags are set by the variable's PRESENCE, whatever its value.
struct CallSwitches {
    bool narrow_stores = false;   // 16-byte (paired) column stores switched off: every emitting launch takes its one-signature-per-lane form
    bool cp_no_runs = false, cp_no_quad = false, cp_no_alt_b = false, cp_fb_serial = false;
    bool cp_piece_ops_quad_set = false, cp_tail_ops_quad_set = false;   // atoi of the value; choose_curve ignores one out of range
    int cp_piece_ops_quad = 0, cp_tail_ops_quad = 0;
};
template <class Env>
inline CallSwitches read_call_switches(Env env) {
    CallSwitches s;
    s.narrow_stores = env("P2E_NARROW_STORES") != nullptr;
    s.cp_no_runs = env("P2E_CP_NO_RUNS") != nullptr;
    s.cp_no_quad = env("P2E_CP_NO_QUAD") != nullptr;
    s.cp_no_alt_b = env("P2E_CP_NO_ALT_B") != nullptr;
    s.cp_fb_serial = env("P2E_CP_FB_SERIAL") != nullptr;
    if (const char* v = env("P2E_CP_PIECE_OPS_QUAD")) {
        s.cp_piece_ops_quad_set = true;
        s.cp_piece_ops_quad = atoi(v);
    }
    if (const char* v = env("P2E_CP_TAIL_OPS_QUAD")) {
        s.cp_tail_ops_quad_set = true;
        s.cp_tail_ops_quad = atoi(v);
    }
    return s;
}

}  // namespace p2e

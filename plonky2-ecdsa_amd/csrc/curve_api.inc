// Curve programs (curves.hpp, curve_program.hpp): kernels, launcher and C ABI.  Included at the end of p2e_hip.hip
// (same translation unit: it shares the context, the staging helper and the finalisation kernel).
//
// Launch plan (launch_plan.hpp choose_curve / build_curve): the op list is cut into pieces; piece k runs  chain (phase A, chain stream)  ->  batch inversion
// (phase B, second stream)  ->  expansion (phase C, caller's stream), so that the HBM-bound expansion of finished pieces
// runs underneath the chains and inversions of later ones, exactly as in the built-in programs.  The per-signature
// window table is its own piece, inverted on the chain stream itself; every later piece reads it in affine form (mixed
// additions).  Batches of >= cp_runs_min_n (49 152): the windowed loop in pieces of plan::CP_RUN_OPS ops expanded as runs
// (body_expand_run<.., 4>, the MSM program's 2-doubling loop body_expand_run<.., 2>), the fixed-base windows of the
// verifier (on a second chain stream) and of the fixed-base program as one run per signature (body_expand_fb_run);
// smaller batches: pieces of <= plan::CP_PIECE_OPS ops expanded op by op.

#if P2E_HAS(2) || P2E_HAS(3)
template <class CV, int MODE>
__global__ __launch_bounds__(BS) void kc_scalar(Program G, Buffers B, size_t first) {
    size_t i = lane_sig<(MODE & 1) != 0>(first);
    if ((MODE & 1) || i < B.n) body_cscalar<CV, typename EmitOf<MODE>::type>(G, B, i);
}
template <class CV>
__global__ __launch_bounds__(BS) void kc_chains(Program G, Buffers B, int lo, int hi, int table_affine) {
    __builtin_amdgcn_s_setprio(3);
    size_t i = (size_t)blockIdx.x * BS + threadIdx.x;
    if (i < B.n) body_chain_range<CV, true>(G, B, i, lo, hi, table_affine != 0, false);
}
// small batches: four lanes per signature (quad.hpp body_chain_range_quad_cv), the inversion batch cut into sub-ranges
template <class CV>
__global__ __launch_bounds__(BS) void kc_chains_quad(Program G, Buffers B, int lo, int hi, int table_affine) {
    __builtin_amdgcn_s_setprio(3);
    const size_t g = (size_t)blockIdx.x * BS + threadIdx.x;
    const size_t i = g >> 2;
    if (i < B.n) body_chain_range_quad_cv<CV>(G, B, i, (int)(g & 3), lo, hi, table_affine != 0);
}
template <class CV>
__global__ __launch_bounds__(BS) void kc_batch_inv_split(Program G, Buffers B, int lo, int hi, int split_log2) {
    const size_t g = (size_t)blockIdx.x * BS + threadIdx.x;
    const size_t i = g >> split_log2;
    if (i < B.n) body_batch_inv_split<CV>(G, B, i, lo, hi, true, (int)(g & ((1u << split_log2) - 1)), 1 << split_log2);
}
// verdict only (p2e_p256_verify_batch): r == x on the final add's Jacobian result
template <class CV>
__global__ __launch_bounds__(BS) void kc_verify_check(Program G, Buffers B) {
    size_t i = (size_t)blockIdx.x * BS + threadIdx.x;
    if (i < B.n) body_verify_check<CV>(G, B, i, G.num_ops - 1);
}
// runs of the windowed loop (4 doublings + conditional add per iteration), as k_expand_runs
template <class CV, int MODE>
__global__ __launch_bounds__(BS) void kc_expand_runs(Program G, Buffers B, int it_first, int run_iters, int it_end, size_t first) {
    size_t i = lane_sig<(MODE & 1) != 0>(first);
    int it0 = it_first + (int)blockIdx.y * run_iters;
    int it1 = it0 + run_iters < it_end ? it0 + run_iters : it_end;
    if ((MODE & 1) || i < B.n) body_expand_run<typename EmitOf<MODE>::type, CV, 4>(G, B, i, it0, it1);
}
// ... and of the MSM program's digit loop (2 doublings + conditional add per iteration)
template <class CV, int MODE>
__global__ __launch_bounds__(BS) void kc_expand_runs2(Program G, Buffers B, int it_first, int run_iters, int it_end, size_t first) {
    size_t i = lane_sig<(MODE & 1) != 0>(first);
    int it0 = it_first + (int)blockIdx.y * run_iters;
    int it1 = it0 + run_iters < it_end ? it0 + run_iters : it_end;
    if ((MODE & 1) || i < B.n) body_expand_run<typename EmitOf<MODE>::type, CV, 2>(G, B, i, it0, it1);
}
template <class CV, int MODE>
__global__ __launch_bounds__(BS) void kc_expand_fb_run(Program G, Buffers B, int t_after, size_t first) {
    size_t i = lane_sig<(MODE & 1) != 0>(first);
    if ((MODE & 1) || i < B.n) body_expand_fb_run<typename EmitOf<MODE>::type, CV>(G, B, i, t_after);
}
template <class CV>
__global__ __launch_bounds__(BS) void kc_batch_inv(Program G, Buffers B, int lo, int hi) {
    size_t i = (size_t)blockIdx.x * BS + threadIdx.x;
    if (i < B.n) body_batch_inv<CV>(G, B, i, lo, hi, true);
}
template <class CV, int MODE>
__global__ __launch_bounds__(BS) void kc_expand(Program G, Buffers B, int lo, size_t first) {
    size_t i = lane_sig<(MODE & 1) != 0>(first);
    if ((MODE & 1) || i < B.n) body_expand<typename EmitOf<MODE>::type, CV>(G, B, i, lo + (int)blockIdx.y);
}

#endif   // P2E_HAS(2) || P2E_HAS(3)
#if P2E_HAS(0)
// built-in-generator / constraint-block passes of a curve program (aux.hpp body_aux_cv, ux.hpp body_ux_cv)
template <int MODE>
__global__ __launch_bounds__(BS) void kc_aux(AuxArgs A, size_t first) {
    size_t i = lane_sig<(MODE & 1) != 0>(first);
    if ((MODE & 1) || i < A.n) body_aux_cv<typename AuxEmitOf<MODE>::type>(A, (int)blockIdx.y, i);
}
template <int MODE>
__global__ __launch_bounds__(BS) void kc_ux(UxArgs A, size_t first) {
    size_t i = lane_sig<(MODE & 1) != 0>(first);
    if ((MODE & 1) || i < A.n) body_ux_cv<typename AuxEmitOf<MODE>::type>(A, (int)blockIdx.y, i);
}
template <int MODE>
__global__ __launch_bounds__(BS) void kc_ux_compact(UxArgs A, size_t first) {
    size_t i = lane_sig<(MODE & 1) != 0>(first);
    if ((MODE & 1) || i < A.n) body_ux_cv<typename AuxEmitOf<MODE>::type, true>(A, (int)blockIdx.y, i);
}

#endif   // P2E_HAS(0)

struct p2e_curve_program {
    host::CurveProgramHost H;
    // compact container (include/p2e.h p2e_curve_program_compact_layout): per column its slot in the u32 narrow matrix
    // or COMPACT_WIDE | slot in the u64 wide matrix (the check_sum / carry columns of the mul generators), in
    // registration order; wide_before[c] = wide columns before column c (the emitters' second cursor)
    host::CompactLayout compact;
    int device = 0;
    DeviceArray<OpDesc> d_ops;        // every op expanded on its own
    DeviceArray<OpDesc> d_ops_runs;   // with the run marks (F_NO_AFFINE) of CP_RUN_ITERS and of the fixed-base windows
    DeviceArray<Aff> d_cpts, d_fbtab;
    PassTables tab;
    DeviceArray<U256> d_constv;   // constants by source id: points at 2c / 2c + 1, scalar constants from AUX_GCONST_BASE
};
using plan::cp_run_iters;   // loop iterations per expansion run: the run marks of d_ops_runs (launch_plan.hpp)

// the pipeline of one curve: defined (and explicitly instantiated) in parts 2 and 3
template <class CV>
long run_curve_program(p2e_ctx* c, const p2e_curve_program* P, const uint8_t* msg, const uint8_t* r, const uint8_t* s,
                       const uint8_t* pkx, const uint8_t* pky, uint64_t* cols, size_t n, size_t ld, uint8_t* err,
                       uint8_t* valid, bool verify_only, uint32_t* narrow, size_t ldn, uint64_t* wide, size_t ldw,
                       const uint8_t* qx, const uint8_t* qy);

#if P2E_HAS(0)
// does any aux item (or the random-access table it selects from) read the MSM program's q (INPUT_QX / INPUT_QY)?
static bool aux_reads_q(const host::ScheduleBuilder& sb) {
    auto is_q = [](u32 src) {
        return src != AUX_SRC_NONE && (src & AUX_SRC_KIND_MASK) == AUX_SRC_INPUT && ((src & 7u) == INPUT_QX || (src & 7u) == INPUT_QY);
    };
    for (const AuxItem& it : sb.aux_items)
        for (u32 src : {it.a, it.c, it.sumx, it.sumy, it.p1x, it.p1y})
            if (is_q(src)) return true;
    for (int k = 0; k < 16; k++)
        if (is_q(sb.aux_tab.tabx[k]) || is_q(sb.aux_tab.taby[k])) return true;
    return false;
}
extern "C" int p2e_curve_program_create(p2e_ctx* c, int kind, int curve, const uint8_t* blind_x32, const uint8_t* blind_y32,
                                        p2e_curve_program** out) {
    // the MSM program takes no point (its constants do not depend on the build); every other kind takes one: the
    // rand() blinding point, or the fixed-base program's base
    const bool takes_point = kind != CP_MSM;
    if (!c || !out || (takes_point && (!blind_x32 || !blind_y32))) return P2E_E_INVALID;
    Aff blind{};
    if (takes_point) {
        const char* what = kind == CP_FIXED_BASE_MUL ? "fixed-base point" : "blinding point";
        memcpy(blind.x.w, blind_x32, 32);
        memcpy(blind.y.w, blind_y32, 32);
        const bool ge = curve == 1 ? (geq_mod<ModP256>(blind.x.w) || geq_mod<ModP256>(blind.y.w)) : (geq_mod<ModP>(blind.x.w) || geq_mod<ModP>(blind.y.w));
        if (ge) {
            set_error(std::string(what) + " coordinate is not a canonical field element");
            return P2E_E_INVALID;
        }
        // The reference always draws rand() * G here (gadgets/curve_windowed_mul.rs:57, gadgets/curve.rs:253): a point ON the
        // curve.  Anything else (a typo, a point of the other curve) would build a program whose witnesses match no circuit
        // the reference can build, and would only show as bulk error flags later.  The same holds for a fixed base
        // (an AffinePoint<C> of the program's curve, gadgets/curve_fixed_base.rs:18).
        const bool on_curve = curve == 1 ? host::aff_on_curve_cv<P256>(blind) : host::aff_on_curve_cv<Secp256k1>(blind);
        if ((curve == 0 || curve == 1) && !on_curve) {
            set_error(std::string(what) + " is not on the curve (y^2 != x^3 + a x + b of the program's curve)");
            return P2E_E_INVALID;
        }
    }
    DeviceGuard guard(c->device);
    std::unique_ptr<p2e_curve_program> P(new p2e_curve_program());   // a failure below frees what was uploaded before it
    if (!host::make_curve_program(P->H, kind, curve, blind)) {
        set_error("unknown curve program (kind 1..5, curve 0..1; the verifier program is P-256 only)");
        return P2E_E_INVALID;
    }
    const host::ScheduleBuilder& sb = P->H.sb;
    // the aux pass (p2e_curve_program_aux_witness_batch) has no argument for the MSM program's q: no aux item may read it
    if (aux_reads_q(sb)) {
        set_error("curve program: an aux item reads q (input slot 5 / 6), which the aux pass has no argument for");
        return P2E_E_INVALID;
    }
    {   // compact container layout (as host_program of the built-in programs), and the host-only check of what the
        // compact-source ux pass walks: before anything is allocated on the device
        P->compact = host::compact_layout(sb.gens, (size_t)sb.prog.num_cols);
        std::string why;
        if (!host::ux_items_compact_ok(sb.ux_items, P->compact.map, why)) {
            set_error(why);
            return P2E_E_INVALID;
        }
    }
    P->device = c->device;
    HIP_TRY(P->d_ops.upload(sb.ops));
    if (sb.prog.msm_loop_iters > 0 || kind == CP_FIXED_BASE_MUL)
        HIP_TRY(P->d_ops_runs.upload(sb.ops_with_runs(cp_run_iters(sb.prog))));
    HIP_TRY(P->d_cpts.upload(sb.gpts));
    HIP_TRY(P->d_fbtab.upload(sb.gfbtab));
    HIP_TRY(P->tab.upload(sb, P->compact, false));
    {
        std::vector<U256> cv(AUX_GCONST_BASE + sb.gvals.size(), u256_zero());
        for (size_t k = 0; k < sb.gpts.size(); k++) {
            cv[2 * k] = sb.gpts[k].x;
            cv[2 * k + 1] = sb.gpts[k].y;
        }
        for (size_t j = 0; j < sb.gvals.size(); j++) cv[AUX_GCONST_BASE + j] = sb.gvals[j];
        HIP_TRY(P->d_constv.upload(cv));
    }
    *out = P.release();
    return 0;
}
extern "C" void p2e_curve_program_destroy(p2e_ctx* c, p2e_curve_program* P) {
    if (!P) return;
    DeviceGuard guard(P->device);
    if (c && c->stream) (void)hipStreamSynchronize(c->stream);
    delete P;
}
extern "C" long p2e_curve_program_num_cols(const p2e_curve_program* P) { return P ? P->H.sb.prog.num_cols : P2E_E_INVALID; }
extern "C" long p2e_curve_program_num_aux_cols(const p2e_curve_program* P) { return P ? (long)P->H.sb.aux_tab.num_aux_cols : P2E_E_INVALID; }
extern "C" long p2e_curve_program_num_gate_cols(const p2e_curve_program* P) { return P ? (long)P->H.sb.num_gate_cols : P2E_E_INVALID; }
extern "C" long p2e_curve_program_num_ux_cols(const p2e_curve_program* P) { return P ? (long)P->H.sb.num_ux_cols : P2E_E_INVALID; }
extern "C" long p2e_curve_program_ux_describe(const p2e_curve_program* P, p2e_ux_desc* out, size_t cap) {
    if (!P) return P2E_E_INVALID;
    const auto& sb = P->H.sb;
    for (size_t k = 0; out && k < sb.ux_first.size() && k < cap; k++) {
        out[k].first_col = sb.ux_first[k];
        out[k].num_cols = sb.ux_count[k];
    }
    return (long)sb.ux_first.size();
}
extern "C" size_t p2e_curve_program_scratch_bytes(const p2e_curve_program* P, size_t n) {
    return P ? scratch_layout(P->H.sb.prog, n).total : 0;
}
static void fill_gen_desc(const host::GenOp& g, p2e_gen_desc& d) {
    d.kind = g.kind;
    d.field = g.field;
    d.first_col = g.col;
    d.num_cols = g.ncols;
    memset(d.label, 0, sizeof d.label);
    strncpy(d.label, g.label.c_str(), sizeof d.label - 1);
}
extern "C" long p2e_curve_program_describe(const p2e_curve_program* P, p2e_gen_desc* out, size_t cap) {
    if (!P) return P2E_E_INVALID;
    const auto& gens = P->H.sb.gens;
    for (size_t k = 0; out && k < gens.size() && k < cap; k++) fill_gen_desc(gens[k], out[k]);
    return (long)gens.size();
}
extern "C" long p2e_curve_program_wiring(const p2e_curve_program* P, p2e_gen_wiring* out, size_t cap) {
    if (!P) return P2E_E_INVALID;
    const auto& gens = P->H.sb.gens;
    for (size_t k = 0; out && k < gens.size() && k < cap; k++) {
        out[k].num_operands = (uint32_t)gens[k].nops;
        out[k].range_check = gens[k].range_check ? 1u : 0u;
        for (int j = 0; j < 4; j++) {
            out[k].src[j] = gens[k].src[j];
            out[k].num_limbs[j] = gens[k].nl[j];
        }
    }
    return (long)gens.size();
}
extern "C" long p2e_curve_program_aux_describe(const p2e_curve_program* P, p2e_aux_desc* out, size_t cap) {
    if (!P) return P2E_E_INVALID;
    const auto& ag = P->H.sb.aux_gens;
    for (size_t k = 0; out && k < ag.size() && k < cap; k++) {
        out[k].kind = ag[k].kind;
        out[k].first_col = ag[k].col;
        out[k].num_cols = ag[k].ncols;
        memset(out[k].label, 0, sizeof out[k].label);
        strncpy(out[k].label, ag[k].label.c_str(), sizeof out[k].label - 1);
    }
    return (long)ag.size();
}
extern "C" int p2e_curve_program_const(const p2e_curve_program* P, uint32_t id, uint8_t out32[32]) {
    if (!P || !out32) return P2E_E_INVALID;
    const host::ScheduleBuilder& sb = P->H.sb;
    id &= 0xFFFFu;
    if (id >= AUX_GCONST_BASE ? id - AUX_GCONST_BASE >= sb.gvals.size() : (id >> 1) >= sb.gpts.size()) return P2E_E_INVALID;
    const U256 v = sb.cval(id);
    memcpy(out32, v.w, 32);
    return 0;
}

#endif   // P2E_HAS(0)

#if P2E_HAS(2) || P2E_HAS(3)
template <class CV>
struct CurveKernels {
    static constexpr bool has_rows = false;   // no curve plan walks a table as rows
    static int loop_stride(const Program& G) { return G.loop_dbls + 1; }   // the loop's doublings + the conditional add
    template <int MODE>
    static void scalar(dim3 g, hipStream_t st, const Program& G, const Buffers& B, size_t first) {
        hipLaunchKernelGGL((kc_scalar<CV, MODE>), g, dim3(BS), 0, st, G, B, first);
    }
    // (the curve programs' chains never continue a prefix and their inversion batches always have phase A's)
    static void chain_lane(dim3 g, hipStream_t st, const Program& G, const Buffers& B, int lo, int hi, int table_affine, int) {
        hipLaunchKernelGGL((kc_chains<CV>), g, dim3(BS), 0, st, G, B, lo, hi, table_affine);
    }
    static void chain_quad(dim3 g, hipStream_t st, const Program& G, const Buffers& B, int lo, int hi, int table_affine, int) {
        hipLaunchKernelGGL((kc_chains_quad<CV>), g, dim3(BS), 0, st, G, B, lo, hi, table_affine);
    }
    static void binv(dim3 g, hipStream_t st, const Program& G, const Buffers& B, int lo, int hi, int) {
        hipLaunchKernelGGL((kc_batch_inv<CV>), g, dim3(BS), 0, st, G, B, lo, hi);
    }
    static void binv_split(dim3 g, hipStream_t st, const Program& G, const Buffers& B, int lo, int hi, int, int split_log2) {
        hipLaunchKernelGGL((kc_batch_inv_split<CV>), g, dim3(BS), 0, st, G, B, lo, hi, split_log2);
    }
    template <int MODE>
    static void expand(dim3 g, unsigned lds, hipStream_t st, const Program& G, const Buffers& B, int lo, size_t first) {
        hipLaunchKernelGGL((kc_expand<CV, MODE>), g, dim3(BS), lds, st, G, B, lo, first);
    }
    template <int MODE>
    static void expand_runs(dim3 g, unsigned lds, hipStream_t st, const Program& G, const Buffers& B, int it0, int run_iters, int it1,
                            size_t first) {
        if (G.loop_dbls == 2)
            hipLaunchKernelGGL((kc_expand_runs2<CV, MODE>), g, dim3(BS), lds, st, G, B, it0, run_iters, it1, first);
        else
            hipLaunchKernelGGL((kc_expand_runs<CV, MODE>), g, dim3(BS), lds, st, G, B, it0, run_iters, it1, first);
    }
    template <int MODE>
    static void expand_fb_run(dim3 g, unsigned lds, hipStream_t st, const Program& G, const Buffers& B, int t_after, size_t first) {
        hipLaunchKernelGGL((kc_expand_fb_run<CV, MODE>), g, dim3(BS), lds, st, G, B, t_after, first);
    }
};

// Stage, bind, build the plan, issue (as run_program).
template <class CV>
long run_curve_program(p2e_ctx* c, const p2e_curve_program* P, const uint8_t* msg, const uint8_t* r, const uint8_t* s,
                       const uint8_t* pkx, const uint8_t* pky, uint64_t* cols, size_t n, size_t ld, uint8_t* err,
                       uint8_t* valid, bool verify_only, uint32_t* narrow, size_t ldn, uint64_t* wide, size_t ldw,
                       const uint8_t* qx, const uint8_t* qy) {
    const CallSwitches sw = read_call_switches(getenv);
    const bool compact = cols == nullptr && !verify_only;
    const Program& G = P->H.sb.prog;
    Staged S(c);
    FusedIO io{{msg, r, s, pkx, pky, qx, qy}, cols, ld, narrow, ldn, wide, ldw, err, valid};
    Buffers B;
    if (long rc = stage_fused(c, S, G, P->compact, P->tab.wide_before.get(), compact, verify_only, n, io, B)) return S.done(rc);
    B.cpts = P->d_cpts.get();
    B.fbtab = P->d_fbtab.get();
    B.ops = P->d_ops.get();
    ZERO_COUNTER(c);
    c->seg_blocks.clear();
    if (verify_only) {
        // the circuit's verdict alone (the P-256 counterpart of p2e_ecdsa_verify_batch): scalar phase without emission,
        // the fixed-base chain beside the windowed chain in Jacobian coordinates (no batch inversion, no expansion: the
        // window table stays Jacobian), the final add, r == x on its Jacobian result
        const unsigned gx = (unsigned)((n + BS - 1) / BS);
        const int fb_end = G.fb_begin + G.fb_windows + 1;
        hipLaunchKernelGGL((kc_scalar<CV, 4>), dim3(gx), dim3(BS), 0, c->stream, G, B, (size_t)0);
        HIP_TRY(hipEventRecord(c->ev_fork, c->stream));
        HIP_TRY(hipStreamWaitEvent(c->st_fixed, c->ev_fork, 0));
        hipLaunchKernelGGL((kc_chains<CV>), dim3(gx), dim3(BS), 0, c->st_fixed, G, B, G.fb_begin, fb_end, 0);
        HIP_TRY(hipEventRecord(c->ev_fixed, c->st_fixed));
        hipLaunchKernelGGL((kc_chains<CV>), dim3(gx), dim3(BS), 0, c->stream, G, B, fb_end, G.num_ops - 1, 0);
        HIP_TRY(hipStreamWaitEvent(c->stream, c->ev_fixed, 0));
        hipLaunchKernelGGL((kc_chains<CV>), dim3(gx), dim3(BS), 0, c->stream, G, B, G.num_ops - 1, G.num_ops, 0);
        hipLaunchKernelGGL((kc_verify_check<CV>), dim3(gx), dim3(BS), 0, c->stream, G, B);
        hipLaunchKernelGGL(k_finalize, dim3(gx), dim3(BS), 0, c->stream, B.err, B.valid, io.err, io.valid, n, c->d_counter);
        c->have_phases = false;
        return S.done(finish_call(c));
    }
    const plan::CurveParams cp = plan::choose_curve(G, c->tune, n, P->d_ops_runs.get() != nullptr, stream_layout(c),
                                                    (c->flags & P2E_CTX_PHASE_TIMING) != 0, sw);
    plan::Plan pl;
    if (!plan::build_curve(G, cp, pl)) {
        set_plan_error(pl.error, "curve program", cp.quad);
        return S.done(P2E_E_INVALID);
    }
    if (pl.ops == plan::OPS_RUNS) B.ops = P->d_ops_runs.get();
    if (long rc = issue_plan<CurveKernels<CV>>(c, pl, G, B, P->H.sb.ops, compact, !sw.narrow_stores && io.paired_stores_ok(compact), io.err,
                                                io.valid))
        return rc;
    return S.done(finish_call(c));
}

#if P2E_PART < 0 || P2E_PART == 2
template long run_curve_program<Secp256k1>(p2e_ctx*, const p2e_curve_program*, const uint8_t*, const uint8_t*, const uint8_t*,
                                           const uint8_t*, const uint8_t*, uint64_t*, size_t, size_t, uint8_t*, uint8_t*, bool,
                                           uint32_t*, size_t, uint64_t*, size_t, const uint8_t*, const uint8_t*);
#endif
#if P2E_PART < 0 || P2E_PART == 3
template long run_curve_program<P256>(p2e_ctx*, const p2e_curve_program*, const uint8_t*, const uint8_t*, const uint8_t*,
                                      const uint8_t*, const uint8_t*, uint64_t*, size_t, size_t, uint8_t*, uint8_t*, bool,
                                      uint32_t*, size_t, uint64_t*, size_t, const uint8_t*, const uint8_t*);
#endif
#endif   // P2E_HAS(2) || P2E_HAS(3)

#if P2E_HAS(0)
static long curve_dispatch(p2e_ctx* c, const p2e_curve_program* P, const uint8_t* msg, const uint8_t* r, const uint8_t* s,
                           const uint8_t* pkx, const uint8_t* pky, uint64_t* cols, size_t n, size_t ld, uint8_t* err, uint8_t* valid,
                           bool verify_only = false, uint32_t* narrow = nullptr, size_t ldn = 0, uint64_t* wide = nullptr, size_t ldw = 0,
                           const uint8_t* qx = nullptr, const uint8_t* qy = nullptr) {
    if (P->device != c->device) {
        set_error("curve program was created on another device");
        return P2E_E_INVALID;
    }
    if (P->H.curve == 1)
        return run_curve_program<P256>(c, P, msg, r, s, pkx, pky, cols, n, ld, err, valid, verify_only, narrow, ldn, wide, ldw, qx, qy);
    return run_curve_program<Secp256k1>(c, P, msg, r, s, pkx, pky, cols, n, ld, err, valid, verify_only, narrow, ldn, wide, ldw, qx, qy);
}
// the fills of a point-and-scalar program: the windowed and scalar multiplications take (px, py, k), the fixed-base
// program k alone (px32 = py32 = NULL: its base is a circuit constant)
static bool curve_mul_args_ok(const p2e_curve_program* P, const uint8_t* px32, const uint8_t* py32) {
    if (P->H.kind != CP_WINDOWED && P->H.kind != CP_SCALAR_MUL && P->H.kind != CP_FIXED_BASE_MUL) {
        set_error("not a scalar-multiplication program");
        return false;
    }
    if (P->H.kind != CP_FIXED_BASE_MUL && (!px32 || !py32)) {
        set_error("this program multiplies the caller's point: px32 / py32 must not be NULL");
        return false;
    }
    return true;
}
static bool curve_msm_args_ok(const p2e_curve_program* P) {
    if (P->H.kind != CP_MSM) {
        set_error("not an MSM program (p2e_curve_msm_witness_batch needs a program of kind P2E_CP_MSM)");
        return false;
    }
    return true;
}
// what the MSM program's constraint-block pass reads, in either container: p, q and both scalars (n in msg32, m in r32)
static bool curve_msm_ux_inputs_ok(const uint8_t* px, const uint8_t* py, const uint8_t* qx, const uint8_t* qy, const uint8_t* n32,
                                   const uint8_t* m32) {
    if (!px || !py || !qx || !qy || !n32 || !m32) {
        set_error("the MSM program's constraint-block pass reads p, q, n and m: none of their pointers may be NULL");
        return false;
    }
    return true;
}
// the verifier circuit's verdict alone: valid[i] = curve_assert_valid's connect and r == x both hold (and no error
// flag), no witness written -- a pre-filter for invalid signatures; native counterpart curve/ecdsa.rs:42-62
// verify_message on P-256, with exactly the circuit's verdict
extern "C" long p2e_p256_verify_batch(p2e_ctx* c, const p2e_curve_program* prog, const uint8_t* msg32, const uint8_t* r32,
                                      const uint8_t* s32, const uint8_t* pkx32, const uint8_t* pky32, size_t n, uint8_t* err,
                                      uint8_t* valid) {
    // (staging is curve_dispatch's own, as for every curve program)
    const Args args = {ARG_OPAQUE(prog),         ARG_SHARED(msg32, 32, n), ARG_SHARED(r32, 32, n), ARG_SHARED(s32, 32, n),
                       ARG_SHARED(pkx32, 32, n), ARG_SHARED(pky32, 32, n), ARG_OUT(err, 1, n),     ARG_OUT(valid, 1, n)};
    if (missing(args) || bad_overlap(n, args) || bad_ctx(c)) return P2E_E_INVALID;
    if (prog->H.kind != CP_VERIFY) {
        set_error("not a verifier program");
        return P2E_E_INVALID;
    }
    if (n == 0) return 0;
    return curve_dispatch(c, prog, msg32, r32, s32, pkx32, pky32, nullptr, n, n, err, valid, true);
}
// curve_scalar_mul_windowed(p, k) / curve_scalar_mul(p, k) witnesses of a batch of (point, scalar) pairs
extern "C" long p2e_curve_mul_witness_batch(p2e_ctx* c, const p2e_curve_program* P, const uint8_t* px32, const uint8_t* py32,
                                            const uint8_t* k32, uint64_t* cols, size_t n, size_t ld, uint8_t* err, uint8_t* valid) {
    if (bad_common(c, n, ld) || !P || !k32 || !cols || !err || !curve_mul_args_ok(P, px32, py32)) return P2E_E_INVALID;
    if (n == 0) return 0;
    if (P->H.kind == CP_FIXED_BASE_MUL) px32 = py32 = nullptr;
    return curve_dispatch(c, P, k32, k32, k32, px32, py32, cols, n, ld, err, valid);
}
// curve_msm_circuit(p, q, n, m) witnesses of a batch (gadgets/curve_msm.rs:21-79)
extern "C" long p2e_curve_msm_witness_batch(p2e_ctx* c, const p2e_curve_program* P, const uint8_t* px32, const uint8_t* py32,
                                            const uint8_t* qx32, const uint8_t* qy32, const uint8_t* n32, const uint8_t* m32,
                                            uint64_t* cols, size_t n, size_t ld, uint8_t* err, uint8_t* valid) {
    if (bad_common(c, n, ld) || !P || !px32 || !py32 || !qx32 || !qy32 || !n32 || !m32 || !cols || !err || !curve_msm_args_ok(P))
        return P2E_E_INVALID;
    if (n == 0) return 0;
    return curve_dispatch(c, P, n32, m32, nullptr, px32, py32, cols, n, ld, err, valid, false, nullptr, 0, nullptr, 0, qx32, qy32);
}
extern "C" long p2e_curve_msm_witness_compact_batch(p2e_ctx* c, const p2e_curve_program* P, const uint8_t* px32, const uint8_t* py32,
                                                    const uint8_t* qx32, const uint8_t* qy32, const uint8_t* n32, const uint8_t* m32,
                                                    uint32_t* narrow, size_t ld_narrow, uint64_t* wide, size_t ld_wide, size_t n,
                                                    uint8_t* err, uint8_t* valid) {
    if (bad_common(c, n, ld_narrow) || ld_wide < n || !P || !px32 || !py32 || !qx32 || !qy32 || !n32 || !m32 || !narrow || !wide ||
        !err || !curve_msm_args_ok(P))
        return P2E_E_INVALID;
    if (n == 0) return 0;
    return curve_dispatch(c, P, n32, m32, nullptr, px32, py32, nullptr, n, 0, err, valid, false, narrow, ld_narrow, wide, ld_wide, qx32, qy32);
}
// verify_p256_message_circuit witnesses (gadgets/ecdsa.rs:55-78)
extern "C" long p2e_p256_verify_witness_batch(p2e_ctx* c, const p2e_curve_program* P, const uint8_t* msg32, const uint8_t* r32,
                                              const uint8_t* s32, const uint8_t* pkx32, const uint8_t* pky32, uint64_t* cols, size_t n,
                                              size_t ld, uint8_t* err, uint8_t* valid) {
    if (bad_common(c, n, ld) || !P || !msg32 || !r32 || !s32 || !pkx32 || !pky32 || !cols || !err) return P2E_E_INVALID;
    if (P->H.kind != CP_VERIFY) {
        set_error("not a verifier program");
        return P2E_E_INVALID;
    }
    if (n == 0) return 0;
    return curve_dispatch(c, P, msg32, r32, s32, pkx32, pky32, cols, n, ld, err, valid);
}
// the same two fills writing the compact container (include/p2e.h): u32 narrow[num_narrow][ld_narrow] for the columns
// that only ever hold values < 2^32, u64 wide[num_wide][ld_wide] for the check_sum / carry columns of the mul generators
extern "C" long p2e_curve_mul_witness_compact_batch(p2e_ctx* c, const p2e_curve_program* P, const uint8_t* px32, const uint8_t* py32,
                                                    const uint8_t* k32, uint32_t* narrow, size_t ld_narrow, uint64_t* wide, size_t ld_wide,
                                                    size_t n, uint8_t* err, uint8_t* valid) {
    if (bad_common(c, n, ld_narrow) || ld_wide < n || !P || !k32 || !narrow || !wide || !err || !curve_mul_args_ok(P, px32, py32))
        return P2E_E_INVALID;
    if (n == 0) return 0;
    if (P->H.kind == CP_FIXED_BASE_MUL) px32 = py32 = nullptr;
    return curve_dispatch(c, P, k32, k32, k32, px32, py32, nullptr, n, 0, err, valid, false, narrow, ld_narrow, wide, ld_wide);
}
extern "C" long p2e_p256_verify_witness_compact_batch(p2e_ctx* c, const p2e_curve_program* P, const uint8_t* msg32, const uint8_t* r32,
                                                      const uint8_t* s32, const uint8_t* pkx32, const uint8_t* pky32, uint32_t* narrow,
                                                      size_t ld_narrow, uint64_t* wide, size_t ld_wide, size_t n, uint8_t* err,
                                                      uint8_t* valid) {
    if (bad_common(c, n, ld_narrow) || ld_wide < n || !P || !msg32 || !r32 || !s32 || !pkx32 || !pky32 || !narrow || !wide || !err)
        return P2E_E_INVALID;
    if (P->H.kind != CP_VERIFY) {
        set_error("not a verifier program");
        return P2E_E_INVALID;
    }
    if (n == 0) return 0;
    return curve_dispatch(c, P, msg32, r32, s32, pkx32, pky32, nullptr, n, 0, err, valid, false, narrow, ld_narrow, wide, ld_wide);
}
extern "C" long p2e_curve_program_compact_layout(const p2e_curve_program* P, uint32_t* col_map, size_t cap, uint32_t* num_narrow,
                                                 uint32_t* num_wide) {
    if (!P) return P2E_E_INVALID;
    for (size_t k = 0; col_map && k < P->compact.map.size() && k < cap; k++) col_map[k] = P->compact.map[k];
    if (num_narrow) *num_narrow = P->compact.num_narrow;
    if (num_wide) *num_wide = P->compact.num_wide;
    return (long)P->compact.map.size();
}
// ---- the other targets of a curve program's circuit (SURVEY.md 8(f) ranks 1 and 2 for the rank-4 gadgets) ---------------
// Inputs as for the program's fill (multiplication programs: the scalar in msg32; r32 / s32 may be NULL there; the MSM
// program: n in msg32, m in r32, no point is read; the fixed-base program: the scalar in msg32 alone).
static bool curve_inputs_ok(const p2e_curve_program* P, const uint8_t* msg, const uint8_t* r, const uint8_t* s, const uint8_t* px,
                            const uint8_t* py) {
    if (!P || !msg) return false;
    if (P->H.kind == CP_MSM) return r != nullptr;
    if (P->H.kind == CP_FIXED_BASE_MUL) return true;
    return px && py && (P->H.kind != CP_VERIFY || (r && s));
}
// built-in-generator targets (split bits / digits, is_equal / not, random-access selections, bool products) from the
// finished witness matrix: aux[num_aux_cols][ld_aux], order and layout p2e_curve_program_aux_describe
// cols == nullptr: read the compact container's narrow matrix and write the u32 aux matrix (as run_aux)
static long run_curve_aux(p2e_ctx* c, const p2e_curve_program* P, const uint8_t* msg32, const uint8_t* r32, const uint8_t* s32,
                          const uint8_t* pkx32, const uint8_t* pky32, const uint64_t* cols, size_t ld, const uint32_t* narrow, size_t ldn,
                          void* aux, size_t ld_aux, size_t n, uint8_t* err) {
    const bool compact = cols == nullptr;
    const host::ScheduleBuilder& sb = P->H.sb;
    Staged S(c);
    msg32 = S.in(msg32, 32 * n);
    if (r32) r32 = S.in(r32, 32 * n);
    if (s32) s32 = S.in(s32, 32 * n);
    if (pkx32) pkx32 = S.in(pkx32, 32 * n);
    if (pky32) pky32 = S.in(pky32, 32 * n);
    if (compact)
        narrow = S.in(narrow, (size_t)P->compact.num_narrow * ldn * 4);
    else
        cols = S.in(cols, (size_t)sb.prog.num_cols * ld * 8);
    aux = S.out((char*)aux, (size_t)sb.aux_tab.num_aux_cols * ld_aux * (compact ? 4 : 8));
    err = S.out(err, n);
    if (S.rc) return S.done(S.rc);
    if (int rc = ensure_scratch(c, n * sizeof(u32))) return S.done(rc);
    ZERO_COUNTER(c);
    u32* err32 = (u32*)c->scratch;
    HIP_TRY(hipMemsetAsync(err32, 0, n * sizeof(u32), c->stream));
    AuxArgs A{cols, ld, aux, ld_aux, n, pky32, P->d_cpts.get(), P->d_fbtab.get(), P->tab.aux_items.get(), P->tab.aux_tab.get(),
              err32, narrow, ldn, compact ? P->tab.wide_before.get() : nullptr, {}};
    A.in[INPUT_PY] = pky32;
    A.in[INPUT_PX] = pkx32;
    A.in[INPUT_MSG] = msg32;
    A.in[INPUT_R] = r32 ? r32 : msg32;
    A.in[INPUT_S] = s32 ? s32 : msg32;
    // (A.in[INPUT_QX / INPUT_QY] stay null: p2e_curve_program_create refuses a program whose aux items would read q)
    const unsigned gx = (unsigned)((n + BS - 1) / BS), items = (unsigned)sb.aux_items.size();
    const bool wide_ok = (ld_aux % 2 == 0) && ((reinterpret_cast<uintptr_t>(aux) & (compact ? 7 : 15)) == 0) && !narrow_stores_forced();
    const size_t n_wide = wide_ok ? (n / BS) * BS : 0;
    const dim3 gw((unsigned)(n_wide / BS), items), gt((unsigned)((n - n_wide + BS - 1) / BS), items);
    if (compact) {
        if (n_wide) hipLaunchKernelGGL(kc_aux<3>, gw, dim3(BS), 0, c->stream, A, (size_t)0);
        if (n > n_wide) hipLaunchKernelGGL(kc_aux<2>, gt, dim3(BS), 0, c->stream, A, n_wide);
    } else {
        if (n_wide) hipLaunchKernelGGL(kc_aux<1>, gw, dim3(BS), 0, c->stream, A, (size_t)0);
        if (n > n_wide) hipLaunchKernelGGL(kc_aux<0>, gt, dim3(BS), 0, c->stream, A, n_wide);
    }
    hipLaunchKernelGGL(k_finalize, dim3(gx), dim3(BS), 0, c->stream, err32, (const uint8_t*)nullptr, err, (uint8_t*)nullptr, n, c->d_counter);
    c->have_phases = false;
    return S.done(finish_call(c));
}
extern "C" long p2e_curve_program_aux_witness_batch(p2e_ctx* c, const p2e_curve_program* P, const uint8_t* msg32, const uint8_t* r32,
                                                    const uint8_t* s32, const uint8_t* pkx32, const uint8_t* pky32, const uint64_t* cols,
                                                    size_t ld, uint64_t* aux, size_t ld_aux, size_t n, uint8_t* err) {
    if (bad_common(c, n, ld) || !curve_inputs_ok(P, msg32, r32, s32, pkx32, pky32) || !cols || !aux || !err || ld_aux < n) {
        if (c && ld_aux < n) set_error("ld_aux < n");
        return P2E_E_INVALID;
    }
    if (n == 0) return 0;
    return run_curve_aux(c, P, msg32, r32, s32, pkx32, pky32, cols, ld, nullptr, 0, aux, ld_aux, n, err);
}
extern "C" long p2e_curve_program_aux_witness_compact_batch(p2e_ctx* c, const p2e_curve_program* P, const uint8_t* msg32,
                                                            const uint8_t* r32, const uint8_t* s32, const uint8_t* pkx32,
                                                            const uint8_t* pky32, const uint32_t* narrow, size_t ld_narrow, uint32_t* aux32,
                                                            size_t ld_aux, size_t n, uint8_t* err) {
    if (bad_common(c, n, ld_narrow) || !curve_inputs_ok(P, msg32, r32, s32, pkx32, pky32) || !narrow || !aux32 || !err || ld_aux < n) {
        if (c && ld_aux < n) set_error("ld_aux < n");
        return P2E_E_INVALID;
    }
    if (n == 0) return 0;
    return run_curve_aux(c, P, msg32, r32, s32, pkx32, pky32, nullptr, 0, narrow, ld_narrow, aux32, ld_aux, n, err);
}
// gate-internal values of the built-in gates behind the windows (is_equal internals, RandomAccessGate index bits), from
// the aux matrix: gate[num_gate_cols][ld_gate] (curve_scalar_mul has none)
static bool curve_gate_args_ok(p2e_ctx* c, const p2e_curve_program* P, const void* aux, size_t ld_aux, const uint64_t* gate, size_t ld_gate,
                               size_t n) {
    if (bad_common(c, n, ld_aux) || !P || !aux || !gate || ld_gate < n || P->H.sb.gate_items.empty()) {
        if (c && P && P->H.sb.gate_items.empty()) set_error("this program has no gate-internal values");
        return false;
    }
    return true;
}
extern "C" long p2e_curve_program_gate_internal_batch(p2e_ctx* c, const p2e_curve_program* P, const uint64_t* aux, size_t ld_aux,
                                                      uint64_t* gate, size_t ld_gate, size_t n) {
    if (!curve_gate_args_ok(c, P, aux, ld_aux, gate, ld_gate, n)) return P2E_E_INVALID;
    if (n == 0) return 0;
    const host::ScheduleBuilder& sb = P->H.sb;
    return run_gate(c, aux, false, ld_aux, gate, ld_gate, n, sb.aux_tab.num_aux_cols, sb.num_gate_cols, P->tab.gate_items.get(),
                    (unsigned)sb.gate_items.size());
}
extern "C" long p2e_curve_program_gate_internal_compact_batch(p2e_ctx* c, const p2e_curve_program* P, const uint32_t* aux32, size_t ld_aux,
                                                              uint64_t* gate, size_t ld_gate, size_t n) {
    if (!curve_gate_args_ok(c, P, aux32, ld_aux, gate, ld_gate, n)) return P2E_E_INVALID;
    if (n == 0) return 0;
    const host::ScheduleBuilder& sb = P->H.sb;
    return run_gate(c, aux32, true, ld_aux, gate, ld_gate, n, sb.aux_tab.num_aux_cols, sb.num_gate_cols, P->tab.gate_items.get(),
                    (unsigned)sb.gate_items.size());
}
// constraint-block (U29 gate) values from the finished witness and aux matrices: ux[num_ux_cols][ld_ux], u32 or u64
static UxCall curve_ux_call(const p2e_curve_program* P, const uint8_t* msg32, const uint8_t* r32, const uint8_t* s32, const uint8_t* pkx32,
                            const uint8_t* pky32, const uint8_t* qx32, const uint8_t* qy32, void* ux, int ux_u32, size_t ld_ux, size_t n,
                            uint8_t* err) {
    const host::ScheduleBuilder& sb = P->H.sb;
    UxCall U;
    U.in[INPUT_PY] = pky32;
    U.in[INPUT_PX] = pkx32;
    U.in[INPUT_MSG] = msg32;
    U.in[INPUT_R] = r32;
    U.in[INPUT_S] = s32;
    if (P->H.kind == CP_MSM) {
        U.in[INPUT_QX] = qx32;
        U.in[INPUT_QY] = qy32;
    }
    U.ux = ux;
    U.ux_u32 = ux_u32;
    U.ld_ux = ld_ux;
    U.n = n;
    U.err = err;
    U.num_cols = (u32)sb.prog.num_cols;
    U.num_narrow = P->compact.num_narrow;
    U.num_aux_cols = sb.aux_tab.num_aux_cols;
    U.num_ux_cols = sb.num_ux_cols;
    U.d_consts = P->d_constv.get();
    U.d_items = P->tab.ux_items.get();
    U.d_items_compact = P->tab.ux_items_compact.get();
    U.items = (unsigned)sb.ux_items.size();
    return U;
}
static long run_curve_ux_u64(p2e_ctx* c, UxCall U, const uint64_t* cols, size_t ld, const uint64_t* aux, size_t ld_aux) {
    U.cols = cols;
    U.ld = ld;
    U.aux = aux;
    U.ld_aux = ld_aux;
    static const UxKernel kern[4] = {kc_ux<0>, kc_ux<1>, kc_ux<2>, kc_ux<3>};
    return run_ux(c, U, kern);
}
extern "C" long p2e_curve_program_ux_witness_batch(p2e_ctx* c, const p2e_curve_program* P, const uint8_t* msg32, const uint8_t* r32,
                                                   const uint8_t* s32, const uint8_t* pkx32, const uint8_t* pky32, const uint64_t* cols,
                                                   size_t ld, const uint64_t* aux, size_t ld_aux, void* ux, int ux_u32, size_t ld_ux,
                                                   size_t n, uint8_t* err) {
    if (c && P && P->H.kind == CP_MSM) {
        set_error("the constraint-block pass of the MSM program reads q, and this signature has no slot for q: call "
                  "p2e_curve_msm_ux_witness_batch (u64 matrices) or p2e_curve_program_ux_witness_compact_batch");
        return P2E_E_INVALID;
    }
    if (bad_common(c, n, ld) || !curve_inputs_ok(P, msg32, r32, s32, pkx32, pky32) || !cols || !aux || !ux || !err || ld_aux < n || ld_ux < n) {
        if (c && (ld_aux < n || ld_ux < n)) set_error("ld_aux / ld_ux < n");
        return P2E_E_INVALID;
    }
    if (n == 0) return 0;
    return run_curve_ux_u64(c, curve_ux_call(P, msg32, r32, s32, pkx32, pky32, nullptr, nullptr, ux, ux_u32, ld_ux, n, err), cols, ld, aux,
                            ld_aux);
}
// the MSM program's pass on the u64 matrices: its table additions read q (P2E_SRC_INPUT slots 5 and 6)
extern "C" long p2e_curve_msm_ux_witness_batch(p2e_ctx* c, const p2e_curve_program* P, const uint8_t* px32, const uint8_t* py32,
                                               const uint8_t* qx32, const uint8_t* qy32, const uint8_t* n32, const uint8_t* m32,
                                               const uint64_t* cols, size_t ld, const uint64_t* aux, size_t ld_aux, void* ux, int ux_u32,
                                               size_t ld_ux, size_t n, uint8_t* err) {
    if (bad_common(c, n, ld) || !P || !cols || !aux || !ux || !err || ld_aux < n || ld_ux < n) {
        if (c && ld >= n && (ld_aux < n || ld_ux < n)) set_error("ld_aux / ld_ux < n");
        return P2E_E_INVALID;
    }
    if (!curve_msm_args_ok(P) || !curve_msm_ux_inputs_ok(px32, py32, qx32, qy32, n32, m32)) return P2E_E_INVALID;
    if (n == 0) return 0;
    return run_curve_ux_u64(c, curve_ux_call(P, n32, m32, nullptr, px32, py32, qx32, qy32, ux, ux_u32, ld_ux, n, err), cols, ld, aux, ld_aux);
}
// every program kind inside the compact container; qx32 / qy32 are read by the MSM program alone
extern "C" long p2e_curve_program_ux_witness_compact_batch(p2e_ctx* c, const p2e_curve_program* P, const uint8_t* msg32, const uint8_t* r32,
                                                           const uint8_t* s32, const uint8_t* pkx32, const uint8_t* pky32,
                                                           const uint8_t* qx32, const uint8_t* qy32, const uint32_t* narrow, size_t ld_narrow,
                                                           const uint32_t* aux32, size_t ld_aux, void* ux, int ux_u32, size_t ld_ux, size_t n,
                                                           uint8_t* err) {
    if (bad_common(c, n, ld_narrow) || !curve_inputs_ok(P, msg32, r32, s32, pkx32, pky32) || !narrow || !aux32 || !ux || !err || ld_aux < n ||
        ld_ux < n) {
        if (c && (ld_aux < n || ld_ux < n)) set_error("ld_aux / ld_ux < n");
        return P2E_E_INVALID;
    }
    if (P->H.kind == CP_MSM && !curve_msm_ux_inputs_ok(pkx32, pky32, qx32, qy32, msg32, r32)) return P2E_E_INVALID;
    if (n == 0) return 0;
    UxCall U = curve_ux_call(P, msg32, r32, s32, pkx32, pky32, qx32, qy32, ux, ux_u32, ld_ux, n, err);
    U.narrow = narrow;
    U.ldn = ld_narrow;
    U.aux = aux32;
    U.ld_aux = ld_aux;
    static const UxKernel kern[4] = {kc_ux_compact<0>, kc_ux_compact<1>, kc_ux_compact<2>, kc_ux_compact<3>};
    return run_ux(c, U, kern);
}
// wire-matrix assembly (SURVEY.md 8(f) rank 3) for a curve program's four matrices: the map of p2e_wire_map_create with this
// program's column counts as limits; p2e_assemble_wires / p2e_wire_map_destroy take the result as they are
extern "C" int p2e_curve_program_wire_map_create(p2e_ctx* c, const p2e_curve_program* P, const p2e_wire_map_entry* entries, size_t count,
                                                 uint32_t num_wires, uint32_t degree, p2e_wire_map** out) {
    if (!P) return P2E_E_INVALID;
    const host::ScheduleBuilder& sb = P->H.sb;
    const u32 limit[4] = {(u32)sb.prog.num_cols, sb.aux_tab.num_aux_cols, sb.num_ux_cols, sb.num_gate_cols};
    return make_wire_map(c, limit, P->compact, entries, count, num_wires, degree, out);
}
// synthetic valid signatures on a curve (host side; tests and benches)
extern "C" int p2e_synth_signatures_curve(int curve, uint64_t seed, size_t first, size_t n, uint8_t* msg32, uint8_t* r32, uint8_t* s32,
                                          uint8_t* pkx32, uint8_t* pky32) {
    if ((curve != 0 && curve != 1) || !msg32 || !r32 || !s32 || !pkx32 || !pky32) return P2E_E_INVALID;
#pragma omp parallel for schedule(dynamic, 16)
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
#endif   // P2E_HAS(0)

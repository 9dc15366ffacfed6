// CPU harness of the compact-source kernel bodies (test infrastructure only): the bodies k_ux_compact, k_gate_compact,
// kc_aux<2>, kc_ux_compact and (u64 source, with q) kc_ux run per lane, compiled with g++ against the library's headers,
// and the host-side compact layout with the check contexts and curve programs make when they are created.
// tests/emu/p2e_emu.cpp holds the u64-source bodies these are compared with.
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../plonky2-ecdsa_amd/csrc/curve_program.hpp"
#include "../../plonky2-ecdsa_amd/csrc/schedule.hpp"

using namespace p2e;

namespace {
bool builtin_program(host::ScheduleBuilder& sb, int program) {
    if (program == 0)
        sb.verify_secp256k1_message_circuit();
    else if (program == 1)
        sb.glv_mul_circuit();
    else
        return false;
    return true;
}
bool curve_program(host::CurveProgramHost& H, int kind, int curve, const uint8_t* bx, const uint8_t* by) {
    Aff blind{};
    if (bx && by) {
        memcpy(blind.x.w, bx, 32);
        memcpy(blind.y.w, by, 32);
    }
    return host::make_curve_program(H, kind, curve, blind);
}
void fill_inv16(GateArgs& A) {
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
}
long run_gate(const host::ScheduleBuilder& sb, const uint32_t* aux32, size_t ald, uint64_t* gate, size_t gld, size_t n) {
    GateArgs A{};
    A.aux32 = aux32;
    A.ald = ald;
    A.gate = gate;
    A.gld = gld;
    A.n = n;
    A.items = sb.gate_items.data();
    fill_inv16(A);
    for (int item = 0; item < (int)sb.gate_items.size(); item++)
        for (size_t i = 0; i < n; i++) body_gate<Emit, true>(A, item, i);
    return (long)sb.num_gate_cols;
}
// in: packed inputs by INPUT_* slot (null: none).  narrow != null: compact source (aux = u32 matrix), else cols / aux u64.
template <bool CURVE>
long run_ux(const host::ScheduleBuilder& sb, const U256* consts, const uint8_t* const in[7], const uint32_t* narrow, size_t ldn,
            const uint64_t* cols, size_t ld, const void* aux, size_t ald, void* ux, int ux_u32, size_t uld, size_t n, uint8_t* err) {
    const host::CompactLayout L = host::compact_layout(sb.gens, (size_t)sb.prog.num_cols);
    const std::vector<UxItem> citems = host::ux_items_compact(sb.ux_items, L.map);
    std::vector<u32> err32(n);
    UxArgs A{};
    A.cols = cols;
    A.ld = ld;
    A.ald = ald;
    if (narrow) {
        A.nar = narrow;
        A.ldn = ldn;
        A.aux32 = static_cast<const u32*>(aux);
    } else {
        A.aux = static_cast<const u64*>(aux);
    }
    A.ux = ux;
    A.uld = uld;
    A.n = n;
    for (int k = 0; k < 7; k++) A.in[k] = in[k];
    if (!A.in[INPUT_R]) A.in[INPUT_R] = A.in[INPUT_MSG];
    if (!A.in[INPUT_S]) A.in[INPUT_S] = A.in[INPUT_MSG];
    A.consts = consts;
    A.items = narrow ? citems.data() : sb.ux_items.data();
    A.err = err32.data();
#pragma omp parallel for
    for (long long item = 0; item < (long long)sb.ux_items.size(); item++)
        for (size_t i = 0; i < n; i++) {
            if (CURVE) {
                if (narrow && ux_u32)
                    body_ux_cv<Emit32, true>(A, (int)item, i);
                else if (narrow)
                    body_ux_cv<Emit, true>(A, (int)item, i);
                else if (ux_u32)
                    body_ux_cv<Emit32>(A, (int)item, i);
                else
                    body_ux_cv<Emit>(A, (int)item, i);
            } else {
                if (ux_u32)
                    body_ux<Emit32, true>(A, (int)item, i);
                else
                    body_ux<Emit, true>(A, (int)item, i);
            }
        }
    for (size_t i = 0; i < n; i++) err[i] = (uint8_t)err32[i];
    return (long)sb.num_ux_cols;
}
long layout_out(const host::ScheduleBuilder& sb, uint32_t* col_map, size_t cap, uint32_t* num_narrow, uint32_t* num_wide, int* ux_ok) {
    const host::CompactLayout L = host::compact_layout(sb.gens, (size_t)sb.prog.num_cols);
    for (size_t k = 0; col_map && k < L.map.size() && k < cap; k++) col_map[k] = L.map[k];
    if (num_narrow) *num_narrow = L.num_narrow;
    if (num_wide) *num_wide = L.num_wide;
    std::string why;
    if (ux_ok) *ux_ok = host::ux_items_compact_ok(sb.ux_items, L.map, why) ? 1 : 0;
    return (long)L.map.size();
}
long gens_out(const host::ScheduleBuilder& sb, int32_t* kinds, uint32_t* first, uint32_t* ncols, int32_t* nops, uint32_t* src, uint8_t* nl,
              size_t cap) {
    const auto& g = sb.gens;
    for (size_t k = 0; kinds && k < g.size() && k < cap; k++) {
        kinds[k] = g[k].kind;
        first[k] = g[k].col;
        ncols[k] = g[k].ncols;
        nops[k] = g[k].nops;
        for (int j = 0; j < 4; j++) {
            src[4 * k + j] = g[k].src[j];
            nl[4 * k + j] = g[k].nl[j];
        }
    }
    return (long)g.size();
}
}   // namespace

extern "C" {
// ---- built-in programs (0 verify, 1 glv_mul) ---------------------------------------------------------------------------
long emuc_ux(int program, const uint8_t* msg, const uint8_t* r, const uint8_t* s, const uint8_t* pkx, const uint8_t* pky,
             const uint32_t* narrow, size_t ldn, const uint32_t* aux32, size_t ald, void* ux, int ux_u32, size_t uld, size_t n, uint8_t* err) {
    host::ScheduleBuilder sb;
    if (!builtin_program(sb, program)) return -1;
    U256 cv[NUM_CONSTV];
    for (u32 id = 0; id < NUM_CONSTV; id++) cv[id] = host::ScheduleBuilder::const_value(id);
    const uint8_t* in[7] = {};
    in[INPUT_PY] = pky;
    in[INPUT_PX] = pkx;
    in[INPUT_MSG] = msg;
    in[INPUT_R] = r;
    in[INPUT_S] = s;
    return run_ux<false>(sb, cv, in, narrow, ldn, nullptr, 0, aux32, ald, ux, ux_u32, uld, n, err);
}
long emuc_gate(int program, const uint32_t* aux32, size_t ald, uint64_t* gate, size_t gld, size_t n) {
    host::ScheduleBuilder sb;
    if (!builtin_program(sb, program)) return -1;
    return run_gate(sb, aux32, ald, gate, gld, n);
}
// ---- curve programs (kind / curve: include/p2e.h P2E_CP_* / P2E_CURVE_*; the MSM program ignores the point) -------------------
// each returns the output matrix' column count (call with n = 0 to query it), -1 for an unknown program
long emuc_curve_aux(int kind, int curve, const uint8_t* bx, const uint8_t* by, const uint8_t* msg, const uint8_t* r, const uint8_t* s,
                    const uint8_t* pkx, const uint8_t* pky, const uint32_t* narrow, size_t ldn, uint32_t* aux32, size_t ald, size_t n,
                    uint8_t* err) {
    host::CurveProgramHost H;
    if (!curve_program(H, kind, curve, bx, by)) return -1;
    const host::ScheduleBuilder& sb = H.sb;
    if (n == 0) return (long)sb.aux_tab.num_aux_cols;
    const host::CompactLayout L = host::compact_layout(sb.gens, (size_t)sb.prog.num_cols);
    std::vector<u32> err32(n);
    AuxArgs A{nullptr, 0, aux32, ald, n, pky, sb.gpts.data(), sb.gfbtab.data(), sb.aux_items.data(), &sb.aux_tab, err32.data(),
              narrow, ldn, L.wide_before.data(), {}};
    A.in[INPUT_PY] = pky;
    A.in[INPUT_PX] = pkx;
    A.in[INPUT_MSG] = msg;
    A.in[INPUT_R] = r ? r : msg;
    A.in[INPUT_S] = s ? s : msg;
    for (int item = 0; item < (int)sb.aux_items.size(); item++) {
#pragma omp parallel for
        for (long long i = 0; i < (long long)n; i++) body_aux_cv<Emit32>(A, item, (size_t)i);
    }
    for (size_t i = 0; i < n; i++) err[i] = (uint8_t)err32[i];
    return (long)sb.aux_tab.num_aux_cols;
}
long emuc_curve_gate(int kind, int curve, const uint8_t* bx, const uint8_t* by, const uint32_t* aux32, size_t ald, uint64_t* gate, size_t gld,
                     size_t n) {
    host::CurveProgramHost H;
    if (!curve_program(H, kind, curve, bx, by)) return -1;
    if (n == 0) return (long)H.sb.num_gate_cols;
    return run_gate(H.sb, aux32, ald, gate, gld, n);
}
// narrow != null: the compact source (aux = the u32 aux matrix); else the u64 matrices cols / aux (the MSM program's pass
// with q, which tests/emu has no entry for)
long emuc_curve_ux(int kind, int curve, const uint8_t* bx, const uint8_t* by, const uint8_t* msg, const uint8_t* r, const uint8_t* s,
                   const uint8_t* pkx, const uint8_t* pky, const uint8_t* qx, const uint8_t* qy, const uint32_t* narrow, size_t ldn,
                   const uint64_t* cols, size_t ld, const void* aux, size_t ald, void* ux, int ux_u32, size_t uld, size_t n, uint8_t* err) {
    host::CurveProgramHost H;
    if (!curve_program(H, kind, curve, bx, by)) return -1;
    const host::ScheduleBuilder& sb = H.sb;
    if (n == 0) return (long)sb.num_ux_cols;
    std::vector<U256> cv(AUX_GCONST_BASE + sb.gvals.size(), u256_zero());
    for (size_t k = 0; k < sb.gpts.size(); k++) {
        cv[2 * k] = sb.gpts[k].x;
        cv[2 * k + 1] = sb.gpts[k].y;
    }
    for (size_t j = 0; j < sb.gvals.size(); j++) cv[AUX_GCONST_BASE + j] = sb.gvals[j];
    const uint8_t* in[7] = {};
    in[INPUT_PY] = pky;
    in[INPUT_PX] = pkx;
    in[INPUT_MSG] = msg;
    in[INPUT_R] = r;
    in[INPUT_S] = s;
    in[INPUT_QX] = qx;
    in[INPUT_QY] = qy;
    return run_ux<true>(sb, cv.data(), in, narrow, ldn, cols, ld, aux, ald, ux, ux_u32, uld, n, err);
}
// what p2e_curve_program_ux_describe reports (a program object needs a device): (first, count) per generator, the generator count
long emuc_curve_ux_describe(int kind, int curve, const uint8_t* bx, const uint8_t* by, uint32_t* first, uint32_t* count, size_t cap) {
    host::CurveProgramHost H;
    if (!curve_program(H, kind, curve, bx, by)) return -1;
    const host::ScheduleBuilder& sb = H.sb;
    for (size_t k = 0; first && count && k < sb.ux_first.size() && k < cap; k++) {
        first[k] = sb.ux_first[k];
        count[k] = sb.ux_count[k];
    }
    return (long)sb.ux_first.size();
}
// ---- layout: the generator table with its wiring, the compact layout, and the library's own consecutive-rows check ------------
long emuc_gens(int program, int32_t* kinds, uint32_t* first, uint32_t* ncols, int32_t* nops, uint32_t* src, uint8_t* nl, size_t cap) {
    host::ScheduleBuilder sb;
    if (!builtin_program(sb, program)) return -1;
    return gens_out(sb, kinds, first, ncols, nops, src, nl, cap);
}
long emuc_layout(int program, uint32_t* col_map, size_t cap, uint32_t* num_narrow, uint32_t* num_wide, int* ux_ok) {
    host::ScheduleBuilder sb;
    if (!builtin_program(sb, program)) return -1;
    return layout_out(sb, col_map, cap, num_narrow, num_wide, ux_ok);
}
long emuc_curve_gens(int kind, int curve, const uint8_t* bx, const uint8_t* by, int32_t* kinds, uint32_t* first, uint32_t* ncols,
                     int32_t* nops, uint32_t* src, uint8_t* nl, size_t cap) {
    host::CurveProgramHost H;
    if (!curve_program(H, kind, curve, bx, by)) return -1;
    return gens_out(H.sb, kinds, first, ncols, nops, src, nl, cap);
}
long emuc_curve_layout(int kind, int curve, const uint8_t* bx, const uint8_t* by, uint32_t* col_map, size_t cap, uint32_t* num_narrow,
                       uint32_t* num_wide, int* ux_ok) {
    host::CurveProgramHost H;
    if (!curve_program(H, kind, curve, bx, by)) return -1;
    return layout_out(H.sb, col_map, cap, num_narrow, num_wide, ux_ok);
}
// the check on a layout of the caller's: 1 if the compact ux pass may walk it, 0 otherwise (the message in why[cap])
int emuc_ux_layout_ok(int program, const uint32_t* col_map, size_t count, char* why, size_t cap) {
    host::ScheduleBuilder sb;
    if (!builtin_program(sb, program)) return -1;
    std::string w;
    const bool ok = host::ux_items_compact_ok(sb.ux_items, std::vector<u32>(col_map, col_map + count), w);
    if (why && cap) {
        strncpy(why, w.c_str(), cap - 1);
        why[cap - 1] = 0;
    }
    return ok ? 1 : 0;
}
}

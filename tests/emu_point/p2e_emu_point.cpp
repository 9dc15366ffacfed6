// CPU harness of the per-element point arithmetic (test infrastructure only): body_point_mul, body_point_lincomb and
// body_point_add of csrc/point_arith.hpp run per element, compiled with g++ against the library's headers, on either
// curve and every plan, with the fixed-base tables the library uploads.  emup_glv_decompose exposes what the GLV walk
// consumes, so that the test can assert k = +-k1 +- k2 lambda (mod n) and the 128-bit bound on every scalar.
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../plonky2-ecdsa_amd/csrc/consts.hpp"
#include "../../plonky2-ecdsa_amd/csrc/curve_program.hpp"
#include "../../plonky2-ecdsa_amd/csrc/point_arith.hpp"

using namespace p2e;

namespace {
template <class CV>
const Aff* point_table();
template <>
const Aff* point_table<Secp256k1>() {
    return host::consts().fbtab.data();
}
template <>
const Aff* point_table<P256>() {
    static const std::vector<Aff> t = host::fixed_base_table_cv<P256>(host::generator_cv<P256>());
    return t.data();
}
template <class CV, int PLAN>
long run_mul(const uint8_t* k, const uint8_t* px, const uint8_t* py, uint8_t* ox, uint8_t* oy, size_t n, uint8_t* err) {
    long bad = 0;
#pragma omp parallel for schedule(dynamic, 16) reduction(+ : bad)
    for (long long i = 0; i < (long long)n; i++) {
        err[i] = body_point_mul<CV, PLAN>(k, px, py, ox, oy, (size_t)i);
        bad += err[i] != 0;
    }
    return bad;
}
template <class CV, int PLAN>
long run_lincomb(const uint8_t* a, const uint8_t* b, const uint8_t* px, const uint8_t* py, uint8_t* ox, uint8_t* oy, size_t n,
                 uint8_t* err) {
    const Aff* T = point_table<CV>();
    long bad = 0;
#pragma omp parallel for schedule(dynamic, 16) reduction(+ : bad)
    for (long long i = 0; i < (long long)n; i++) {
        err[i] = body_point_lincomb<CV, PLAN>(T, a, b, px, py, ox, oy, (size_t)i);
        bad += err[i] != 0;
    }
    return bad;
}
template <class CV>
long run_add(const uint8_t* px, const uint8_t* py, const uint8_t* qx, const uint8_t* qy, uint8_t* ox, uint8_t* oy, size_t n,
             uint8_t* err) {
    long bad = 0;
#pragma omp parallel for schedule(dynamic, 16) reduction(+ : bad)
    for (long long i = 0; i < (long long)n; i++) {
        err[i] = body_point_add<CV>(px, py, qx, qy, ox, oy, (size_t)i);
        bad += err[i] != 0;
    }
    return bad;
}
// the library's rule (p2e_hip.hip point_mul_prepare): -1 = P2E_E_INVALID, else the walk; AUTO is GLV on secp256k1
int chosen_plan(int curve, int plan) {
    if ((curve != 0 && curve != 1) || plan < MUL_PLAN_AUTO || plan > MUL_PLAN_GLV) return -1;
    if (plan == MUL_PLAN_GLV && curve != 0) return -1;
    return plan == MUL_PLAN_AUTO ? (curve == 0 ? MUL_PLAN_GLV : MUL_PLAN_PLAIN) : plan;
}
}  // namespace

extern "C" long emup_mul(int curve, int plan, const uint8_t* k, const uint8_t* px, const uint8_t* py, uint8_t* ox, uint8_t* oy,
                         size_t n, uint8_t* err) {
    const int p = chosen_plan(curve, plan);
    if (p < 0) return -1;
    if (curve == 1) return run_mul<P256, MUL_PLAN_PLAIN>(k, px, py, ox, oy, n, err);
    return p == MUL_PLAN_GLV ? run_mul<Secp256k1, MUL_PLAN_GLV>(k, px, py, ox, oy, n, err)
                             : run_mul<Secp256k1, MUL_PLAN_PLAIN>(k, px, py, ox, oy, n, err);
}
extern "C" long emup_lincomb(int curve, int plan, const uint8_t* a, const uint8_t* b, const uint8_t* px, const uint8_t* py,
                             uint8_t* ox, uint8_t* oy, size_t n, uint8_t* err) {
    const int p = chosen_plan(curve, plan);
    if (p < 0) return -1;
    if (curve == 1) return run_lincomb<P256, MUL_PLAN_PLAIN>(a, b, px, py, ox, oy, n, err);
    return p == MUL_PLAN_GLV ? run_lincomb<Secp256k1, MUL_PLAN_GLV>(a, b, px, py, ox, oy, n, err)
                             : run_lincomb<Secp256k1, MUL_PLAN_PLAIN>(a, b, px, py, ox, oy, n, err);
}
extern "C" long emup_add(int curve, const uint8_t* px, const uint8_t* py, const uint8_t* qx, const uint8_t* qy, uint8_t* ox,
                         uint8_t* oy, size_t n, uint8_t* err) {
    if (curve != 0 && curve != 1) return -1;
    return curve == 0 ? run_add<Secp256k1>(px, py, qx, qy, ox, oy, n, err) : run_add<P256>(px, py, qx, qy, ox, oy, n, err);
}
// secp256k1: |k1|, |k2| (32 bytes each, little-endian) and the two sign bytes of glv_decompose(k mod n)
extern "C" void emup_glv_decompose(const uint8_t* k32, uint8_t* k1, uint8_t* k2, uint8_t* neg1, uint8_t* neg2, size_t n) {
    for (size_t i = 0; i < n; i++) {
        const GlvOut g = glv_decompose(sign_scalar<Secp256k1>(k32, i));
        store_packed(k1, i, g.k1);
        store_packed(k2, i, g.k2);
        neg1[i] = (uint8_t)g.n1;
        neg2[i] = (uint8_t)g.n2;
    }
}
// lambda and beta as the walk uses them (32 bytes each, little-endian)
extern "C" void emup_glv_constants(uint8_t* lambda32, uint8_t* beta32) {
    store_packed(lambda32, 0, glv_lambda());
    store_packed(beta32, 0, glv_beta());
}

// CPU harness of the recovery kernel body and of the recoverable signer (test infrastructure only): body_recover of
// csrc/recover.hpp and body_sign<CV, PLAN, true> of csrc/sign.hpp run per element, compiled with g++ against the library's
// headers, on either curve, with the fixed-base tables the library uploads.
#include <cstdint>
#include <vector>

#include "../../plonky2-ecdsa_amd/csrc/consts.hpp"
#include "../../plonky2-ecdsa_amd/csrc/curve_program.hpp"
#include "../../plonky2-ecdsa_amd/csrc/recover.hpp"

using namespace p2e;

namespace {
template <class CV>
const Aff* recover_table();
template <>
const Aff* recover_table<Secp256k1>() {
    return host::consts().fbtab.data();
}
template <>
const Aff* recover_table<P256>() {
    static const std::vector<Aff> t = host::fixed_base_table_cv<P256>(host::generator_cv<P256>());
    return t.data();
}
template <class CV>
long run_recover(const uint8_t* msg, const uint8_t* r, const uint8_t* s, const uint8_t* v, uint8_t* pkx, uint8_t* pky, size_t n,
                 uint8_t* err) {
    const Aff* T = recover_table<CV>();
    long bad = 0;
#pragma omp parallel for schedule(dynamic, 16) reduction(+ : bad)
    for (long long i = 0; i < (long long)n; i++) {
        err[i] = body_recover<CV>(T, msg, r, s, v, pkx, pky, (size_t)i);
        bad += err[i] != 0;
    }
    return bad;
}
template <class CV, int PLAN>
long run_sign_recoverable(const uint8_t* msg, const uint8_t* sk, const uint8_t* k, uint8_t* r, uint8_t* s, uint8_t* v, size_t n,
                          uint8_t* err) {
    const Aff* T = recover_table<CV>();
    long bad = 0;
#pragma omp parallel for schedule(dynamic, 16) reduction(+ : bad)
    for (long long i = 0; i < (long long)n; i++) {
        err[i] = body_sign<CV, PLAN, true>(T, msg, sk, k, r, s, (size_t)i, 0, v);
        bad += err[i] != 0;
    }
    return bad;
}
}  // namespace

extern "C" long emur_recover(int curve, const uint8_t* msg, const uint8_t* r, const uint8_t* s, const uint8_t* v, uint8_t* pkx,
                             uint8_t* pky, size_t n, uint8_t* err) {
    if (curve != 0 && curve != 1) return -1;
    return curve == 0 ? run_recover<Secp256k1>(msg, r, s, v, pkx, pky, n, err) : run_recover<P256>(msg, r, s, v, pkx, pky, n, err);
}
extern "C" long emur_sign_recoverable(int curve, int plan, const uint8_t* msg, const uint8_t* sk, const uint8_t* k, uint8_t* r,
                                      uint8_t* s, uint8_t* v, size_t n, uint8_t* err) {
    if ((curve != 0 && curve != 1) || (plan != SIGN_PLAN_LANE && plan != SIGN_PLAN_QUAD)) return -1;
    if (curve == 0)
        return plan == SIGN_PLAN_LANE ? run_sign_recoverable<Secp256k1, SIGN_PLAN_LANE>(msg, sk, k, r, s, v, n, err)
                                      : run_sign_recoverable<Secp256k1, SIGN_PLAN_QUAD>(msg, sk, k, r, s, v, n, err);
    return plan == SIGN_PLAN_LANE ? run_sign_recoverable<P256, SIGN_PLAN_LANE>(msg, sk, k, r, s, v, n, err)
                                  : run_sign_recoverable<P256, SIGN_PLAN_QUAD>(msg, sk, k, r, s, v, n, err);
}

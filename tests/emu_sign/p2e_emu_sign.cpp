// CPU harness of the key-derivation and signing kernel bodies (test infrastructure only): body_public_key and body_sign
// of csrc/sign.hpp run per element, compiled with g++ against the library's headers, in the lane-per-scalar plan
// (plan 1) and the four-lanes-per-scalar plan (plan 2, the quad exchange in its host form), on either curve, with the
// fixed-base tables the library uploads (host::consts().fbtab, host::fixed_base_table_cv<P256>(G)).
#include <cstdint>
#include <vector>

#include "../../plonky2-ecdsa_amd/csrc/consts.hpp"
#include "../../plonky2-ecdsa_amd/csrc/curve_program.hpp"
#include "../../plonky2-ecdsa_amd/csrc/sign.hpp"

using namespace p2e;

namespace {
template <class CV>
const Aff* sign_table();
template <>
const Aff* sign_table<Secp256k1>() {
    return host::consts().fbtab.data();
}
template <>
const Aff* sign_table<P256>() {
    static const std::vector<Aff> t = host::fixed_base_table_cv<P256>(host::generator_cv<P256>());
    return t.data();
}
template <class CV, int PLAN>
long run_public_key(const uint8_t* sk, uint8_t* pkx, uint8_t* pky, size_t n, uint8_t* err) {
    const Aff* T = sign_table<CV>();
    long bad = 0;
#pragma omp parallel for schedule(dynamic, 16) reduction(+ : bad)
    for (long long i = 0; i < (long long)n; i++) {
        err[i] = body_public_key<CV, PLAN>(T, sk, pkx, pky, (size_t)i, 0);
        bad += err[i] != 0;
    }
    return bad;
}
template <class CV, int PLAN>
long run_sign(const uint8_t* msg, const uint8_t* sk, const uint8_t* k, uint8_t* r, uint8_t* s, size_t n, uint8_t* err) {
    const Aff* T = sign_table<CV>();
    long bad = 0;
#pragma omp parallel for schedule(dynamic, 16) reduction(+ : bad)
    for (long long i = 0; i < (long long)n; i++) {
        err[i] = body_sign<CV, PLAN>(T, msg, sk, k, r, s, (size_t)i, 0);
        bad += err[i] != 0;
    }
    return bad;
}
}  // namespace

extern "C" long emus_public_key(int curve, int plan, const uint8_t* sk, uint8_t* pkx, uint8_t* pky, size_t n, uint8_t* err) {
    if ((curve != 0 && curve != 1) || (plan != SIGN_PLAN_LANE && plan != SIGN_PLAN_QUAD)) return -1;
    if (curve == 0)
        return plan == SIGN_PLAN_LANE ? run_public_key<Secp256k1, SIGN_PLAN_LANE>(sk, pkx, pky, n, err)
                                      : run_public_key<Secp256k1, SIGN_PLAN_QUAD>(sk, pkx, pky, n, err);
    return plan == SIGN_PLAN_LANE ? run_public_key<P256, SIGN_PLAN_LANE>(sk, pkx, pky, n, err)
                                  : run_public_key<P256, SIGN_PLAN_QUAD>(sk, pkx, pky, n, err);
}
extern "C" long emus_sign(int curve, int plan, const uint8_t* msg, const uint8_t* sk, const uint8_t* k, uint8_t* r, uint8_t* s, size_t n,
                          uint8_t* err) {
    if ((curve != 0 && curve != 1) || (plan != SIGN_PLAN_LANE && plan != SIGN_PLAN_QUAD)) return -1;
    if (curve == 0)
        return plan == SIGN_PLAN_LANE ? run_sign<Secp256k1, SIGN_PLAN_LANE>(msg, sk, k, r, s, n, err)
                                      : run_sign<Secp256k1, SIGN_PLAN_QUAD>(msg, sk, k, r, s, n, err);
    return plan == SIGN_PLAN_LANE ? run_sign<P256, SIGN_PLAN_LANE>(msg, sk, k, r, s, n, err)
                                  : run_sign<P256, SIGN_PLAN_QUAD>(msg, sk, k, r, s, n, err);
}

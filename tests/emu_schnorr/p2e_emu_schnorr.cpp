// CPU harness of the BIP-340 layer (test infrastructure only): the bodies of csrc/schnorr.hpp run per element, compiled with
// g++ against the library's headers and the generator table the library uploads.  The aggregate's preparation mirrors the
// device's shape as far as it decides bytes: per-block partial sums of SCHNORR_AGG_LANES elements, then the finishing body.
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../plonky2-ecdsa_amd/csrc/consts.hpp"
#include "../../plonky2-ecdsa_amd/csrc/schnorr.hpp"

using namespace p2e;

namespace {
const Aff* gen_table() { return host::consts().fbtab.data(); }
}  // namespace

extern "C" void emusch_midstate(int tag, uint32_t* out8) {
    const Sha256State s = schnorr_midstate(tag);
    for (int j = 0; j < 8; j++) out8[j] = s.h[j];
}
extern "C" long emusch_public_key(const uint8_t* sk32, uint8_t* pk32, size_t n, uint8_t* err) {
    const Aff* T = gen_table();
    long bad = 0;
#pragma omp parallel for schedule(dynamic, 16) reduction(+ : bad)
    for (long long i = 0; i < (long long)n; i++) {
        err[i] = body_schnorr_public_key(T, sk32, pk32, (size_t)i);
        bad += err[i] != 0;
    }
    return bad;
}
extern "C" long emusch_sign(const uint8_t* msg32, const uint8_t* sk32, const uint8_t* aux32, uint8_t* sig64, size_t n, uint8_t* err) {
    const Aff* T = gen_table();
    long bad = 0;
#pragma omp parallel for schedule(dynamic, 16) reduction(+ : bad)
    for (long long i = 0; i < (long long)n; i++) {
        err[i] = body_schnorr_sign(T, msg32, sk32, aux32, sig64, (size_t)i);
        bad += err[i] != 0;
    }
    return bad;
}
// the inner signer alone: d (adjusted), px, msg, k' as 32 big-endian bytes each; sig64 is written only where the code is 0
extern "C" int emusch_sign_with_nonce(const uint8_t* d32, const uint8_t* px32, const uint8_t* msg32, const uint8_t* k32, uint8_t* sig64) {
    U256 rx = u256_zero(), s = u256_zero();
    const uint8_t e = schnorr_sign_with_nonce(gen_table(), schnorr_load_be(d32), schnorr_load_be(px32), schnorr_load_be(msg32),
                                              schnorr_load_be(k32), rx, s);
    if (!e) {
        schnorr_store_be(sig64, rx);
        schnorr_store_be(sig64 + 32, s);
    }
    return e;
}
extern "C" long emusch_verify(const uint8_t* msg32, const uint8_t* pk32, const uint8_t* sig64, size_t n, uint8_t* err, uint8_t* valid) {
    const Aff* T = gen_table();
    long bad = 0;
#pragma omp parallel for schedule(dynamic, 16) reduction(+ : bad)
    for (long long i = 0; i < (long long)n; i++) {
        err[i] = body_schnorr_verify(T, msg32, pk32, sig64, valid, (size_t)i);
        bad += err[i] != 0;
    }
    return bad;
}
extern "C" long emusch_xonly_decode(const uint8_t* pk32, uint8_t* px32, uint8_t* py32, size_t n, uint8_t* err) {
    long bad = 0;
#pragma omp parallel for schedule(dynamic, 16) reduction(+ : bad)
    for (long long i = 0; i < (long long)n; i++) {
        err[i] = body_xonly_decode(pk32, px32, py32, (size_t)i);
        bad += err[i] != 0;
    }
    return bad;
}
// the 2 n + 1 terms of the aggregate check into k32, px32, py32 ((2 n + 1) * 32 bytes each); err nullable; returns the flag count
extern "C" long emusch_agg_prepare(const uint8_t* msg32, const uint8_t* pk32, const uint8_t* sig64, const uint8_t* seed32, size_t n,
                                   uint8_t* k32, uint8_t* px32, uint8_t* py32, uint8_t* err) {
    const size_t blocks = (n + SCHNORR_AGG_LANES - 1) / SCHNORR_AGG_LANES;
    std::vector<U256> partial(blocks, u256_zero());
    long bad = 0;
#pragma omp parallel for schedule(dynamic, 1) reduction(+ : bad)
    for (long long b = 0; b < (long long)blocks; b++) {
        U256 sum = u256_zero();
        for (size_t i = (size_t)b * SCHNORR_AGG_LANES; i < n && i < (size_t)(b + 1) * SCHNORR_AGG_LANES; i++) {
            U256 as;
            const uint8_t e = body_schnorr_agg_prepare(msg32, pk32, sig64, seed32, n, k32, px32, py32, i, &as);
            if (err) err[i] = e;
            bad += e != 0;
            sum = fe_add<SchnorrCV::Fn>(sum, as);
        }
        partial[(size_t)b] = sum;
    }
    U256 total = u256_zero();
    for (const U256& p : partial) total = fe_add<SchnorrCV::Fn>(total, p);
    body_schnorr_agg_finish(gen_table(), total, k32, px32, py32);
    return bad;
}
extern "C" int emusch_agg_verdict(int msm_status, unsigned long long flagged) { return schnorr_agg_verdict((uint8_t)msm_status, flagged); }

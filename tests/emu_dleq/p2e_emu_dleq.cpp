// CPU harness of a P + b Q and of the DLEQ layer (test infrastructure only): body_point_lincomb2 of csrc/point_arith.hpp on either
// curve and every plan, and the bodies of csrc/dleq.hpp, run per element, compiled with g++ against the library's headers and
// the generator table the library uploads.  The functions behind the hashes are exposed with forced k and forced e.
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../plonky2-ecdsa_amd/csrc/consts.hpp"
#include "../../plonky2-ecdsa_amd/csrc/curve_program.hpp"
#include "../../plonky2-ecdsa_amd/csrc/dleq.hpp"

using namespace p2e;

namespace {
const Aff* gen_table() { return host::consts().fbtab.data(); }
template <class CV, int PLAN>
long run_lincomb2(const uint8_t* a, const uint8_t* b, const uint8_t* px, const uint8_t* py, const uint8_t* qx, const uint8_t* qy, uint8_t* ox,
                  uint8_t* oy, size_t count, uint8_t* err) {
    long bad = 0;
#pragma omp parallel for schedule(dynamic, 8) reduction(+ : bad)
    for (long long i = 0; i < (long long)count; i++) {
        err[i] = body_point_lincomb2<CV, PLAN>(a, b, px, py, qx, qy, ox, oy, (size_t)i);
        bad += err[i] != 0;
    }
    return bad;
}
Aff load_aff(const uint8_t* x32, const uint8_t* y32, size_t i) {
    Aff P;
    P.x = load_packed(x32, i), P.y = load_packed(y32, i);
    return P;
}
}  // namespace

// the library's rule (p2e_hip.hip point_mul_prepare): -1 = P2E_E_INVALID, else the walk; AUTO is GLV on secp256k1
extern "C" long emud_lincomb2(int curve, int plan, const uint8_t* a, const uint8_t* b, const uint8_t* px, const uint8_t* py, const uint8_t* qx,
                              const uint8_t* qy, uint8_t* ox, uint8_t* oy, size_t count, uint8_t* err) {
    if ((curve != 0 && curve != 1) || plan < MUL_PLAN_AUTO || plan > MUL_PLAN_GLV || (plan == MUL_PLAN_GLV && curve != 0)) return -1;
    if (curve == 1) return run_lincomb2<P256, MUL_PLAN_PLAIN>(a, b, px, py, qx, qy, ox, oy, count, err);
    return plan == MUL_PLAN_PLAIN ? run_lincomb2<Secp256k1, MUL_PLAN_PLAIN>(a, b, px, py, qx, qy, ox, oy, count, err)
                                  : run_lincomb2<Secp256k1, MUL_PLAN_GLV>(a, b, px, py, qx, qy, ox, oy, count, err);
}

// the three constant chaining values, 8 words each
extern "C" void emud_midstates(uint32_t* out24) {
    for (int t = 0; t < 3; t++) {
        const Sha256State s = dleq_midstate(t);
        for (int j = 0; j < 8; j++) out24[8 * t + j] = s.h[j];
    }
}
extern "C" long emud_prove(const uint8_t* a_sk32, const uint8_t* bx32, const uint8_t* by32, const uint8_t* aux_rand32, const uint8_t* msg32,
                           uint8_t* proof64, uint8_t* cx32, uint8_t* cy32, size_t count, uint8_t* err) {
    const Aff* T = gen_table();
    long bad = 0;
#pragma omp parallel for schedule(dynamic, 4) reduction(+ : bad)
    for (long long i = 0; i < (long long)count; i++) {
        err[i] = body_dleq_prove(T, a_sk32, bx32, by32, aux_rand32, msg32, proof64, cx32, cy32, (size_t)i);
        bad += err[i] != 0;
    }
    return bad;
}
extern "C" long emud_verify(const uint8_t* ax32, const uint8_t* ay32, const uint8_t* bx32, const uint8_t* by32, const uint8_t* cx32,
                            const uint8_t* cy32, const uint8_t* proof64, const uint8_t* msg32, size_t count, uint8_t* err, uint8_t* valid) {
    const Aff* T = gen_table();
    long bad = 0;
#pragma omp parallel for schedule(dynamic, 4) reduction(+ : bad)
    for (long long i = 0; i < (long long)count; i++) {
        err[i] = body_dleq_verify(T, ax32, ay32, bx32, by32, cx32, cy32, proof64, msg32, valid, (size_t)i);
        bad += err[i] != 0;
    }
    return bad;
}
// behind the nonce hash, with ANY k (32 big-endian bytes): code[i] and proof64 (zeros where the code is not 0).  The points are
// taken as given (A, B, C little-endian, already checked by the caller), a_sk32 little-endian.
extern "C" void emud_prove_with_nonce(const uint8_t* a_sk32, const uint8_t* ax32, const uint8_t* ay32, const uint8_t* bx32, const uint8_t* by32,
                                      const uint8_t* cx32, const uint8_t* cy32, const uint8_t* k32, const uint8_t* msg32, uint8_t* proof64,
                                      uint8_t* code, size_t count) {
    const Aff* T = gen_table();
    for (size_t i = 0; i < count; i++) {
        U256 e = u256_zero(), s = u256_zero();
        const U256 msg = msg32 ? schnorr_load_be(msg32 + 32 * i) : u256_zero();
        code[i] = dleq_prove_with_nonce(T, load_packed(a_sk32, i), load_aff(ax32, ay32, i), load_aff(bx32, by32, i), load_aff(cx32, cy32, i),
                                        schnorr_load_be(k32 + 32 * i), msg32 != nullptr, msg, e, s);
        if (code[i]) e = s = u256_zero();
        schnorr_store_be(proof64 + 64 * i, e);
        schnorr_store_be(proof64 + 64 * i + 32, s);
    }
}
// behind the challenge hash on the prover's side: s = k + e a mod n for ANY e (k, e, s big-endian; a little-endian)
extern "C" void emud_response(const uint8_t* k32, const uint8_t* e32, const uint8_t* a_sk32, uint8_t* s32, size_t count) {
    for (size_t i = 0; i < count; i++)
        schnorr_store_be(s32 + 32 * i, dleq_response(schnorr_load_be(k32 + 32 * i), schnorr_load_be(e32 + 32 * i), load_packed(a_sk32, i)));
}
// behind e on the verifier's side, with ANY e and any s < n (big-endian): ok[i] = neither point is neutral; R1, R2 little-endian
// (x, y), zeros where ok[i] is 0
extern "C" void emud_verify_points(const uint8_t* ax32, const uint8_t* ay32, const uint8_t* bx32, const uint8_t* by32, const uint8_t* cx32,
                                   const uint8_t* cy32, const uint8_t* e32, const uint8_t* s32, uint8_t* r1x32, uint8_t* r1y32, uint8_t* r2x32,
                                   uint8_t* r2y32, uint8_t* ok, size_t count) {
    const Aff* T = gen_table();
    for (size_t i = 0; i < count; i++) {
        Aff R1, R2;
        const bool good = dleq_verify_points(T, load_aff(ax32, ay32, i), load_aff(bx32, by32, i), load_aff(cx32, cy32, i),
                                             schnorr_load_be(e32 + 32 * i), schnorr_load_be(s32 + 32 * i), R1, R2);
        if (!good) R1.x = R1.y = R2.x = R2.y = u256_zero();
        ok[i] = good ? 1 : 0;
        store_packed(r1x32, i, R1.x), store_packed(r1y32, i, R1.y);
        store_packed(r2x32, i, R2.x), store_packed(r2y32, i, R2.y);
    }
}

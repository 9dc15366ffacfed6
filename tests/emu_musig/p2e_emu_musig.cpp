// CPU harness of the MuSig2 layer (test infrastructure only): the bodies of csrc/musig.hpp run per element, compiled with g++
// against the library's headers and the generator table the library uploads.
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../plonky2-ecdsa_amd/csrc/consts.hpp"
#include "../../plonky2-ecdsa_amd/csrc/musig.hpp"

using namespace p2e;

namespace {
const Aff* gen_table() { return host::consts().fbtab.data(); }
}  // namespace

// the three constant chaining values, 8 words each
extern "C" void emumusig_midstates(uint32_t* out24) {
    for (int t = 0; t < 3; t++) {
        const Sha256State s = musig_midstate(t);
        for (int j = 0; j < 8; j++) out24[8 * t + j] = s.h[j];
    }
}
// Key aggregation behind ANY coefficients: session i sums coef32[j] P_j (32 big-endian bytes each, reduced modulo n) over its
// keys, which must be valid.  code[i], and where it is 0 the point (little-endian x, y); zeros otherwise.
extern "C" void emumusig_forced_key_agg(const uint8_t* pkx32, const uint8_t* pky32, const uint8_t* coef32, const uint64_t* key_offsets,
                                        uint8_t* code, uint8_t* qx32, uint8_t* qy32, size_t count) {
    for (size_t i = 0; i < count; i++) {
        SignSum<MusigCV> sum = msm_neutral<MusigCV>();
        for (uint64_t j = key_offsets[i]; j < key_offsets[i + 1]; j++)
            sum = msm_add<MusigCV, false>(sum, musig_term(musig_load_point(pkx32, pky32, (size_t)j), fe_canon<MusigCV::Fn>(schnorr_load_be(coef32 + 32 * j))));
        MusigKeyAgg r;
        r.Q.x = r.Q.y = u256_zero();
        code[i] = musig_key_agg_finish(sum, r);
        hd_store_key(qx32, i, r.Q.x, code[i] != 0);
        hd_store_key(qy32, i, r.Q.y, code[i] != 0);
    }
}
// The session values behind ANY b (32 big-endian bytes, reduced modulo n); the other arguments as emumusig_session's, checked
// by the caller.  code[i] and session128.
extern "C" void emumusig_forced_session(const uint8_t* keyagg192, const uint8_t* aggnonce128, const uint8_t* msg32, const uint8_t* b32,
                                        uint8_t* code, uint8_t* session128, size_t count) {
    const Aff* T = gen_table();
    for (size_t i = 0; i < count; i++) {
        const MusigKeyAgg ka = musig_load_keyagg(keyagg192, i);
        const Aff R1 = musig_load_nonce(aggnonce128, i, 0), R2 = musig_load_nonce(aggnonce128, i, 1);
        const bool n1 = u256_is_zero(R1.x) && u256_is_zero(R1.y), n2 = u256_is_zero(R2.x) && u256_is_zero(R2.y);
        MusigSession r;
        r.b = r.e = r.rx = u256_zero();
        r.flags = 0;
        MusigParkHost park;
        code[i] = musig_session_finish(park, T, ka.Q.x, R1, n1, R2, n2, fe_canon<MusigCV::Fn>(schnorr_load_be(b32 + 32 * i)),
                                       schnorr_load_be(msg32 + 32 * i), r);
        musig_store_session(session128, i, r, code[i] != 0);
    }
}

extern "C" long emumusig_key_agg(const uint8_t* pkx32, const uint8_t* pky32, const uint64_t* key_offsets, uint8_t* keyagg192,
                                 uint8_t* agg_pk32, size_t count, uint8_t* err) {
    long bad = 0;
#pragma omp parallel for schedule(dynamic, 4) reduction(+ : bad)
    for (long long i = 0; i < (long long)count; i++) {
        MusigParkHost park;
        err[i] = body_musig_key_agg(park, pkx32, pky32, key_offsets, keyagg192, agg_pk32, (size_t)i);
        bad += err[i] != 0;
    }
    return bad;
}
extern "C" long emumusig_apply_tweak(const uint8_t* keyagg192_in, const uint8_t* tweak32, int mode, uint8_t* keyagg192_out,
                                     uint8_t* agg_pk32, size_t count, uint8_t* err) {
    if (mode < 0 || mode > 2 || (!tweak32 && mode != MUSIG_TWEAK_TAPROOT)) return -1;
    const Aff* T = gen_table();
    long bad = 0;
#pragma omp parallel for schedule(dynamic, 4) reduction(+ : bad)
    for (long long i = 0; i < (long long)count; i++) {
        err[i] = body_musig_apply_tweak(T, keyagg192_in, tweak32, mode, keyagg192_out, agg_pk32, (size_t)i);
        bad += err[i] != 0;
    }
    return bad;
}
extern "C" long emumusig_nonce_agg(const uint8_t* pubnonce128, const uint64_t* key_offsets, uint8_t* aggnonce128, size_t count,
                                   uint8_t* err) {
    long bad = 0;
#pragma omp parallel for schedule(dynamic, 4) reduction(+ : bad)
    for (long long i = 0; i < (long long)count; i++) {
        err[i] = body_musig_nonce_agg(pubnonce128, key_offsets, aggnonce128, (size_t)i);
        bad += err[i] != 0;
    }
    return bad;
}
extern "C" long emumusig_session(const uint8_t* keyagg192, const uint8_t* aggnonce128, const uint8_t* msg32, uint8_t* session128,
                                 size_t count, uint8_t* err) {
    const Aff* T = gen_table();
    long bad = 0;
#pragma omp parallel for schedule(dynamic, 4) reduction(+ : bad)
    for (long long i = 0; i < (long long)count; i++) {
        MusigParkHost park;
        err[i] = body_musig_session(park, T, keyagg192, aggnonce128, msg32, session128, (size_t)i);
        bad += err[i] != 0;
    }
    return bad;
}
extern "C" long emumusig_partial_sign(const uint8_t* secnonce64, const uint8_t* sk32, const uint8_t* keyagg192, const uint8_t* session128,
                                      uint8_t* psig32, size_t count, uint8_t* err) {
    const Aff* T = gen_table();
    long bad = 0;
#pragma omp parallel for schedule(dynamic, 4) reduction(+ : bad)
    for (long long i = 0; i < (long long)count; i++) {
        err[i] = body_musig_partial_sign(T, secnonce64, sk32, keyagg192, session128, psig32, (size_t)i);
        bad += err[i] != 0;
    }
    return bad;
}
extern "C" long emumusig_partial_verify(const uint8_t* psig32, const uint8_t* pubnonce128, const uint8_t* pkx32, const uint8_t* pky32,
                                        const uint32_t* session_index, const uint8_t* keyagg192, const uint8_t* session128,
                                        size_t n_sessions, size_t count, uint8_t* err, uint8_t* valid) {
    const Aff* T = gen_table();
    long bad = 0;
#pragma omp parallel for schedule(dynamic, 4) reduction(+ : bad)
    for (long long i = 0; i < (long long)count; i++) {
        MusigParkHost park;
        err[i] = body_musig_partial_verify(park, T, psig32, pubnonce128, pkx32, pky32, session_index, keyagg192, session128, n_sessions, valid,
                                           (size_t)i);
        bad += err[i] != 0;
    }
    return bad;
}
extern "C" long emumusig_sig_agg(const uint8_t* psig32, const uint64_t* key_offsets, const uint8_t* keyagg192, const uint8_t* session128,
                                 uint8_t* sig64, size_t count, uint8_t* err) {
    long bad = 0;
#pragma omp parallel for schedule(dynamic, 16) reduction(+ : bad)
    for (long long i = 0; i < (long long)count; i++) {
        err[i] = body_musig_sig_agg(psig32, key_offsets, keyagg192, session128, sig64, (size_t)i);
        bad += err[i] != 0;
    }
    return bad;
}

// CPU harness of the Taproot layer (test infrastructure only): the bodies of csrc/taproot.hpp run per element, compiled with
// g++ against the library's headers and the generator table the library uploads.
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../plonky2-ecdsa_amd/csrc/consts.hpp"
#include "../../plonky2-ecdsa_amd/csrc/taproot.hpp"

using namespace p2e;

namespace {
const Aff* gen_table() { return host::consts().fbtab.data(); }
U256 be256(const uint8_t* p) {
    U256 r;
    for (int j = 0; j < 8; j++) r.w[7 - j] = ((u32)p[4 * j] << 24) | ((u32)p[4 * j + 1] << 16) | ((u32)p[4 * j + 2] << 8) | (u32)p[4 * j + 3];
    return r;
}
void put_be256(uint8_t* p, const U256& v) {
    for (int j = 0; j < 32; j++) p[j] = (uint8_t)(v.w[7 - j / 4] >> (8 * (3 - j % 4)));
}
}  // namespace

// the three constant chaining values, 8 words each
extern "C" void emutr_midstates(uint32_t* out24) {
    for (int t = 0; t < 3; t++) {
        const Sha256State s = taproot_midstate(t);
        for (int j = 0; j < 8; j++) out24[8 * t + j] = s.h[j];
    }
}
// SHA-256(prefix || data[lo, hi)) from the IV: the prefixed absorption alone (prefix_len <= 8)
extern "C" void emutr_sha256_prefixed(const uint8_t* prefix, unsigned prefix_len, const uint8_t* data, uint64_t lo, uint64_t hi, uint8_t* out32) {
    ShaPrefix px;
    px.w[0] = px.w[1] = 0;
    px.len = prefix_len;
    for (unsigned k = 0; k < prefix_len; k++) px.w[k / 4] |= (u32)prefix[k] << (8 * (3 - k % 4));
    const uint64_t offsets[2] = {lo, hi};
    bool bad;
    const Sha256State s = sha256_prefixed_message(sha256_iv(), 0, px, msg_view(data, offsets, 0, &bad));
    for (int j = 0; j < 32; j++) out32[j] = (uint8_t)(s.h[j / 4] >> (8 * (3 - j % 4)));
}
// the arithmetic behind the hash with ANY t (32-byte big-endian values); outputs are written only where the code is 0
extern "C" int emutr_finish_pub(const uint8_t* pk32, const uint8_t* t32, uint8_t* out32, uint8_t* parity) {
    Aff P;
    if (schnorr_lift_x(be256(pk32), false, P)) return -1;
    U256 qx = u256_zero();
    u32 par = 0;
    const uint8_t e = taproot_finish_pub(gen_table(), P, be256(t32), qx, par);
    if (!e) put_be256(out32, qx), *parity = (uint8_t)par;
    return e;
}
extern "C" int emutr_finish_sec(const uint8_t* d32, const uint8_t* t32, uint8_t* out32) {
    U256 out = u256_zero();
    const uint8_t e = taproot_finish_sec(be256(d32), be256(t32), out);
    if (!e) put_be256(out32, out);
    return e;
}

extern "C" long emutr_leaf_hash(const uint8_t* leaf_version, const uint8_t* script, const uint64_t* offsets, uint8_t* leaf32, size_t count,
                                uint8_t* err) {
    long bad = 0;
#pragma omp parallel for schedule(dynamic, 1) reduction(+ : bad)
    for (long long i = 0; i < (long long)count; i++) {
        err[i] = body_taproot_leaf_hash(leaf_version, script, offsets, leaf32, (size_t)i);
        bad += err[i] != 0;
    }
    return bad;
}
extern "C" long emutr_merkle_root(const uint8_t* leaf32, const uint8_t* path32, const uint8_t* depth, size_t max_depth, uint8_t* root32,
                                  size_t count, uint8_t* err) {
    long bad = 0;
#pragma omp parallel for schedule(dynamic, 16) reduction(+ : bad)
    for (long long i = 0; i < (long long)count; i++) {
        err[i] = body_taproot_merkle_root(leaf32, path32, depth, max_depth, root32, (size_t)i);
        bad += err[i] != 0;
    }
    return bad;
}
extern "C" long emutr_tweak_pubkey(const uint8_t* pk32, const uint8_t* root32, uint8_t* out_pk32, uint8_t* out_parity, size_t count,
                                   uint8_t* err) {
    const Aff* T = gen_table();
    long bad = 0;
#pragma omp parallel for schedule(dynamic, 16) reduction(+ : bad)
    for (long long i = 0; i < (long long)count; i++) {
        err[i] = body_taproot_tweak_pubkey(T, pk32, root32, out_pk32, out_parity, (size_t)i);
        bad += err[i] != 0;
    }
    return bad;
}
extern "C" long emutr_tweak_seckey(const uint8_t* sk32, const uint8_t* root32, uint8_t* out_sk32, size_t count, uint8_t* err) {
    const Aff* T = gen_table();
    long bad = 0;
#pragma omp parallel for schedule(dynamic, 16) reduction(+ : bad)
    for (long long i = 0; i < (long long)count; i++) {
        err[i] = body_taproot_tweak_seckey(T, sk32, root32, out_sk32, (size_t)i);
        bad += err[i] != 0;
    }
    return bad;
}
extern "C" long emutr_verify_commitment(const uint8_t* out_pk32, const uint8_t* out_parity, const uint8_t* pk32, const uint8_t* leaf32,
                                        const uint8_t* path32, const uint8_t* depth, size_t max_depth, size_t count, uint8_t* err,
                                        uint8_t* valid) {
    const Aff* T = gen_table();
    long bad = 0;
#pragma omp parallel for schedule(dynamic, 16) reduction(+ : bad)
    for (long long i = 0; i < (long long)count; i++) {
        err[i] = body_taproot_verify_commitment(T, out_pk32, out_parity, pk32, leaf32, path32, depth, max_depth, valid, (size_t)i);
        bad += err[i] != 0;
    }
    return bad;
}

// CPU harness of the hashing, nonce and address kernel bodies (test infrastructure only): body_hash, body_nonce and
// body_eth_address of csrc/hash.hpp run per element, compiled with g++ against the library's header, plus the nonce
// generator with the order as an argument (the form the retry tests use).
#include <cstdint>

#include "../../plonky2-ecdsa_amd/csrc/hash.hpp"

using namespace p2e;

extern "C" long emuh_hash(int alg, unsigned form, const uint8_t* data, const uint64_t* offsets, uint8_t* out32, size_t n) {
    if (alg < 0 || alg > 2 || form > 1) return -1;
    long bad = 0;
#pragma omp parallel for schedule(dynamic, 64) reduction(+ : bad)
    for (long long i = 0; i < (long long)n; i++) {
        if (alg == HASH_SHA256) bad += body_hash<HASH_SHA256>(data, offsets, out32, (size_t)i, form);
        if (alg == HASH_SHA256D) bad += body_hash<HASH_SHA256D>(data, offsets, out32, (size_t)i, form);
        if (alg == HASH_KECCAK256) bad += body_hash<HASH_KECCAK256>(data, offsets, out32, (size_t)i, form);
    }
    return bad;
}
extern "C" long emuh_nonce(int curve, const uint8_t* msg32, const uint8_t* sk32, uint8_t* k32, size_t n) {
    if (curve != 0 && curve != 1) return -1;
#pragma omp parallel for schedule(dynamic, 16)
    for (long long i = 0; i < (long long)n; i++) {
        if (curve == 0)
            body_nonce<ModN>(msg32, sk32, k32, (size_t)i);
        else
            body_nonce<ModN256>(msg32, sk32, k32, (size_t)i);
    }
    return 0;
}
// rfc6979_nonce(q, x, z) with q, x, z as given (x < q is the caller's); rejected[i] = candidates refused
extern "C" long emuh_nonce_order(const uint8_t* q32, const uint8_t* x32, const uint8_t* z32, uint8_t* k32, uint32_t* rejected, size_t n) {
    const U256 q = hash_load_packed(q32, 0);
    for (size_t i = 0; i < n; i++)
        hash_store_packed(k32, i, rfc6979_nonce(q, hash_load_packed(x32, i), hash_load_packed(z32, i), &rejected[i]));
    return 0;
}
extern "C" long emuh_eth_address(const uint8_t* pkx32, const uint8_t* pky32, const uint8_t* err, uint8_t* addr20, size_t n) {
    for (size_t i = 0; i < n; i++) body_eth_address(pkx32, pky32, err, addr20, i);
    return 0;
}

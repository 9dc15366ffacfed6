/* Minimal C client of the native front end on the device (include/p2e.h): derive public keys, sign, and hand the result
 * to the verdict-only verifier -- curve/ecdsa.rs to_public, sign_message (the nonce is an input) and verify_message.
 *     gcc -std=c11 -Iinclude examples/sign_verify.c -Lplonky2-ecdsa_amd -lp2e_hip -o sign_verify
 *     GPU_MAX_HW_QUEUES=8 LD_LIBRARY_PATH=plonky2-ecdsa_amd:/opt/rocm/lib ./sign_verify 512
 * Keys, messages and nonces come from a toy generator here: a real caller brings its own (RFC 6979 or an RNG for the
 * nonce -- it must never repeat). */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "p2e.h"

static uint64_t next64(uint64_t *s) {   /* splitmix64 */
    uint64_t z = (*s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

int main(int argc, char **argv) {
    size_t n = argc > 1 ? (size_t)strtoull(argv[1], NULL, 10) : 128;
    uint8_t *sk = malloc(32 * n), *msg = malloc(32 * n), *k = malloc(32 * n);
    uint8_t *pkx = malloc(32 * n), *pky = malloc(32 * n), *r = malloc(32 * n), *s = malloc(32 * n);
    uint8_t *err = malloc(n), *valid = malloc(n);
    uint64_t seed = 2024;
    for (size_t i = 0; i < 32 * n; i++) {   /* any 32 bytes are a scalar: the calls take them modulo the group order */
        sk[i] = (uint8_t)next64(&seed);
        msg[i] = (uint8_t)next64(&seed);
        k[i] = (uint8_t)next64(&seed);
    }
    p2e_ctx *ctx = NULL;
    if (p2e_ctx_create(0, P2E_CTX_HOST_POINTERS, NULL, &ctx)) {
        fprintf(stderr, "p2e_ctx_create: %s\n", p2e_last_error());   /* no GPU: there is no CPU fallback */
        return 2;
    }
    long bad_pk = p2e_ecdsa_public_key_batch(ctx, P2E_CURVE_SECP256K1, P2E_SIGN_PLAN_AUTO, sk, pkx, pky, n, err);
    long bad_sig = p2e_ecdsa_sign_batch(ctx, P2E_CURVE_SECP256K1, P2E_SIGN_PLAN_AUTO, msg, sk, k, r, s, n, err);
    if (bad_pk < 0 || bad_sig < 0) {
        fprintf(stderr, "p2e: %s\n", p2e_last_error());
        return 3;
    }
    if (n > 1) msg[32 * (n / 2)] ^= 1;   /* one tampered message: it must be the only signature that does not verify */
    long bad_v = p2e_ecdsa_verify_batch(ctx, msg, r, s, pkx, pky, n, err, valid);
    if (bad_v < 0) {
        fprintf(stderr, "p2e: %s\n", p2e_last_error());
        return 4;
    }
    size_t verified = 0;
    for (size_t i = 0; i < n; i++) verified += valid[i];
    printf("%zu keys (%ld flagged), %zu signatures (%ld flagged), %zu verify, %ld flagged by the verifier\n", n, bad_pk, n, bad_sig,
           verified, bad_v);
    p2e_ctx_destroy(ctx);
    free(sk), free(msg), free(k), free(pkx), free(pky), free(r), free(s), free(err), free(valid);
    return (bad_pk == 0 && bad_sig == 0 && bad_v == 0 && verified == n - (n > 1 ? 1 : 0)) ? 0 : 1;
}

/* Minimal C client of the DLEQ calls (include/p2e.h p2e_dleq_prove_batch, p2e_dleq_verify_batch): a collaborative
 * silent-payment sender.  Derive the signers' public keys A = a G and the receivers' scan keys B = b G on the device, publish
 * each ECDH share C = a B with its BIP-374 proof, verify every proof (the step the prover itself leaves out: the two calls are
 * chained here), then flip ONE bit of one proof and see exactly that element rejected.  Device buffers throughout; keys and
 * points are the library's little-endian values, the proof is the standard's big-endian e || s.
 *     gcc -std=c11 -Iinclude examples/dleq_share.c -Lplonky2-ecdsa_amd -lp2e_hip -L/opt/rocm/lib -lamdhip64 -o dleq_share
 *     GPU_MAX_HW_QUEUES=8 LD_LIBRARY_PATH=plonky2-ecdsa_amd:/opt/rocm/lib ./dleq_share 1000
 * aux_rand32 must come from the system's random source in a real signer; this demonstration uses a counter.
 * The three HIP runtime calls a C client needs are declared here, so that no HIP header (C++) is required. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "p2e.h"

extern int hipMalloc(void **ptr, size_t size);
extern int hipFree(void *ptr);
extern int hipMemcpy(void *dst, const void *src, size_t size, int kind);   /* 1 = host to device, 2 = device to host */

static uint64_t next64(uint64_t *s) {   /* splitmix64 */
    uint64_t z = (*s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

int main(int argc, char **argv) {
    size_t n = argc > 1 ? (size_t)strtoull(argv[1], NULL, 10) : 1000;
    if (n < 2) n = 2;
    /* host: a, b (little-endian; the top byte is cleared so that 0 < key < the group order), aux, msg: 32 n each */
    uint8_t *host = malloc(128 * n), *valid = malloc(n);
    uint64_t rng = 374;
    for (size_t at = 0; at < 128 * n; at += 8) {
        uint64_t v = next64(&rng);
        memcpy(host + at, &v, 8);
    }
    for (size_t i = 0; i < 2 * n; i++) host[32 * i + 31] = 0, host[32 * i] |= 1;
    p2e_ctx *ctx = NULL;
    if (p2e_ctx_create(0, 0, NULL, &ctx)) {
        fprintf(stderr, "p2e_ctx_create: %s\n", p2e_last_error());   /* no GPU: there is no CPU fallback */
        return 2;
    }
    uint8_t *dev = NULL;   /* a, b, aux, msg | A, B, C (64 n each), proof (64 n), err (n), valid (n) */
    if (hipMalloc((void **)&dev, 128 * n + 3 * 64 * n + 64 * n + 2 * n) || hipMemcpy(dev, host, 128 * n, 1)) {
        fprintf(stderr, "device allocation or upload failed\n");
        return 2;
    }
    uint8_t *a = dev, *b = dev + 32 * n, *aux = dev + 64 * n, *msg = dev + 96 * n;
    uint8_t *ax = dev + 128 * n, *ay = ax + 32 * n, *bx = ay + 32 * n, *by = bx + 32 * n, *cx = by + 32 * n, *cy = cx + 32 * n;
    uint8_t *proof = cy + 32 * n, *err = proof + 64 * n, *ok = err + n;
    long bad_a = p2e_ecdsa_public_key_batch(ctx, P2E_CURVE_SECP256K1, P2E_SIGN_PLAN_AUTO, a, ax, ay, n, err);
    long bad_b = p2e_ecdsa_public_key_batch(ctx, P2E_CURVE_SECP256K1, P2E_SIGN_PLAN_AUTO, b, bx, by, n, err);
    long bad_prove = p2e_dleq_prove_batch(ctx, a, bx, by, aux, msg, proof, cx, cy, n, err);
    long bad_verify = p2e_dleq_verify_batch(ctx, ax, ay, bx, by, cx, cy, proof, msg, n, err, ok);
    if (bad_a < 0 || bad_b < 0 || bad_prove < 0 || bad_verify < 0) {
        fprintf(stderr, "p2e: %s\n", p2e_last_error());
        return 3;
    }
    if (hipMemcpy(valid, ok, n, 2)) return 4;
    size_t accepted = 0;
    for (size_t i = 0; i < n; i++) accepted += valid[i] == 1;
    /* one flipped bit in the e half of one proof */
    size_t victim = n / 2;
    uint8_t byte;
    if (hipMemcpy(&byte, proof + 64 * victim + 17, 1, 2)) return 4;
    byte ^= 4;
    if (hipMemcpy(proof + 64 * victim + 17, &byte, 1, 1)) return 4;
    long bad_verify2 = p2e_dleq_verify_batch(ctx, ax, ay, bx, by, cx, cy, proof, msg, n, err, ok);
    if (bad_verify2 < 0) {
        fprintf(stderr, "p2e: %s\n", p2e_last_error());
        return 3;
    }
    if (hipMemcpy(valid, ok, n, 2)) return 4;
    size_t still = 0, where = n;
    for (size_t i = 0; i < n; i++) {
        still += valid[i] == 1;
        if (valid[i] != 1) where = i;
    }
    printf("%zu shares proven (%ld refused), %zu proofs valid; with one bit flipped in proof %zu: %zu valid\n", n, bad_prove, accepted, victim,
           still);
    int good = bad_a == 0 && bad_b == 0 && bad_prove == 0 && bad_verify == 0 && bad_verify2 == 0 && accepted == n && still == n - 1 &&
               where == victim;
    p2e_ctx_destroy(ctx);
    hipFree(dev);
    free(host);
    free(valid);
    return good ? 0 : 1;
}

/* Minimal C client of the BIP-340 calls (include/p2e.h p2e_schnorr_public_key_batch and the calls after it): derive x-only
 * keys and sign a batch on the device, verify it per element and in aggregate, then corrupt ONE signature and see the
 * aggregate verdict turn 0 and the per-element call name the element.  Device buffers throughout; every value is the
 * standard's big-endian byte string.
 *     gcc -std=c11 -Iinclude examples/schnorr_verify.c -Lplonky2-ecdsa_amd -lp2e_hip -L/opt/rocm/lib -lamdhip64 -o schnorr_verify
 *     GPU_MAX_HW_QUEUES=8 LD_LIBRARY_PATH=plonky2-ecdsa_amd:/opt/rocm/lib ./schnorr_verify 1000
 * The seed of the aggregate check must be unpredictable to whoever made the signatures.  A real caller draws it from the
 * system's random source or hashes the whole batch; this demonstration, which signs its own batch, uses a counter.
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
    if (n < 1) n = 1;
    /* host: msg, sk, aux (32 n each) and the seed; sk's top byte is cleared so that 0 < sk < the group order */
    uint8_t *host = malloc(96 * n + 32), *valid = malloc(n), verdict[2] = {0xFF, 0xFF};
    uint64_t rng = 340;
    for (size_t b = 0; b < 96 * n + 32; b += 8) {
        uint64_t v = next64(&rng);
        memcpy(host + b, &v, 8);
    }
    for (size_t i = 0; i < n; i++) host[32 * n + 32 * i] = 0, host[32 * n + 32 * i + 31] |= 1;
    p2e_ctx *ctx = NULL;
    if (p2e_ctx_create(0, 0, NULL, &ctx)) {
        fprintf(stderr, "p2e_ctx_create: %s\n", p2e_last_error());   /* no GPU: there is no CPU fallback */
        return 2;
    }
    uint8_t *dev = NULL;   /* msg, sk, aux, seed | pk (32 n), sig (64 n), err (n), valid (n), two verdict bytes */
    if (hipMalloc((void **)&dev, 96 * n + 32 + 98 * n + 8) || hipMemcpy(dev, host, 96 * n + 32, 1)) {
        fprintf(stderr, "device allocation or upload failed\n");
        return 2;
    }
    uint8_t *msg = dev, *sk = dev + 32 * n, *aux = dev + 64 * n, *seed = dev + 96 * n, *pk = seed + 32, *sig = pk + 32 * n;
    uint8_t *err = sig + 64 * n, *ok = err + n, *verd = ok + n;
    long bad_pk = p2e_schnorr_public_key_batch(ctx, sk, pk, n, err);
    long bad_sign = p2e_schnorr_sign_batch(ctx, msg, sk, aux, sig, n, err);
    long bad_verify = p2e_schnorr_verify_batch(ctx, msg, pk, sig, n, err, ok);
    long bad_agg = p2e_schnorr_verify_aggregate(ctx, msg, pk, sig, n, seed, P2E_MSM_WINDOW_AUTO, verd, NULL);
    if (bad_pk < 0 || bad_sign < 0 || bad_verify < 0 || bad_agg < 0) {
        fprintf(stderr, "p2e: %s\n", p2e_last_error());
        return 3;
    }
    if (hipMemcpy(valid, ok, n, 2)) return 4;
    size_t accepted = 0;
    for (size_t i = 0; i < n; i++) accepted += valid[i] == 1;
    /* one flipped bit in the s half of one signature */
    size_t victim = n / 2;
    uint8_t byte;
    if (hipMemcpy(&byte, sig + 64 * victim + 63, 1, 2)) return 4;
    byte ^= 1;
    if (hipMemcpy(sig + 64 * victim + 63, &byte, 1, 1)) return 4;
    long bad_agg2 = p2e_schnorr_verify_aggregate(ctx, msg, pk, sig, n, seed, P2E_MSM_WINDOW_AUTO, verd + 1, NULL);
    long bad_verify2 = p2e_schnorr_verify_batch(ctx, msg, pk, sig, n, err, ok);
    if (bad_agg2 < 0 || bad_verify2 < 0) {
        fprintf(stderr, "p2e: %s\n", p2e_last_error());
        return 3;
    }
    if (hipMemcpy(verdict, verd, 2, 2) || hipMemcpy(valid, ok, n, 2)) return 4;
    size_t rejected = 0, where = n;
    for (size_t i = 0; i < n; i++)
        if (valid[i] != 1) rejected++, where = i;
    printf("%zu signatures: %zu accepted one by one, aggregate verdict %d; after one flipped bit: aggregate verdict %d, "
           "%zu rejected one by one (element %zu, the corrupted one is %zu)\n",
           n, accepted, verdict[0], verdict[1], rejected, where, victim);
    int good = bad_pk == 0 && bad_sign == 0 && bad_verify == 0 && bad_agg == 0 && accepted == n && verdict[0] == 1 && verdict[1] == 0 &&
               rejected == 1 && where == victim;
    p2e_ctx_destroy(ctx);
    hipFree(dev);
    free(host);
    free(valid);
    return good ? 0 : 1;
}

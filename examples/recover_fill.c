/* Minimal C client of the recovery path (include/p2e.h): sign recoverably on the device, recover the public keys from
 * (msg, r, s, v), and feed them to the verdict-only verifier -- the input of the witness fill made from a batch that
 * carries no public key.  Device buffers throughout: nothing crosses to the host between the three calls.
 *     gcc -std=c11 -Iinclude examples/recover_fill.c -Lplonky2-ecdsa_amd -lp2e_hip -L/opt/rocm/lib -lamdhip64 -o recover_fill
 *     GPU_MAX_HW_QUEUES=8 LD_LIBRARY_PATH=plonky2-ecdsa_amd:/opt/rocm/lib ./recover_fill 512
 * The three HIP runtime calls a C client needs are declared here, so that no HIP header (C++) is required.
 * Ethereum's v is 27 + this library's v (or the EIP-155 form 35 + 2 chain_id + v): subtract the offset first. */
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
    size_t n = argc > 1 ? (size_t)strtoull(argv[1], NULL, 10) : 128;
    uint8_t *host = malloc(3 * 32 * n), *valid = malloc(n), *pk_host = malloc(2 * 32 * n), *pk_want = malloc(2 * 32 * n);
    uint64_t seed = 2025;
    for (size_t i = 0; i < 3 * 32 * n; i++) host[i] = (uint8_t)next64(&seed);   /* msg | sk | k: any 32 bytes are a scalar */
    p2e_ctx *ctx = NULL;
    if (p2e_ctx_create(0, 0, NULL, &ctx)) {
        fprintf(stderr, "p2e_ctx_create: %s\n", p2e_last_error());   /* no GPU: there is no CPU fallback */
        return 2;
    }
    uint8_t *dev = NULL;   /* msg, sk, k, r, s, pkx, pky, wantx, wanty (32 n each), v, err, valid (n each) */
    if (hipMalloc((void **)&dev, (9 * 32 + 3) * n) || hipMemcpy(dev, host, 3 * 32 * n, 1)) {
        fprintf(stderr, "device allocation or upload failed\n");
        return 2;
    }
    uint8_t *msg = dev, *sk = dev + 32 * n, *k = dev + 64 * n, *r = dev + 96 * n, *s = dev + 128 * n, *pkx = dev + 160 * n;
    uint8_t *pky = dev + 192 * n, *wantx = dev + 224 * n, *v = dev + 288 * n, *err = v + n, *dvalid = err + n;
    long bad_sig = p2e_ecdsa_sign_recoverable_batch(ctx, P2E_CURVE_SECP256K1, P2E_SIGN_PLAN_AUTO, msg, sk, k, r, s, v, n, err);
    long bad_rec = p2e_ecdsa_recover_batch(ctx, P2E_CURVE_SECP256K1, msg, r, s, v, pkx, pky, n, err);
    long bad_ver = p2e_ecdsa_verify_batch(ctx, msg, r, s, pkx, pky, n, err, dvalid);
    /* for the report only: the keys the signer's secrets derive, to compare on the host */
    long bad_pk = p2e_ecdsa_public_key_batch(ctx, P2E_CURVE_SECP256K1, P2E_SIGN_PLAN_AUTO, sk, wantx, wantx + 32 * n, n, err);
    if (bad_sig < 0 || bad_rec < 0 || bad_ver < 0 || bad_pk < 0) {
        fprintf(stderr, "p2e: %s\n", p2e_last_error());
        return 3;
    }
    if (hipMemcpy(valid, dvalid, n, 2) || hipMemcpy(pk_host, pkx, 2 * 32 * n, 2) || hipMemcpy(pk_want, wantx, 2 * 32 * n, 2)) return 4;
    size_t verified = 0;
    for (size_t i = 0; i < n; i++) verified += valid[i];
    int same = memcmp(pk_host, pk_want, 2 * 32 * n) == 0;
    printf("%zu signatures (%ld flagged), %zu keys recovered (%ld flagged), %zu verify (%ld flagged), recovered keys %s sk G\n", n,
           bad_sig, n, bad_rec, verified, bad_ver, same ? "equal" : "DIFFER FROM");
    p2e_ctx_destroy(ctx);
    hipFree(dev);
    free(host), free(valid), free(pk_host), free(pk_want);
    return (bad_sig == 0 && bad_rec == 0 && bad_ver == 0 && bad_pk == 0 && verified == n && same) ? 0 : 1;
}

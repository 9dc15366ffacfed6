/* Minimal C client of the many-point sum (include/p2e.h p2e_point_msm): derive a batch of public keys on the device, sum
 * them with scalars by the bucket method, and compare with the public key of the summed scalar --
 *     sum_i k_i (sk_i G) = (sum_i k_i sk_i) G.
 * Device buffers throughout: the keys never visit the host.  The secret keys and the scalars are kept below 2^32 here so
 * that the host can form sum k_i sk_i (below 2^96 for any batch the call takes) without modular arithmetic; the library
 * takes any 32 bytes.
 *     gcc -std=c11 -Iinclude examples/msm_sum.c -Lplonky2-ecdsa_amd -lp2e_hip -L/opt/rocm/lib -lamdhip64 -o msm_sum
 *     GPU_MAX_HW_QUEUES=8 LD_LIBRARY_PATH=plonky2-ecdsa_amd:/opt/rocm/lib ./msm_sum 1000
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
static void put_le(uint8_t *dst, uint64_t lo, uint64_t hi) {   /* 32 little-endian bytes */
    memset(dst, 0, 32);
    for (int b = 0; b < 8; b++) dst[b] = (uint8_t)(lo >> (8 * b)), dst[8 + b] = (uint8_t)(hi >> (8 * b));
}

int main(int argc, char **argv) {
    size_t n = argc > 1 ? (size_t)strtoull(argv[1], NULL, 10) : 1000;
    int failures = 0;
    for (int curve = P2E_CURVE_SECP256K1; curve <= P2E_CURVE_P256; curve++) {
        uint8_t *host = malloc(2 * 32 * n + 32), sum32[32], got[64], want[64], status = 0xFF, err1 = 0xFF;
        uint64_t seed = 2026 + (uint64_t)curve, lo = 0, hi = 0;
        for (size_t i = 0; i < n; i++) {
            uint64_t sk = 1 + (next64(&seed) >> 33), k = next64(&seed) >> 32, prod = sk * k;
            put_le(host + 32 * i, sk, 0);
            put_le(host + 32 * (n + i), k, 0);
            lo += prod;
            hi += lo < prod;
        }
        put_le(sum32, lo, hi);
        p2e_ctx *ctx = NULL;
        if (p2e_ctx_create(0, 0, NULL, &ctx)) {
            fprintf(stderr, "p2e_ctx_create: %s\n", p2e_last_error());   /* no GPU: there is no CPU fallback */
            return 2;
        }
        uint8_t *dev = NULL;   /* sk, k, pkx, pky (32 n each), sum, out x | y, want x | y (32 each), err (n), status, err1 */
        if (hipMalloc((void **)&dev, (4 * 32 + 1) * n + 5 * 32 + 8) || hipMemcpy(dev, host, 2 * 32 * n, 1) ||
            hipMemcpy(dev + 128 * n, sum32, 32, 1)) {
            fprintf(stderr, "device allocation or upload failed\n");
            return 2;
        }
        uint8_t *sk = dev, *k = dev + 32 * n, *pkx = dev + 64 * n, *pky = dev + 96 * n, *sum = dev + 128 * n, *out = sum + 32;
        uint8_t *wantd = out + 64, *err = wantd + 64, *st = err + n;
        long bad_pk = p2e_ecdsa_public_key_batch(ctx, curve, P2E_SIGN_PLAN_AUTO, sk, pkx, pky, n, err);
        long bad_msm = p2e_point_msm(ctx, curve, P2E_MSM_WINDOW_AUTO, k, pkx, pky, n, out, out + 32, st, NULL);
        long bad_want = p2e_ecdsa_public_key_batch(ctx, curve, P2E_SIGN_PLAN_AUTO, sum, wantd, wantd + 32, 1, st + 1);
        if (bad_pk < 0 || bad_msm < 0 || bad_want < 0) {
            fprintf(stderr, "p2e: %s\n", p2e_last_error());
            return 3;
        }
        if (hipMemcpy(got, out, 64, 2) || hipMemcpy(want, wantd, 64, 2) || hipMemcpy(&status, st, 1, 2) || hipMemcpy(&err1, st + 1, 1, 2)) return 4;
        /* sum = 0 (every k zero: not with these seeds) would be P2E_MSM_NEUTRAL against P2E_ERR_POINT_AT_INFINITY */
        int same = memcmp(got, want, 64) == 0 && status == (err1 ? P2E_MSM_NEUTRAL : P2E_MSM_OK);
        uint64_t plan[P2E_MSM_PLAN_WORDS];
        if (p2e_point_msm_plan(curve, n, P2E_MSM_WINDOW_AUTO, plan)) return 5;
        printf("curve %d: %zu keys (%ld flagged) summed at %u-bit windows (status %d, %ld rejected): the sum %s the key of the summed scalar\n",
               curve, n, bad_pk, (unsigned)plan[P2E_MSM_PLAN_WINDOW_BITS], status, bad_msm, same ? "equals" : "DIFFERS FROM");
        failures += !(bad_pk == 0 && bad_msm == 0 && same);
        p2e_ctx_destroy(ctx);
        hipFree(dev);
        free(host);
    }
    return failures ? 1 : 0;
}

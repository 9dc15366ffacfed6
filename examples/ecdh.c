/* Minimal C client of the per-element point arithmetic (include/p2e.h p2e_point_mul_batch): ECDH on the device.  Two batches
 * of secret keys a_i and b_i are expanded to public keys A_i = a_i G and B_i = b_i G by p2e_ecdsa_public_key_batch; each side
 * multiplies the other's public key by its own secret, and the shared secrets must agree,
 *     a_i (b_i G) = b_i (a_i G),
 * which the program counts.  Device buffers throughout: neither the keys nor the shared secrets visit the host except for the
 * final comparison.  On secp256k1 one side walks with P2E_MUL_PLAN_PLAIN and the other with P2E_MUL_PLAN_GLV: all plans give
 * the same bytes.
 *     gcc -std=c11 -Iinclude examples/ecdh.c -Lplonky2-ecdsa_amd -lp2e_hip -L/opt/rocm/lib -lamdhip64 -o ecdh
 *     GPU_MAX_HW_QUEUES=8 LD_LIBRARY_PATH=plonky2-ecdsa_amd:/opt/rocm/lib ./ecdh 1000
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
    int failures = 0;
    if (n == 0) return 0;
    for (int curve = P2E_CURVE_SECP256K1; curve <= P2E_CURVE_P256; curve++) {
        uint8_t *host = malloc(4 * 32 * n);   /* the two secret-key batches; later the two batches of shared secrets (x | y) */
        uint64_t seed = 2027 + (uint64_t)curve;
        for (size_t i = 0; i < 2 * 32 * n; i += 8) {   /* any 32 bytes are a key: the library takes them modulo n */
            uint64_t w = next64(&seed);
            memcpy(host + i, &w, 8);
        }
        p2e_ctx *ctx = NULL;
        if (p2e_ctx_create(0, 0, NULL, &ctx)) {
            fprintf(stderr, "p2e_ctx_create: %s\n", p2e_last_error());   /* no GPU: there is no CPU fallback */
            return 2;
        }
        uint8_t *dev = NULL;   /* a, b, Ax, Ay, Bx, By, Sx, Sy, Tx, Ty (32 n each), err (n) */
        if (hipMalloc((void **)&dev, (10 * 32 + 1) * n) || hipMemcpy(dev, host, 2 * 32 * n, 1)) {
            fprintf(stderr, "device allocation or upload failed\n");
            return 2;
        }
        uint8_t *a = dev, *b = a + 32 * n, *ax = b + 32 * n, *ay = ax + 32 * n, *bx = ay + 32 * n, *by = bx + 32 * n;
        uint8_t *sx = by + 32 * n, *sy = sx + 32 * n, *tx = sy + 32 * n, *ty = tx + 32 * n, *err = ty + 32 * n;
        unsigned other = curve == P2E_CURVE_SECP256K1 ? P2E_MUL_PLAN_GLV : P2E_MUL_PLAN_AUTO;
        long bad_a = p2e_ecdsa_public_key_batch(ctx, curve, P2E_SIGN_PLAN_AUTO, a, ax, ay, n, err);
        long bad_b = p2e_ecdsa_public_key_batch(ctx, curve, P2E_SIGN_PLAN_AUTO, b, bx, by, n, err);
        long bad_s = p2e_point_mul_batch(ctx, curve, P2E_MUL_PLAN_PLAIN, a, bx, by, sx, sy, n, err);   /* a_i B_i */
        long bad_t = p2e_point_mul_batch(ctx, curve, other, b, ax, ay, tx, ty, n, err);                /* b_i A_i */
        if (bad_a < 0 || bad_b < 0 || bad_s < 0 || bad_t < 0) {
            fprintf(stderr, "p2e: %s\n", p2e_last_error());
            return 3;
        }
        if (hipMemcpy(host, sx, 4 * 32 * n, 2)) return 4;   /* Sx, Sy, Tx, Ty are contiguous */
        size_t equal = 0;
        for (size_t i = 0; i < n; i++)
            equal += memcmp(host + 32 * i, host + 32 * (2 * n + i), 32) == 0 && memcmp(host + 32 * (n + i), host + 32 * (3 * n + i), 32) == 0;
        /* a flagged element (a key that is 0 modulo n: not with these seeds) holds zeros on both sides and counts as equal */
        printf("curve %d: %zu of %zu shared secrets agree (%ld + %ld keys flagged, %ld + %ld products flagged)\n", curve, equal, n, bad_a,
               bad_b, bad_s, bad_t);
        failures += !(equal == n && bad_s == bad_t);
        p2e_ctx_destroy(ctx);
        hipFree(dev);
        free(host);
    }
    return failures ? 1 : 0;
}

/* Minimal C client of the point tables (include/p2e.h p2e_point_table_create, p2e_ecdsa_verify_table_batch): many signatures
 * by few known keys -- a validator set, one CA key.  Three secret keys become public keys (p2e_ecdsa_public_key_batch) and
 * sign a few hundred synthetic messages, key i % 3 signing message i (p2e_ecdsa_sign_batch).  The window table of the three
 * public keys is built once; every verification is then two table walks without a doubling.  All signatures must verify;
 * after one message is altered, all but that one.  The program prints the verdict counts.  Host buffers throughout (a
 * P2E_CTX_HOST_POINTERS context), so no HIP runtime call is needed here.
 *     gcc -std=c11 -Iinclude examples/verify_known_keys.c -Lplonky2-ecdsa_amd -lp2e_hip -o verify_known_keys
 *     GPU_MAX_HW_QUEUES=8 LD_LIBRARY_PATH=plonky2-ecdsa_amd:/opt/rocm/lib ./verify_known_keys 300 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "p2e.h"

#define KEYS 3

static uint64_t next64(uint64_t *s) {   /* splitmix64 */
    uint64_t z = (*s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
static void fill(uint8_t *dst, size_t bytes, uint64_t *seed) {   /* any 32 bytes are a scalar: the library takes them modulo n */
    for (size_t i = 0; i < bytes; i += 8) {
        uint64_t w = next64(seed);
        memcpy(dst + i, &w, 8);
    }
}
static size_t count(const uint8_t *v, size_t n) {
    size_t c = 0;
    for (size_t i = 0; i < n; i++) c += v[i] != 0;
    return c;
}

int main(int argc, char **argv) {
    size_t n = argc > 1 ? (size_t)strtoull(argv[1], NULL, 10) : 300;
    int failures = 0;
    if (n < 8) n = 8;
    for (int curve = P2E_CURVE_SECP256K1; curve <= P2E_CURVE_P256; curve++) {
        uint64_t seed = 2028 + (uint64_t)curve;
        uint8_t key[KEYS * 32], pkx[KEYS * 32], pky[KEYS * 32], key_err[KEYS];
        uint8_t *buf = malloc((5 * 32 + 2) * n);   /* msg, sk, nonce, r, s (32 n each), err, valid (n each) */
        uint32_t *idx = malloc(sizeof(uint32_t) * n);
        uint8_t *msg = buf, *sk = msg + 32 * n, *nonce = sk + 32 * n, *r = nonce + 32 * n, *s = r + 32 * n, *err = s + 32 * n, *valid = err + n;
        p2e_ctx *ctx = NULL;
        if (p2e_ctx_create(0, P2E_CTX_HOST_POINTERS, NULL, &ctx)) {
            fprintf(stderr, "p2e_ctx_create: %s\n", p2e_last_error());   /* no GPU: there is no CPU fallback */
            return 2;
        }
        fill(key, sizeof key, &seed);
        fill(msg, 32 * n, &seed);
        fill(nonce, 32 * n, &seed);
        for (size_t i = 0; i < n; i++) {
            idx[i] = (uint32_t)(i % KEYS);
            memcpy(sk + 32 * i, key + 32 * idx[i], 32);
        }
        if (p2e_ecdsa_public_key_batch(ctx, curve, P2E_SIGN_PLAN_AUTO, key, pkx, pky, KEYS, key_err) != 0 ||
            p2e_ecdsa_sign_batch(ctx, curve, P2E_SIGN_PLAN_AUTO, msg, sk, nonce, r, s, n, err) != 0) {
            fprintf(stderr, "key derivation or signing: %s\n", p2e_last_error());
            return 3;
        }
        p2e_point_table *table = NULL;
        long rejected = p2e_point_table_create(ctx, curve, pkx, pky, KEYS, key_err, &table);
        if (rejected != 0) {
            fprintf(stderr, "p2e_point_table_create: %ld (%s)\n", rejected, rejected < 0 ? p2e_last_error() : "rejected keys");
            return 3;
        }
        long bad = p2e_ecdsa_verify_table_batch(ctx, table, idx, msg, r, s, n, err, valid);
        size_t before = count(valid, n);
        msg[32 * 7] ^= 1;                                   /* signature 7 no longer fits its message */
        long bad2 = p2e_ecdsa_verify_table_batch(ctx, table, idx, msg, r, s, n, err, valid);
        size_t after = count(valid, n);
        if (bad < 0 || bad2 < 0) {
            fprintf(stderr, "p2e: %s\n", p2e_last_error());
            return 3;
        }
        printf("curve %d: %ld keys in the table; %zu of %zu signatures valid, %zu after altering message 7 (valid[7] = %d; %ld + %ld flagged)\n",
               curve, p2e_point_table_num_points(table), before, n, after, valid[7], bad, bad2);
        failures += !(before == n && after == n - 1 && valid[7] == 0 && bad == 0 && bad2 == 0);
        p2e_point_table_destroy(ctx, table);
        p2e_ctx_destroy(ctx);
        free(idx);
        free(buf);
    }
    return failures ? 1 : 0;
}

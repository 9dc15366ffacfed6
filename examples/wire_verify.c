/* Minimal C client of the wire-form calls (include/p2e.h): a Bitcoin-style batch -- 33-byte compressed keys, strict DER
 * signatures with a low s, raw messages -- is decoded, hashed with SHA-256d, verified and turned into witness columns on
 * the device.  The batch itself is made with the library (keys derived and encoded, messages signed and encoded), packed
 * on the host the way such input arrives (DER signatures concatenated without padding behind offsets), and uploaded again.
 *     gcc -std=c11 -Iinclude examples/wire_verify.c -Lplonky2-ecdsa_amd -lp2e_hip -L/opt/rocm/lib -lamdhip64 -o wire_verify
 *     GPU_MAX_HW_QUEUES=8 LD_LIBRARY_PATH=plonky2-ecdsa_amd:/opt/rocm/lib ./wire_verify 512
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

#define CHECK(call)                                                  \
    do {                                                             \
        if ((call) < 0) {                                            \
            fprintf(stderr, "%s: %s\n", #call, p2e_last_error());    \
            return 3;                                                \
        }                                                            \
    } while (0)

int main(int argc, char **argv) {
    size_t n = argc > 1 ? (size_t)strtoull(argv[1], NULL, 10) : 128;
    const int curve = P2E_CURVE_SECP256K1;
    /* messages of 1 .. 300 bytes, concatenated without padding */
    uint64_t seed = 2027, *msg_off = malloc((n + 1) * sizeof(uint64_t)), *sig_off = malloc((n + 1) * sizeof(uint64_t));
    msg_off[0] = 0;
    for (size_t i = 0; i < n; i++) msg_off[i + 1] = msg_off[i] + 1 + next64(&seed) % 300;
    size_t total = (size_t)msg_off[n];
    uint8_t *raw = malloc(total), *sk_host = malloc(32 * n);
    for (size_t i = 0; i < total; i++) raw[i] = (uint8_t)next64(&seed);
    for (size_t i = 0; i < 32 * n; i++) sk_host[i] = (uint8_t)next64(&seed);   /* any 32 bytes are a scalar */
    p2e_ctx *ctx = NULL;
    if (p2e_ctx_create(0, 0, NULL, &ctx)) {
        fprintf(stderr, "p2e_ctx_create: %s\n", p2e_last_error());   /* no GPU: there is no CPU fallback */
        return 2;
    }
    /* the three offset arrays (8 (n + 1) each); msg, sk, r, s, pkx, pky (32 n each); der (72 n), packed der (72 n), keys (33 n);
     * der_len, err, valid (n each); the raw bytes; the columns last (8-byte aligned) */
    size_t ld = n, fixed = 24 * (n + 1) + (6 * 32 + 2 * 72 + 33 + 3) * n;
    size_t cols_at = (fixed + total + 7) / 8 * 8;
    uint8_t *dev = NULL;
    if (hipMalloc((void **)&dev, cols_at + (size_t)P2E_VERIFY_COLS * ld * 8)) {
        fprintf(stderr, "device allocation failed\n");
        return 2;
    }
    uint64_t *d_msg_off = (uint64_t *)dev, *d_sig_off = d_msg_off + (n + 1), *d_key_off = d_sig_off + (n + 1);
    uint8_t *msg = dev + 24 * (n + 1), *sk = msg + 32 * n, *r = sk + 32 * n, *s = r + 32 * n, *pkx = s + 32 * n, *pky = pkx + 32 * n;
    uint8_t *der = pky + 32 * n, *packed = der + 72 * n, *keys = packed + 72 * n, *der_len = keys + 33 * n, *err = der_len + n;
    uint8_t *valid = err + n, *data = valid + n;
    uint64_t *cols = (uint64_t *)(dev + cols_at);
    if (hipMemcpy(d_msg_off, msg_off, 8 * (n + 1), 1) || hipMemcpy(sk, sk_host, 32 * n, 1) || hipMemcpy(data, raw, total, 1)) {
        fprintf(stderr, "upload failed\n");
        return 2;
    }
    /* ---- the sender's side: keys and signatures in wire form ---- */
    CHECK(p2e_hash_batch(ctx, P2E_HASH_SHA256D, P2E_DIGEST_SCALAR, data, d_msg_off, msg, n));
    CHECK(p2e_ecdsa_public_key_batch(ctx, curve, P2E_SIGN_PLAN_AUTO, sk, pkx, pky, n, err));
    CHECK(p2e_ecdsa_sign_deterministic_batch(ctx, curve, P2E_SIGN_PLAN_AUTO, msg, sk, r, s, NULL, n, err));
    long bad_enc_key = p2e_point_encode_batch(ctx, curve, P2E_SEC1_COMPRESSED, pkx, pky, keys, n, err);
    long bad_enc_sig = p2e_sig_encode_batch(ctx, curve, P2E_SIG_DER, P2E_SIG_NORMALIZE_S, r, s, NULL, der, der_len, n, err);
    CHECK(bad_enc_key);
    CHECK(bad_enc_sig);
    /* concatenate the signatures without padding, as a transaction carries them */
    uint8_t *der_host = malloc(72 * n), *len_host = malloc(n), *packed_host = calloc(72 * n + 1, 1);
    if (hipMemcpy(der_host, der, 72 * n, 2) || hipMemcpy(len_host, der_len, n, 2)) return 4;
    sig_off[0] = 0;
    for (size_t i = 0; i < n; i++) {
        memcpy(packed_host + sig_off[i], der_host + 72 * i, len_host[i]);
        sig_off[i + 1] = sig_off[i] + len_host[i];
    }
    uint64_t *key_off = malloc((n + 1) * sizeof(uint64_t));
    for (size_t i = 0; i <= n; i++) key_off[i] = 33 * i;
    /* ---- the receiver's side: nothing below depends on anything above but the wire bytes ---- */
    if (hipMemcpy(packed, packed_host, (size_t)sig_off[n] + 1, 1) || hipMemcpy(d_sig_off, sig_off, 8 * (n + 1), 1)) return 4;
    uint8_t zero32[32] = {0};
    for (size_t i = 0; i < n; i += 64)   /* wipe what the sender knew (spot-wise is enough to show it is rewritten) */
        if (hipMemcpy(r + 32 * i, zero32, 32, 1) || hipMemcpy(pkx + 32 * i, zero32, 32, 1)) return 4;
    long bad_sig = p2e_sig_decode_batch(ctx, curve, P2E_SIG_DER, P2E_SIG_REQUIRE_LOW_S, packed, d_sig_off, r, s, NULL, n, err);
    CHECK(bad_sig);
    if (hipMemcpy(d_key_off, key_off, 8 * (n + 1), 1)) return 4;
    long bad_key = p2e_point_decode_batch(ctx, curve, keys, d_key_off, pkx, pky, n, err);
    CHECK(bad_key);
    long bad_hash = p2e_hash_batch(ctx, P2E_HASH_SHA256D, P2E_DIGEST_SCALAR, data, d_msg_off, msg, n);
    CHECK(bad_hash);
    long bad_ver = p2e_ecdsa_verify_batch(ctx, msg, r, s, pkx, pky, n, err, valid);
    CHECK(bad_ver);
    uint8_t *valid_host = malloc(2 * n);
    if (hipMemcpy(valid_host, valid, n, 2)) return 4;
    long bad_fill = p2e_ecdsa_verify_witness_batch(ctx, msg, r, s, pkx, pky, cols, n, ld, err, valid);
    CHECK(bad_fill);
    if (hipMemcpy(valid_host + n, valid, n, 2)) return 4;
    size_t ok = 0, filled = 0;
    for (size_t i = 0; i < n; i++) ok += valid_host[i] == 1, filled += valid_host[n + i] == 1;
    printf("%zu keys decoded (%ld flagged), %zu signatures decoded (%ld flagged), %zu messages hashed, %zu valid, %zu witnesses filled\n",
           n, bad_key, n, bad_sig, n, ok, filled);
    p2e_ctx_destroy(ctx);
    hipFree(dev);
    free(msg_off), free(sig_off), free(key_off), free(raw), free(sk_host), free(der_host), free(len_host), free(packed_host), free(valid_host);
    return (bad_enc_key == 0 && bad_enc_sig == 0 && bad_key == 0 && bad_sig == 0 && bad_hash == 0 && bad_ver == 0 && bad_fill == 0 &&
            ok == n && filled == n) ? 0 : 1;
}

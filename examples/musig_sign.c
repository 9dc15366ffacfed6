/* Minimal C client of the MuSig2 calls (include/p2e.h p2e_musig_key_agg_batch and the six calls after it): n Taproot key-path
 * signatures, each made by TWO signers who never see each other's key -- what the two ends of a Taproot Lightning channel do.
 * Session i: the keys a_i G and b_i G are aggregated (p2e_musig_key_agg_batch) and tweaked as BIP-86 asks for a key-path-only
 * output (p2e_musig_apply_tweak_batch, P2E_MUSIG_TWEAK_TAPROOT without a root); both signers publish a nonce pair
 * (p2e_ecdsa_public_key_batch on k_1 and k_2), the pairs are summed (p2e_musig_nonce_agg_batch), the session values derived
 * (p2e_musig_session_batch); each signer signs (p2e_musig_partial_sign_batch), checks the other's partial signature
 * (p2e_musig_partial_verify_batch), and the two are added (p2e_musig_sig_agg_batch).  The result is an ordinary BIP-340
 * signature: p2e_schnorr_verify_batch accepts it under the tweaked aggregate key.
 * Keys, nonces and points are the library's little-endian 32-byte values, messages, partial signatures, agg_pk and sig the
 * standard's big-endian strings.  Host pointers (P2E_CTX_HOST_POINTERS) keep the example free of HIP calls.
 *     gcc -std=c11 -Iinclude examples/musig_sign.c -Lplonky2-ecdsa_amd -lp2e_hip -L/opt/rocm/lib -lamdhip64 -o musig_sign
 *     LD_LIBRARY_PATH=plonky2-ecdsa_amd:/opt/rocm/lib ./musig_sign 1000
 * The secret nonces here are COUNTERS so that the example is reproducible.  A real signer draws them from a CSPRNG, uses each
 * pair for ONE signature and wipes it: two signatures with one nonce reveal the key. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "p2e.h"

/* element i = the little-endian scalar (tag << 32) + i + 1 */
static void fill_scalars(uint8_t *out, size_t stride, size_t n, uint32_t tag) {
    for (size_t i = 0; i < n; i++) {
        const uint32_t v = (uint32_t)i + 1;
        memset(out + stride * i, 0, 32);
        memcpy(out + stride * i, &v, 4);
        memcpy(out + stride * i + 4, &tag, 4);
    }
}

int main(int argc, char **argv) {
    size_t n = argc > 1 ? (size_t)strtoull(argv[1], NULL, 10) : 256;
    if (n < 1) n = 1;
    p2e_ctx *ctx = NULL;
    if (p2e_ctx_create(0, P2E_CTX_HOST_POINTERS, NULL, &ctx)) {
        fprintf(stderr, "p2e_ctx_create: %s\n", p2e_last_error());   /* no GPU: there is no CPU fallback */
        return 2;
    }
    /* per-signer arrays: signer 2 i is a_i, signer 2 i + 1 is b_i */
    uint8_t *sk = malloc(64 * n), *pkx = malloc(64 * n), *pky = malloc(64 * n), *secnonce = malloc(128 * n), *pubnonce = malloc(256 * n);
    uint8_t *k = malloc(128 * n), *kx = malloc(128 * n), *ky = malloc(128 * n), *psig = malloc(64 * n), *err2 = malloc(4 * n), *valid = malloc(2 * n);
    uint64_t *offsets = malloc(8 * (n + 1));
    uint32_t *owner = malloc(8 * n);
    /* per-session arrays */
    uint8_t *keyagg = malloc(192 * n), *agg_pk = malloc(32 * n), *aggnonce = malloc(128 * n), *msg = malloc(32 * n), *session = malloc(128 * n);
    uint8_t *sig = malloc(64 * n), *err = malloc(n), *ok = malloc(n), *one_sk = malloc(32 * n), *one_nonce = malloc(64 * n), *one_psig = malloc(32 * n);
    fill_scalars(sk, 32, 2 * n, 0x5ec7e7u);
    fill_scalars(k, 32, 4 * n, 0x707ce5u);   /* k_1, k_2 of signer j at 2 j, 2 j + 1 */
    for (size_t i = 0; i <= n; i++) offsets[i] = 2 * i;
    for (size_t j = 0; j < 2 * n; j++) owner[j] = (uint32_t)(j / 2);
    for (size_t i = 0; i < n; i++) memset(msg + 32 * i, (int)(i & 0xff), 32);
    long bad = 0, rc;
#define STEP(call)                                              \
    do {                                                        \
        if ((rc = (call)) < 0) {                                \
            fprintf(stderr, "p2e: %s\n", p2e_last_error());     \
            return 3;                                           \
        }                                                       \
        bad += rc;                                              \
    } while (0)
    STEP(p2e_ecdsa_public_key_batch(ctx, P2E_CURVE_SECP256K1, P2E_SIGN_PLAN_LANE, sk, pkx, pky, 2 * n, err2));
    STEP(p2e_ecdsa_public_key_batch(ctx, P2E_CURVE_SECP256K1, P2E_SIGN_PLAN_LANE, k, kx, ky, 4 * n, err2));
    for (size_t j = 0; j < 2 * n; j++) {   /* secnonce64 = k_1 || k_2, pubnonce128 = x(R_1) || y(R_1) || x(R_2) || y(R_2) */
        memcpy(secnonce + 64 * j, k + 64 * j, 64);
        memcpy(pubnonce + 128 * j, kx + 64 * j, 32), memcpy(pubnonce + 128 * j + 32, ky + 64 * j, 32);
        memcpy(pubnonce + 128 * j + 64, kx + 64 * j + 32, 32), memcpy(pubnonce + 128 * j + 96, ky + 64 * j + 32, 32);
    }
    STEP(p2e_musig_key_agg_batch(ctx, pkx, pky, offsets, keyagg, agg_pk, n, err));
    STEP(p2e_musig_apply_tweak_batch(ctx, keyagg, NULL, P2E_MUSIG_TWEAK_TAPROOT, keyagg, agg_pk, n, err));   /* in place */
    STEP(p2e_musig_nonce_agg_batch(ctx, pubnonce, offsets, aggnonce, n, err));
    STEP(p2e_musig_session_batch(ctx, keyagg, aggnonce, msg, session, n, err));
    for (int who = 0; who < 2; who++) {    /* each signer's own batch: one lane per session */
        for (size_t i = 0; i < n; i++) {
            memcpy(one_sk + 32 * i, sk + 32 * (2 * i + who), 32);
            memcpy(one_nonce + 64 * i, secnonce + 64 * (2 * i + who), 64);
        }
        STEP(p2e_musig_partial_sign_batch(ctx, one_nonce, one_sk, keyagg, session, one_psig, n, err));
        for (size_t i = 0; i < n; i++) memcpy(psig + 32 * (2 * i + who), one_psig + 32 * i, 32);
    }
    STEP(p2e_musig_partial_verify_batch(ctx, psig, pubnonce, pkx, pky, owner, keyagg, session, n, 2 * n, err2, valid));
    STEP(p2e_musig_sig_agg_batch(ctx, psig, offsets, keyagg, session, sig, n, err));
    STEP(p2e_schnorr_verify_batch(ctx, msg, agg_pk, sig, n, err, ok));
    size_t partial_ok = 0, accepted = 0;
    for (size_t j = 0; j < 2 * n; j++) partial_ok += valid[j];
    for (size_t i = 0; i < n; i++) accepted += ok[i];
    printf("%zu two-party Taproot signatures: %zu of %zu partial signatures valid, %zu accepted by the BIP-340 verifier, %ld refused; sig[0] = ",
           n, partial_ok, 2 * n, accepted, bad);
    for (int j = 0; j < 64; j++) printf("%02x", sig[j]);
    printf("\n");
    p2e_ctx_destroy(ctx);
    memset(sk, 0, 64 * n), memset(k, 0, 128 * n), memset(secnonce, 0, 128 * n), memset(one_sk, 0, 32 * n), memset(one_nonce, 0, 64 * n);
    free(sk), free(pkx), free(pky), free(secnonce), free(pubnonce), free(k), free(kx), free(ky), free(psig), free(err2), free(valid);
    free(offsets), free(owner), free(keyagg), free(agg_pk), free(aggnonce), free(msg), free(session), free(sig), free(err), free(ok);
    free(one_sk), free(one_nonce), free(one_psig);
    return (bad == 0 && partial_ok == 2 * n && accepted == n) ? 0 : 1;
}

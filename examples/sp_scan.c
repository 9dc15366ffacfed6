/* Minimal C client of the silent-payment calls (include/p2e.h p2e_sp_input_hash_batch and the three calls after it): one
 * BIP-352 payment is made and found again among decoys.  The receiver's scan and spend keys are the hardened children 0' and
 * 1' of BIP-32's test vector 1 at m/0' (p2e_bip32_ckd_priv_batch), their public keys p2e_ecdsa_public_key_batch's.  Every
 * transaction i has one input key a_i (A_i = a_i G), an outpoint and two outputs; the sender of transaction n / 2 pays the
 * receiver with p2e_sp_send_batch into output 1, every other output is a decoy.  The receiver then scans all n transactions
 * with p2e_sp_scan_batch: one ECDH, one hash, one fixed-base walk and one compare per transaction, without visiting the host.
 * Keys and points are the library's little-endian 32-byte values, outpoints, input hashes, outputs and tweaks the standard's
 * big-endian strings.  Host pointers (P2E_CTX_HOST_POINTERS) keep the example free of HIP calls.
 *     gcc -std=c11 -Iinclude examples/sp_scan.c -Lplonky2-ecdsa_amd -lp2e_hip -L/opt/rocm/lib -lamdhip64 -o sp_scan
 *     LD_LIBRARY_PATH=plonky2-ecdsa_amd:/opt/rocm/lib ./sp_scan 1000
 * Summing a transaction's input keys, choosing eligible inputs and the sp1... address string are the caller's. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "p2e.h"

static void unhex(const char *s, uint8_t *out) {
    for (size_t i = 0; s[2 * i]; i++) {
        unsigned v = 0;
        sscanf(s + 2 * i, "%2x", &v);
        out[i] = (uint8_t)v;
    }
}
/* a 32-byte value reversed in place */
static void flip32(uint8_t *v) {
    for (int j = 0; j < 16; j++) {
        uint8_t t = v[j];
        v[j] = v[31 - j];
        v[31 - j] = t;
    }
}

int main(int argc, char **argv) {
    size_t n = argc > 1 ? (size_t)strtoull(argv[1], NULL, 10) : 256;
    if (n < 2) n = 2;
    const size_t target = n / 2;
    uint8_t par_sk[32], par_cc[32];
    unhex("edb2e14f9ee77d26dd93b4ecede8d16ed408ce149b6cd80b0715a2d911a0afea", par_sk);
    unhex("47fdacbd0f1097043b78c63c20c34ef4ed9a111d980047ad16282c7ae6236141", par_cc);
    flip32(par_sk);   /* BIP-32 keys are little-endian in this library */
    p2e_ctx *ctx = NULL;
    if (p2e_ctx_create(0, P2E_CTX_HOST_POINTERS, NULL, &ctx)) {
        fprintf(stderr, "p2e_ctx_create: %s\n", p2e_last_error());   /* no GPU: there is no CPU fallback */
        return 2;
    }
    /* the receiver: (scan key, spend key) = m/0'/0', m/0'/1' and their public keys */
    const uint32_t hardened[2] = {0x80000000u, 0x80000001u};
    uint8_t sk[64], cc[64], pkx[64], pky[64], e2[2] = {0, 0};
    long bad_keys = p2e_bip32_ckd_priv_batch(ctx, par_sk, par_cc, 1, hardened, sk, cc, 2, e2);
    long bad_pub = p2e_ecdsa_public_key_batch(ctx, P2E_CURVE_SECP256K1, P2E_SIGN_PLAN_LANE, sk, pkx, pky, 2, e2);
    /* the chain: n transactions, each with one input key, one outpoint and two outputs */
    uint8_t *a = calloc(n, 32), *ax = malloc(32 * n), *ay = malloc(32 * n), *outpoint = malloc(36 * n), *ih = malloc(32 * n);
    uint8_t *outputs = malloc(64 * n), *err = malloc(n), *n_hits = malloc(n), *hit_label = malloc(n), *hit_tweak = malloc(32 * n);
    uint32_t *hit_output = malloc(4 * n);
    uint64_t *offsets = malloc(8 * (n + 1));
    uint32_t lcg = 12345;
    for (size_t i = 0; i < n; i++) {
        const uint32_t v = (uint32_t)i + 1;
        memcpy(a + 32 * i, &v, 4);
        a[32 * i + 8] = 1;
        memset(outpoint + 36 * i, 0x42, 32);
        memcpy(outpoint + 36 * i + 32, &v, 4);
        for (int j = 0; j < 64; j++) outputs[64 * i + j] = (uint8_t)((lcg = lcg * 1664525u + 1013904223u) >> 24);
        offsets[i] = 2 * i;
    }
    offsets[n] = 2 * n;
    long bad_a = p2e_ecdsa_public_key_batch(ctx, P2E_CURVE_SECP256K1, P2E_SIGN_PLAN_LANE, a, ax, ay, n, err);
    long bad_ih = p2e_sp_input_hash_batch(ctx, outpoint, ax, ay, ih, n, err);
    /* the sender of transaction `target` pays the receiver: k = 0, into output 1 */
    const uint32_t k0 = 0;
    uint8_t e1 = 0;
    long bad_send = p2e_sp_send_batch(ctx, a + 32 * target, ih + 32 * target, pkx, pky, pkx + 32, pky + 32, &k0, outputs + 64 * target + 32, 1, &e1);
    /* the receiver scans the chain */
    long bad_scan = p2e_sp_scan_batch(ctx, sk, pkx + 32, pky + 32, NULL, NULL, 0, ax, ay, ih, outputs, offsets, 1, n_hits, hit_output, hit_label,
                                      hit_tweak, n, err);
    if (bad_keys < 0 || bad_pub < 0 || bad_a < 0 || bad_ih < 0 || bad_send < 0 || bad_scan < 0) {
        fprintf(stderr, "p2e: %s\n", p2e_last_error());
        return 3;
    }
    size_t found = 0, where = 0;
    for (size_t i = 0; i < n; i++)
        if (n_hits[i]) found++, where = i;
    const int right = found == 1 && where == target && hit_output[target] == 1 && hit_label[target] == 0;
    printf("%zu transactions scanned (%ld refused): %zu payment found%s in transaction %zu, output %u, key ", n, bad_scan, found,
           right ? "" : " (WRONG)", where, (unsigned)hit_output[where]);
    for (int j = 0; j < 32; j++) printf("%02x", outputs[64 * target + 32 + j]);
    printf("\n");
    p2e_ctx_destroy(ctx);
    memset(sk, 0, 64), memset(par_sk, 0, 32), memset(a, 0, 32 * n), memset(hit_tweak, 0, 32 * n);
    free(a), free(ax), free(ay), free(outpoint), free(ih), free(outputs), free(err), free(n_hits), free(hit_label), free(hit_tweak);
    free(hit_output), free(offsets);
    return (bad_keys == 0 && bad_pub == 0 && bad_a == 0 && bad_ih == 0 && bad_send == 0 && bad_scan == 0 && right) ? 0 : 1;
}

/* Minimal C client of the BIP-39 call (include/p2e.h): ONE mnemonic sentence against a list of candidate passphrases.
 * Every candidate becomes a seed (p2e_bip39_seed_batch with n_mnemonics = 1: every lane reads sentence 0), the seed a master
 * key, the master key its hardened child m/0', that key a public key and the public key a HASH160; the program prints the
 * index of the candidate whose key hash is the target.  The sentence is BIP-39's "abandon ... about"; the target is the key
 * hash of m/0' under the passphrase TREZOR, which stands at index n / 3 of the candidates "candidate-<i>".
 * Host pointers (P2E_CTX_HOST_POINTERS) keep the example free of HIP calls; on device pointers the five calls chain without
 * a copy in between, and the seeds never visit the host.
 *     gcc -std=c11 -Iinclude examples/mnemonic_scan.c -Lplonky2-ecdsa_amd -lp2e_hip -L/opt/rocm/lib -lamdhip64 -o mnemonic_scan
 *     LD_LIBRARY_PATH=plonky2-ecdsa_amd:/opt/rocm/lib ./mnemonic_scan 1000
 * NFKD normalisation of the sentence and the passphrases is the caller's (these are ASCII); the wordlist and the checksum
 * are not looked at. */
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

int main(int argc, char **argv) {
    size_t n = argc > 1 ? (size_t)strtoull(argv[1], NULL, 10) : 256;
    if (n < 3) n = 3;
    const char *words = "abandon abandon abandon abandon abandon abandon abandon abandon abandon abandon abandon about";
    const size_t secret = n / 3;
    uint8_t target[20];
    unhex("f99a31bb9adc65888283cc9bd22f594cc358586e", target);
    /* the sentence, and the candidates back to back: element i is passphrase[pp_offsets[i], pp_offsets[i + 1]) */
    uint8_t mnemonic[96] = {0};                                          /* (93 bytes, the buffer a multiple of 4) */
    const uint64_t mn_offsets[2] = {0, strlen(words)};
    memcpy(mnemonic, words, strlen(words));
    uint8_t *passphrase = calloc(32 * n + 4, 1);
    uint64_t *pp_offsets = malloc((n + 1) * sizeof(uint64_t));
    pp_offsets[0] = 0;
    for (size_t i = 0; i < n; i++) {
        char *at = (char *)passphrase + pp_offsets[i];
        int len = i == secret ? snprintf(at, 32, "TREZOR") : snprintf(at, 32, "candidate-%zu", i);
        pp_offsets[i + 1] = pp_offsets[i] + (uint64_t)len;               /* (the terminating zero is overwritten by the next one) */
    }
    p2e_ctx *ctx = NULL;
    if (p2e_ctx_create(0, P2E_CTX_HOST_POINTERS, NULL, &ctx)) {
        fprintf(stderr, "p2e_ctx_create: %s\n", p2e_last_error());   /* no GPU: there is no CPU fallback */
        return 2;
    }
    uint8_t *seed = malloc(64 * n), *sk = malloc(32 * n), *cc = malloc(32 * n), *pkx = malloc(32 * n), *pky = malloc(32 * n);
    uint8_t *hash = malloc(20 * n), *err = malloc(n);
    uint32_t *index = malloc(n * sizeof(uint32_t));
    for (size_t i = 0; i < n; i++) index[i] = 0x80000000u;              /* m/0' */
    long bad_seed = p2e_bip39_seed_batch(ctx, mnemonic, mn_offsets, 1, passphrase, pp_offsets, n, seed, n, err);
    long bad_master = bad_seed < 0 ? -1 : p2e_bip32_master_batch(ctx, seed, 64, sk, cc, n, err);
    long bad_child = bad_master < 0 ? -1 : p2e_bip32_ckd_priv_batch(ctx, sk, cc, n, index, sk, cc, n, err);   /* in place */
    long bad_pub = bad_child < 0 ? -1 : p2e_ecdsa_public_key_batch(ctx, P2E_CURVE_SECP256K1, P2E_SIGN_PLAN_AUTO, sk, pkx, pky, n, err);
    long rc_hash = bad_pub < 0 ? -1 : p2e_key_hash160_batch(ctx, P2E_SEC1_COMPRESSED, pkx, pky, err, hash, n);
    if (rc_hash < 0) {
        fprintf(stderr, "p2e: %s\n", p2e_last_error());
        return 3;
    }
    long found = -1, matches = 0;
    for (size_t i = 0; i < n; i++)
        if (memcmp(hash + 20 * i, target, 20) == 0) found = (long)i, matches++;
    printf("%zu passphrases tried against one mnemonic (%ld refused), %ld match the target key hash: index %ld", n,
           bad_seed + bad_master + bad_child + bad_pub, matches, found);
    if (found >= 0) printf(" (%.*s)", (int)(pp_offsets[found + 1] - pp_offsets[found]), (const char *)passphrase + pp_offsets[found]);
    printf("\n");
    p2e_ctx_destroy(ctx);
    free(passphrase), free(pp_offsets), free(seed), free(sk), free(cc), free(pkx), free(pky), free(hash), free(err), free(index);
    return (matches == 1 && found == (long)secret) ? 0 : 1;
}

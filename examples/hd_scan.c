/* Minimal C client of the hierarchical-key calls (include/p2e.h): the scan of ONE extended public key.  The key of BIP-32's
 * test vector 1 at m/0' arrives as the wire holds it (a 33-byte SEC1 key and a 32-byte chain code); it is decoded once, its
 * non-hardened children 0 .. n - 1 are derived with n_parents = 1 (every lane reads parent 0), and each child's HASH160 --
 * the payload of its P2PKH / P2WPKH output -- is computed; child 1 must be the vector's m/0'/1.
 * Host pointers (P2E_CTX_HOST_POINTERS) keep the example free of HIP calls; on device pointers the four calls chain without
 * a copy in between.
 *     gcc -std=c11 -Iinclude examples/hd_scan.c -Lplonky2-ecdsa_amd -lp2e_hip -L/opt/rocm/lib -lamdhip64 -o hd_scan
 *     LD_LIBRARY_PATH=plonky2-ecdsa_amd:/opt/rocm/lib ./hd_scan 1000
 * Base58Check (xpub strings, addresses) is the caller's: the bytes derived here are the bytes those strings carry. */
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
    if (n < 2) n = 2;
    uint8_t xpub_key[36] = {0}, xpub_cc[32], want_key[33], want_cc[32];   /* (the key's buffer padded to a multiple of 4) */
    unhex("035a784662a4a20a65bf6aab9ae98a6c068a81c52e4b032c0fb5400c706cfccc56", xpub_key);
    unhex("47fdacbd0f1097043b78c63c20c34ef4ed9a111d980047ad16282c7ae6236141", xpub_cc);
    unhex("03501e454bf00751f24b1b489aa925215d66af2234e3891c3b21a52bedb3cd711c", want_key);
    unhex("2a7857631386ba23dacac34180dd1983734e444fdbf774041578e9b6adb37c19", want_cc);
    p2e_ctx *ctx = NULL;
    if (p2e_ctx_create(0, P2E_CTX_HOST_POINTERS, NULL, &ctx)) {
        fprintf(stderr, "p2e_ctx_create: %s\n", p2e_last_error());   /* no GPU: there is no CPU fallback */
        return 2;
    }
    const uint64_t one_key[2] = {0, 33};
    uint8_t par_x[32], par_y[32], par_err = 0;
    uint32_t *index = malloc(n * sizeof(uint32_t));
    uint8_t *pkx = malloc(32 * n), *pky = malloc(32 * n), *cc = malloc(32 * n), *err = malloc(n), *hash = malloc(20 * n), *sec1 = malloc(33 * n);
    for (size_t i = 0; i < n; i++) index[i] = (uint32_t)i;
    long bad_key = p2e_point_decode_batch(ctx, P2E_CURVE_SECP256K1, xpub_key, one_key, par_x, par_y, 1, &par_err);
    long bad_child = p2e_bip32_ckd_pub_batch(ctx, par_x, par_y, xpub_cc, 1, index, pkx, pky, cc, n, err);
    long rc_hash = p2e_key_hash160_batch(ctx, P2E_SEC1_COMPRESSED, pkx, pky, err, hash, n);   /* err: a refused child has no hash */
    long bad_enc = p2e_point_encode_batch(ctx, P2E_CURVE_SECP256K1, P2E_SEC1_COMPRESSED, pkx, pky, sec1, n, err);
    if (bad_key < 0 || bad_child < 0 || rc_hash < 0 || bad_enc < 0) {
        fprintf(stderr, "p2e: %s\n", p2e_last_error());
        return 3;
    }
    int known = memcmp(sec1 + 33, want_key, 33) == 0 && memcmp(cc + 32, want_cc, 32) == 0;
    printf("%zu children of m/0' derived (%ld refused), child 1 %s m/0'/1 of test vector 1, its key hash ", n, bad_child,
           known ? "is" : "IS NOT");
    for (int j = 0; j < 20; j++) printf("%02x", hash[20 + j]);
    printf("\n");
    p2e_ctx_destroy(ctx);
    free(index), free(pkx), free(pky), free(cc), free(err), free(hash), free(sec1);
    return (bad_key == 0 && bad_child == 0 && bad_enc == 0 && known) ? 0 : 1;
}

/* Minimal C client of the Taproot calls (include/p2e.h p2e_taproot_leaf_hash_batch and the four calls after it): the scan
 * of ONE extended public key for its BIP-86 outputs, and one key-path spend.  The key of BIP-32's test vector 1 at m/0'
 * arrives as the wire holds it; its non-hardened children 0 .. n - 1 are derived (p2e_bip32_ckd_pub_batch) and each child's
 * x-only key is tweaked with H_TapTweak(key) alone (root32 = NULL): the 32 bytes of its P2TR witness program.  Then the
 * SECRET child 1 is derived from the vector's private key, tweaked the same way (p2e_taproot_tweak_seckey_batch) and signs a
 * message (p2e_schnorr_sign_batch); the signature must verify under output key 1 of the public scan.
 * The BIP-32 calls speak the library's little-endian 32-byte values, the Schnorr and Taproot calls the standards' big-endian
 * strings: the bytes are reversed in between (be32 below; on device pointers a byte flip of the caller's).
 * Host pointers (P2E_CTX_HOST_POINTERS) keep the example free of HIP calls.
 *     gcc -std=c11 -Iinclude examples/taproot_scan.c -Lplonky2-ecdsa_amd -lp2e_hip -L/opt/rocm/lib -lamdhip64 -o taproot_scan
 *     LD_LIBRARY_PATH=plonky2-ecdsa_amd:/opt/rocm/lib ./taproot_scan 1000
 * Bech32m (the address string) is the caller's: the bytes derived here are the bytes that string carries. */
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
/* n 32-byte values, each reversed in place */
static void be32(uint8_t *v, size_t n) {
    for (size_t i = 0; i < n; i++)
        for (int j = 0; j < 16; j++) {
            uint8_t t = v[32 * i + j];
            v[32 * i + j] = v[32 * i + 31 - j];
            v[32 * i + 31 - j] = t;
        }
}

int main(int argc, char **argv) {
    size_t n = argc > 1 ? (size_t)strtoull(argv[1], NULL, 10) : 256;
    if (n < 2) n = 2;
    uint8_t xpub_key[36] = {0}, cc_par[32], xprv_key[32];   /* (the key's buffer padded to a multiple of 4) */
    unhex("035a784662a4a20a65bf6aab9ae98a6c068a81c52e4b032c0fb5400c706cfccc56", xpub_key);
    unhex("47fdacbd0f1097043b78c63c20c34ef4ed9a111d980047ad16282c7ae6236141", cc_par);
    unhex("edb2e14f9ee77d26dd93b4ecede8d16ed408ce149b6cd80b0715a2d911a0afea", xprv_key);
    be32(xprv_key, 1);   /* BIP-32 keys are little-endian in this library */
    p2e_ctx *ctx = NULL;
    if (p2e_ctx_create(0, P2E_CTX_HOST_POINTERS, NULL, &ctx)) {
        fprintf(stderr, "p2e_ctx_create: %s\n", p2e_last_error());   /* no GPU: there is no CPU fallback */
        return 2;
    }
    /* the public scan: children -> x-only keys -> BIP-86 output keys */
    const uint64_t one_key[2] = {0, 33};
    uint8_t par_x[32], par_y[32], par_err = 0;
    uint32_t *index = malloc(n * sizeof(uint32_t));
    uint8_t *pkx = malloc(32 * n), *pky = malloc(32 * n), *cc = malloc(32 * n), *err = malloc(n), *out_pk = malloc(32 * n), *parity = malloc(n);
    for (size_t i = 0; i < n; i++) index[i] = (uint32_t)i;
    long bad_key = p2e_point_decode_batch(ctx, P2E_CURVE_SECP256K1, xpub_key, one_key, par_x, par_y, 1, &par_err);
    long bad_child = p2e_bip32_ckd_pub_batch(ctx, par_x, par_y, cc_par, 1, index, pkx, pky, cc, n, err);
    be32(pkx, n);
    long bad_tweak = p2e_taproot_tweak_pubkey_batch(ctx, pkx, NULL, out_pk, parity, n, err);
    /* the key-path spend of child 1 */
    const uint32_t one = 1;
    uint8_t sk[32], sk_cc[32], tweaked[32], msg[32], aux[32] = {0}, sig[64], e1 = 0, valid = 0;
    memset(msg, 0x5A, 32);
    long bad_sk = p2e_bip32_ckd_priv_batch(ctx, xprv_key, cc_par, 1, &one, sk, sk_cc, 1, &e1);
    be32(sk, 1);
    long bad_tsk = p2e_taproot_tweak_seckey_batch(ctx, sk, NULL, tweaked, 1, &e1);
    long bad_sign = p2e_schnorr_sign_batch(ctx, msg, tweaked, aux, sig, 1, &e1);
    long bad_verify = p2e_schnorr_verify_batch(ctx, msg, out_pk + 32, sig, 1, &e1, &valid);
    if (bad_key < 0 || bad_child < 0 || bad_tweak < 0 || bad_sk < 0 || bad_tsk < 0 || bad_sign < 0 || bad_verify < 0) {
        fprintf(stderr, "p2e: %s\n", p2e_last_error());
        return 3;
    }
    printf("%zu children of m/0' tweaked (%ld refused); the key-path signature of child 1 %s under output key ", n, bad_child + bad_tweak,
           valid == 1 ? "verifies" : "DOES NOT verify");
    for (int j = 0; j < 32; j++) printf("%02x", out_pk[32 + j]);
    printf("\n");
    p2e_ctx_destroy(ctx);
    free(index), free(pkx), free(pky), free(cc), free(err), free(out_pk), free(parity);
    memset(sk, 0, 32), memset(tweaked, 0, 32), memset(xprv_key, 0, 32);
    return (bad_key == 0 && bad_child == 0 && bad_tweak == 0 && bad_sk == 0 && bad_tsk == 0 && bad_sign == 0 && bad_verify == 0 && valid == 1) ? 0 : 1;
}

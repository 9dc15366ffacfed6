/* Minimal C client of the whole sender pipeline (include/p2e.h): raw messages on the device are hashed with Keccak-256
 * into message scalars, signed deterministically (RFC 6979 nonces, recovery byte v), the signers' keys are recovered from
 * (msg, r, s, v) and turned into Ethereum addresses, which must equal the addresses of the keys the secrets derive.
 * Device buffers throughout: nothing crosses to the host between the six calls.
 *     gcc -std=c11 -Iinclude examples/eth_sender.c -Lplonky2-ecdsa_amd -lp2e_hip -L/opt/rocm/lib -lamdhip64 -o eth_sender
 *     GPU_MAX_HW_QUEUES=8 LD_LIBRARY_PATH=plonky2-ecdsa_amd:/opt/rocm/lib ./eth_sender 512
 * The three HIP runtime calls a C client needs are declared here, so that no HIP header (C++) is required.
 * RLP, EIP-155 and personal_sign framing are the caller's: the bytes hashed here are the bytes given. */
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
    /* messages of 1 .. 300 bytes, concatenated without padding: start offsets take every alignment */
    uint64_t seed = 2026, *offsets = malloc((n + 1) * sizeof(uint64_t));
    offsets[0] = 0;
    for (size_t i = 0; i < n; i++) offsets[i + 1] = offsets[i] + 1 + next64(&seed) % 300;
    size_t total = (size_t)offsets[n];
    uint8_t *raw = malloc(total), *sk_host = malloc(32 * n), *addr = malloc(2 * 20 * n);
    for (size_t i = 0; i < total; i++) raw[i] = (uint8_t)next64(&seed);
    for (size_t i = 0; i < 32 * n; i++) sk_host[i] = (uint8_t)next64(&seed);   /* any 32 bytes are a scalar */
    p2e_ctx *ctx = NULL;
    if (p2e_ctx_create(0, 0, NULL, &ctx)) {
        fprintf(stderr, "p2e_ctx_create: %s\n", p2e_last_error());   /* no GPU: there is no CPU fallback */
        return 2;
    }
    /* offsets (8 (n + 1)); msg, sk, r, s, pkx, pky, wantx, wanty (32 n each); both address arrays (20 n each); v, err (n
     * each); the raw bytes last */
    uint8_t *dev = NULL;
    size_t fixed = 8 * (n + 1) + (8 * 32 + 2 * 20 + 2) * n;
    if (hipMalloc((void **)&dev, fixed + total)) {
        fprintf(stderr, "device allocation failed\n");
        return 2;
    }
    uint64_t *doff = (uint64_t *)dev;
    uint8_t *msg = dev + 8 * (n + 1), *sk = msg + 32 * n, *r = sk + 32 * n, *s = r + 32 * n, *pkx = s + 32 * n, *pky = pkx + 32 * n;
    uint8_t *wantx = pky + 32 * n, *wanty = wantx + 32 * n, *got_addr = wanty + 32 * n, *want_addr = got_addr + 20 * n;
    uint8_t *v = want_addr + 20 * n, *err = v + n, *data = err + n;
    if (hipMemcpy(doff, offsets, 8 * (n + 1), 1) || hipMemcpy(sk, sk_host, 32 * n, 1) || hipMemcpy(data, raw, total, 1)) {
        fprintf(stderr, "upload failed\n");
        return 2;
    }
    long bad_hash = p2e_hash_batch(ctx, P2E_HASH_KECCAK256, P2E_DIGEST_SCALAR, data, doff, msg, n);
    long bad_sig = p2e_ecdsa_sign_deterministic_batch(ctx, P2E_CURVE_SECP256K1, P2E_SIGN_PLAN_AUTO, msg, sk, r, s, v, n, err);
    long bad_rec = p2e_ecdsa_recover_batch(ctx, P2E_CURVE_SECP256K1, msg, r, s, v, pkx, pky, n, err);
    long rc_addr = p2e_eth_address_batch(ctx, pkx, pky, err, got_addr, n);   /* err: a key that was not recovered has no address */
    /* for the comparison: the addresses of the keys the secrets derive */
    long bad_pk = p2e_ecdsa_public_key_batch(ctx, P2E_CURVE_SECP256K1, P2E_SIGN_PLAN_AUTO, sk, wantx, wanty, n, err);
    long rc_want = p2e_eth_address_batch(ctx, wantx, wanty, err, want_addr, n);
    if (bad_hash < 0 || bad_sig < 0 || bad_rec < 0 || rc_addr < 0 || bad_pk < 0 || rc_want < 0) {
        fprintf(stderr, "p2e: %s\n", p2e_last_error());
        return 3;
    }
    if (hipMemcpy(addr, got_addr, 2 * 20 * n, 2)) return 4;
    size_t same = 0;
    for (size_t i = 0; i < n; i++) same += memcmp(addr + 20 * i, addr + 20 * (n + i), 20) == 0;
    printf("%zu messages hashed (%ld malformed), %zu signed (%ld flagged), %zu keys recovered (%ld flagged), %zu sender addresses match\n",
           n, bad_hash, n, bad_sig, n, bad_rec, same);
    p2e_ctx_destroy(ctx);
    hipFree(dev);
    free(offsets), free(raw), free(sk_host), free(addr);
    return (bad_hash == 0 && bad_sig == 0 && bad_rec == 0 && bad_pk == 0 && same == n) ? 0 : 1;
}

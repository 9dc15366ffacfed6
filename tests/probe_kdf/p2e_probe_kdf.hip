// Test-only PLAIN PBKDF2-HMAC-SHA512: the second implementation on the device and the yardstick of tools/bench_kdf.py.
//
// The same function as csrc/kdf.hpp's kernel, written the straightforward way with hd.hpp's unchanged sha512_compress and
// nothing of kdf.hpp: messages are gathered byte by byte (no aligned-word view, no carried word), every compression is the
// general one (rolled passes, round constants from the table, the full schedule of a block whose constant words are data).
// One lane per element, the library's own flags (tests/probe_kdf/Makefile).
// probekdf_pbkdf2 takes DEVICE pointers laid out as include/p2e.h p2e_pbkdf2_hmac_sha512_batch takes them (bip39 != 0: the
// eight bytes "mnemonic" in front of the salt; salt_offsets == NULL: the empty salt), launches on `stream` and returns at
// once: 0, or the negated HIP error of the launch.  err[i] = 1 (P2E_WIRE_BAD_LENGTH) and zeros for a reversed offset pair or a
// length of 2^32 or more.  Nothing here is linked into the product library.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "../../plonky2-ecdsa_amd/csrc/hd.hpp"

namespace probe_kdf {
using namespace p2e;

// (inlined: a call would pass its arguments through the private segment, csrc/hd.hpp)
// SHA-512 continued from `st` (which has absorbed `done` bytes) over  plen bytes of `prefix` || b[0, blen) || clen bytes of idx
__device__ __forceinline__ Sha512State plain_sha512(Sha512State st, u64 done, u64 prefix, u32 plen, const uint8_t* b, u64 blen, u32 idx, u32 clen) {
    const u64 total = plen + blen + clen;
    const u64 nblocks = (total + 1 + 16 + 127) / 128;
    for (u64 blk = 0; blk < nblocks; blk++) {
        Sha512Block w;
#pragma unroll
        for (int j = 0; j < 16; j++) {
            u64 v = 0;
#pragma unroll 1
            for (int k = 0; k < 8; k++) {
                const u64 pos = 128 * blk + 8 * j + k;
                u32 byte = 0;
                if (pos < plen)
                    byte = (u32)(prefix >> (8 * (7 - pos))) & 0xFFu;
                else if (pos < plen + blen)
                    byte = b[pos - plen];
                else if (pos < total)
                    byte = (idx >> (8 * (3 - (pos - plen - blen)))) & 0xFFu;
                else if (pos == total)
                    byte = 0x80u;
                v = (v << 8) | byte;
            }
            w.w[j] = v;
        }
        if (blk + 1 == nblocks) w.w[15] = 8 * (done + total);
        st = sha512_compress(st, w);
    }
    return st;
}
__device__ __forceinline__ Sha512Block digest_block(const Sha512State& d) {
    Sha512Block b;
#pragma unroll
    for (int j = 0; j < 16; j++) b.w[j] = j < 8 ? d.h[j & 7] : 0ull;
    b.w[8] = 0x8000000000000000ull;
    b.w[15] = 8 * (128 + 64);
    return b;
}

__global__ __launch_bounds__(256) void k_probe_pbkdf2(int bip39, const uint8_t* password, const uint64_t* pw_offsets, int pw_bcast,
                                                      const uint8_t* salt, const uint64_t* salt_offsets, int salt_bcast, u32 iterations,
                                                      u32 dk_words, uint8_t* dk, size_t count, uint8_t* err) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    const size_t pi = pw_bcast ? 0 : i, si = salt_bcast ? 0 : i;
    const u64 plo = pw_offsets[pi], phi = pw_offsets[pi + 1];
    const u64 slo = salt_offsets ? salt_offsets[si] : 0, shi = salt_offsets ? salt_offsets[si + 1] : 0;
    const bool bad = phi < plo || phi - plo >= ((u64)1 << 32) || shi < slo || shi - slo >= ((u64)1 << 32);
    Sha512State t;
#pragma unroll
    for (int j = 0; j < 8; j++) t.h[j] = 0;
    if (!bad) {
        const uint8_t* pw = password + plo;
        const u64 pw_len = phi - plo;
        // the key block: the password, or its digest where it is longer than a block
        Sha512Block kb;
        if (pw_len > 128) {
            const Sha512State d = plain_sha512(sha512_iv(), 0, 0, 0, pw, pw_len, 0, 0);
#pragma unroll
            for (int j = 0; j < 16; j++) kb.w[j] = j < 8 ? d.h[j & 7] : 0ull;
        } else {
#pragma unroll
            for (int j = 0; j < 16; j++) {
                u64 v = 0;
#pragma unroll 1
                for (int k = 0; k < 8; k++) v = (v << 8) | ((u64)(8 * j + k) < pw_len ? pw[8 * j + k] : 0u);
                kb.w[j] = v;
            }
        }
        Sha512Block pad = kb;
#pragma unroll
        for (int j = 0; j < 16; j++) pad.w[j] = kb.w[j] ^ HMAC512_IPAD;
        const Sha512State inner = sha512_compress(sha512_iv(), pad);
#pragma unroll
        for (int j = 0; j < 16; j++) pad.w[j] = kb.w[j] ^ HMAC512_OPAD;
        const Sha512State outer = sha512_compress(sha512_iv(), pad);
        // U_1 = HMAC(P, S || INT(1))
        Sha512State u = plain_sha512(inner, 128, 0x6d6e656d6f6e6963ull, bip39 ? 8u : 0u, salt_offsets ? salt + slo : nullptr, shi - slo, 1u, 4u);
        u = sha512_compress(outer, digest_block(u));
        t = u;
        // U_2 .. U_c: the inner and the outer hash of an iteration take turns through one copy of the compression, as in
        // hd.hpp's hmac512_one_block
#pragma unroll 1
        for (u32 trip = 0; trip < 2 * (iterations - 1); trip++) {
            const bool second = (trip & 1u) != 0;
            Sha512State cv;
#pragma unroll
            for (int j = 0; j < 8; j++) cv.h[j] = second ? outer.h[j] : inner.h[j];
            u = sha512_compress(cv, digest_block(u));
            if (second) {
#pragma unroll
                for (int j = 0; j < 8; j++) t.h[j] ^= u.h[j];
            }
        }
    }
    u32* q = reinterpret_cast<u32*>(dk + 4 * (size_t)dk_words * i);
#pragma unroll
    for (int j = 0; j < 16; j++)
        if ((u32)j < dk_words) q[j] = hash_bswap32((j & 1) ? (u32)t.h[j / 2] : (u32)(t.h[j / 2] >> 32));
    err[i] = bad ? 1 : 0;
}
}  // namespace probe_kdf

extern "C" long probekdf_pbkdf2(int bip39, const uint8_t* password, const uint64_t* pw_offsets, size_t n_passwords, const uint8_t* salt,
                                const uint64_t* salt_offsets, size_t n_salts, uint32_t iterations, size_t dk_len, uint8_t* dk, size_t count,
                                uint8_t* err, void* stream) {
    using namespace probe_kdf;
    if (!password || !pw_offsets || !dk || !err || iterations == 0 || dk_len < 4 || dk_len > 64 || dk_len % 4) return -1;
    if ((n_passwords != 1 && n_passwords != count) || (salt_offsets && n_salts != 1 && n_salts != count)) return -1;
    if (count == 0) return 0;
    hipLaunchKernelGGL(k_probe_pbkdf2, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, (hipStream_t)stream, bip39, password, pw_offsets,
                       n_passwords != count ? 1 : 0, salt, salt_offsets, n_salts != count ? 1 : 0, iterations, (u32)(dk_len / 4), dk, count, err);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : -(long)e;
}

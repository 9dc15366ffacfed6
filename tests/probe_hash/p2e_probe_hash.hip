// Test-only probe of the RFC 6979 retry branch (csrc/hash.hpp rfc6979_nonce).
//
// On the real curves a refused candidate has probability about 2^-32 (P-256) or 2^-128 (secp256k1): no input of the
// product's entry points reaches the loop, yet it diverges per lane.  Here the group order is an ARGUMENT, so a synthetic
// order just above 2^255 makes about half of the candidates fail.  One kernel: element i gets
// k = rfc6979_nonce(q, x[i], z[i]) and the number of candidates refused on the way.  All n elements are ONE launch, so
// retrying and finished lanes share waves.  The file builds twice (tests/probe_hash/Makefile):
//   libp2e_probe_hash.so       hipcc, the library's own flags;
//   libp2e_probe_hash_host.so  g++ -x c++: the same body through a plain loop.
// Arguments are host pointers: 32-byte little-endian values (q: one, x and z: n), rejected: n u32.  Returns 0, or the
// negated HIP error.  Nothing here is linked into the product library.
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#endif
#include <cstddef>
#include <cstdint>

#include "../../plonky2-ecdsa_amd/csrc/hash.hpp"

namespace probe_hash {
using namespace p2e;

P2E_HD void body(const U256& q, const uint8_t* x32, const uint8_t* z32, uint8_t* k32, uint32_t* rejected, size_t i) {
    u32 refused = 0;
    hash_store_packed(k32, i, rfc6979_nonce(q, hash_load_packed(x32, i), hash_load_packed(z32, i), &refused));
    rejected[i] = refused;
}

#if defined(__HIPCC__)
__global__ __launch_bounds__(256) void k_probe_nonce(U256 q, const uint8_t* x32, const uint8_t* z32, uint8_t* k32, uint32_t* rejected,
                                                     size_t n) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) body(q, x32, z32, k32, rejected, i);
}
#endif
}  // namespace probe_hash

extern "C" long probeh_nonce(const uint8_t* q32, const uint8_t* x32, const uint8_t* z32, uint8_t* k32, uint32_t* rejected, size_t n) {
    using namespace probe_hash;
    if (!q32 || !x32 || !z32 || !k32 || !rejected) return -1;
    if (n == 0) return 0;
    const U256 q = hash_load_packed(q32, 0);
#if defined(__HIPCC__)
    uint8_t* d = nullptr;   // x | z | k | rejected
    hipError_t e = hipMalloc(&d, 100 * n);
    if (e != hipSuccess) return -(long)e;
    uint8_t *dx = d, *dz = d + 32 * n, *dk = d + 64 * n;
    uint32_t* dr = reinterpret_cast<uint32_t*>(d + 96 * n);
    e = hipMemcpy(dx, x32, 32 * n, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(dz, z32, 32 * n, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_probe_nonce, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, q, dx, dz, dk, dr, n);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(k32, dk, 32 * n, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(rejected, dr, 4 * n, hipMemcpyDeviceToHost);
    (void)hipFree(d);
    return e == hipSuccess ? 0 : -(long)e;
#else
    for (size_t i = 0; i < n; i++) body(q, x32, z32, k32, rejected, i);
    return 0;
#endif
}

// Test-only probe of the arithmetic behind the DLEQ hashes (csrc/dleq.hpp dleq_prove_with_nonce, dleq_verify_points).
//
// Through the product's entry points k and e are SHA-256 outputs: no input reaches k = 0, e = 0, e >= n or a neutral R1 / R2.
// Here they are ARGUMENTS.  One kernel each, one lane per element, the library's own flags (tests/probe_dleq/Makefile); the CPU
// build of the same functions is tests/emu_dleq.  Arguments are host pointers, laid out as tests/emu_dleq's
// emud_prove_with_nonce and emud_verify_points take them.  Returns 0, or the negated HIP error.  Nothing here is linked into the
// product library.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../plonky2-ecdsa_amd/csrc/consts.hpp"
#include "../../plonky2-ecdsa_amd/csrc/dleq.hpp"

namespace probe_dleq {
using namespace p2e;

__device__ __forceinline__ Aff load_aff(const uint8_t* x32, const uint8_t* y32, size_t i) {
    Aff P;
    P.x = load_packed(x32, i), P.y = load_packed(y32, i);
    return P;
}
__global__ __launch_bounds__(256) void k_probe_prove_with_nonce(const Aff* T, const uint8_t* a_sk32, const uint8_t* ax32, const uint8_t* ay32,
                                                                const uint8_t* bx32, const uint8_t* by32, const uint8_t* cx32, const uint8_t* cy32,
                                                                const uint8_t* k32, const uint8_t* msg32, uint8_t* proof64, uint8_t* code, size_t n) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    U256 e = u256_zero(), s = u256_zero();
    const U256 msg = msg32 ? schnorr_load_be(msg32 + 32 * i) : u256_zero();
    const uint8_t c = dleq_prove_with_nonce(T, load_packed(a_sk32, i), load_aff(ax32, ay32, i), load_aff(bx32, by32, i), load_aff(cx32, cy32, i),
                                            schnorr_load_be(k32 + 32 * i), msg32 != nullptr, msg, e, s);
    if (c) e = s = u256_zero();
    code[i] = c;
    schnorr_store_be(proof64 + 64 * i, e);
    schnorr_store_be(proof64 + 64 * i + 32, s);
}
__global__ __launch_bounds__(256) void k_probe_verify_points(const Aff* T, const uint8_t* ax32, const uint8_t* ay32, const uint8_t* bx32,
                                                             const uint8_t* by32, const uint8_t* cx32, const uint8_t* cy32, const uint8_t* e32,
                                                             const uint8_t* s32, uint8_t* r1x32, uint8_t* r1y32, uint8_t* r2x32, uint8_t* r2y32,
                                                             uint8_t* ok, size_t n) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    Aff R1, R2;
    const bool good = dleq_verify_points(T, load_aff(ax32, ay32, i), load_aff(bx32, by32, i), load_aff(cx32, cy32, i), schnorr_load_be(e32 + 32 * i),
                                         schnorr_load_be(s32 + 32 * i), R1, R2);
    if (!good) R1.x = R1.y = R2.x = R2.y = u256_zero();
    ok[i] = good ? 1 : 0;
    store_packed(r1x32, i, R1.x), store_packed(r1y32, i, R1.y);
    store_packed(r2x32, i, R2.x), store_packed(r2y32, i, R2.y);
}

// device copies of host arrays, freed together; the first failure sticks
struct Arena {
    hipError_t e = hipSuccess;
    std::vector<void*> held;
    uint8_t* get(size_t bytes) {
        void* d = nullptr;
        if (e == hipSuccess) e = hipMalloc(&d, bytes ? bytes : 1);
        if (d) held.push_back(d);
        return static_cast<uint8_t*>(d);
    }
    uint8_t* up(const void* src, size_t bytes) {
        if (!src) return nullptr;
        uint8_t* d = get(bytes);
        if (e == hipSuccess && bytes) e = hipMemcpy(d, src, bytes, hipMemcpyHostToDevice);
        return d;
    }
    void down(void* dst, const void* src, size_t bytes) {
        if (e == hipSuccess) e = hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost);
    }
    const Aff* table() {
        const std::vector<Aff>& tab = host::consts().fbtab;   // the generator table the library uploads
        return reinterpret_cast<const Aff*>(up(tab.data(), tab.size() * sizeof(Aff)));
    }
    void finish() {
        if (e == hipSuccess) e = hipGetLastError();
        if (e == hipSuccess) e = hipDeviceSynchronize();
    }
    ~Arena() {
        for (void* d : held) (void)hipFree(d);
    }
};
}  // namespace probe_dleq

extern "C" long probedleq_prove_with_nonce(const uint8_t* a_sk32, const uint8_t* ax32, const uint8_t* ay32, const uint8_t* bx32, const uint8_t* by32,
                                           const uint8_t* cx32, const uint8_t* cy32, const uint8_t* k32, const uint8_t* msg32 /* nullable */,
                                           uint8_t* proof64, uint8_t* code, size_t n) {
    using namespace probe_dleq;
    if (!a_sk32 || !ax32 || !ay32 || !bx32 || !by32 || !cx32 || !cy32 || !k32 || !proof64 || !code) return -1;
    if (n == 0) return 0;
    Arena a;
    const Aff* T = a.table();
    const uint8_t *sk = a.up(a_sk32, 32 * n), *ax = a.up(ax32, 32 * n), *ay = a.up(ay32, 32 * n), *bx = a.up(bx32, 32 * n), *by = a.up(by32, 32 * n);
    const uint8_t *cx = a.up(cx32, 32 * n), *cy = a.up(cy32, 32 * n), *k = a.up(k32, 32 * n), *msg = a.up(msg32, 32 * n);
    uint8_t *d_proof = a.get(64 * n), *d_code = a.get(n);
    if (a.e == hipSuccess) {
        hipLaunchKernelGGL(k_probe_prove_with_nonce, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, T, sk, ax, ay, bx, by, cx, cy, k, msg, d_proof,
                           d_code, n);
        a.finish();
    }
    a.down(proof64, d_proof, 64 * n), a.down(code, d_code, n);
    return a.e == hipSuccess ? 0 : -(long)a.e;
}

extern "C" long probedleq_verify_points(const uint8_t* ax32, const uint8_t* ay32, const uint8_t* bx32, const uint8_t* by32, const uint8_t* cx32,
                                        const uint8_t* cy32, const uint8_t* e32, const uint8_t* s32, uint8_t* r1x32, uint8_t* r1y32, uint8_t* r2x32,
                                        uint8_t* r2y32, uint8_t* ok, size_t n) {
    using namespace probe_dleq;
    if (!ax32 || !ay32 || !bx32 || !by32 || !cx32 || !cy32 || !e32 || !s32 || !r1x32 || !r1y32 || !r2x32 || !r2y32 || !ok) return -1;
    if (n == 0) return 0;
    Arena a;
    const Aff* T = a.table();
    const uint8_t *ax = a.up(ax32, 32 * n), *ay = a.up(ay32, 32 * n), *bx = a.up(bx32, 32 * n), *by = a.up(by32, 32 * n), *cx = a.up(cx32, 32 * n);
    const uint8_t *cy = a.up(cy32, 32 * n), *e = a.up(e32, 32 * n), *s = a.up(s32, 32 * n);
    uint8_t *d1x = a.get(32 * n), *d1y = a.get(32 * n), *d2x = a.get(32 * n), *d2y = a.get(32 * n), *d_ok = a.get(n);
    if (a.e == hipSuccess) {
        hipLaunchKernelGGL(k_probe_verify_points, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, T, ax, ay, bx, by, cx, cy, e, s, d1x, d1y, d2x, d2y,
                           d_ok, n);
        a.finish();
    }
    a.down(r1x32, d1x, 32 * n), a.down(r1y32, d1y, 32 * n), a.down(r2x32, d2x, 32 * n), a.down(r2y32, d2y, 32 * n), a.down(ok, d_ok, n);
    return a.e == hipSuccess ? 0 : -(long)a.e;
}

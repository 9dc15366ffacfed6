// Test-only probe of the arithmetic behind Taproot's tweak hash (csrc/taproot.hpp taproot_finish_pub, taproot_finish_sec).
//
// Through the product's entry points t is a SHA-256 output: no input reaches t >= n, t = 0, t G = P (the doubling),
// t G = -P (the neutral element) or d + t = 0.  Here t is an ARGUMENT.  One kernel per body, one lane per element, the
// library's own flags (tests/probe_taproot/Makefile); the CPU build of the same bodies is tests/emu_taproot.
// Arguments are host pointers to 32-byte BIG-endian values; code: n bytes, the WIRE_* code; outputs are zeros where the code
// is not 0.  Returns 0, or the negated HIP error.  Nothing here is linked into the product library.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "../../plonky2-ecdsa_amd/csrc/consts.hpp"
#include "../../plonky2-ecdsa_amd/csrc/taproot.hpp"

namespace probe_taproot {
using namespace p2e;

// pk32: an x-only key that is on the curve (code 0xFF where it is not: the probe's own, no WIRE_* code)
__global__ __launch_bounds__(256) void k_probe_finish_pub(const Aff* T, const uint8_t* pk32, const uint8_t* t32, uint8_t* out32, uint8_t* parity,
                                                          uint8_t* code, size_t n) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    Aff P;
    U256 qx = u256_zero();
    u32 par = 0;
    uint8_t e = 0xFF;
    if (!schnorr_lift_x(schnorr_load_be(pk32 + 32 * i), false, P)) e = taproot_finish_pub(T, P, schnorr_load_be(t32 + 32 * i), qx, par);
    schnorr_store_be(out32 + 32 * i, e ? u256_zero() : qx);
    parity[i] = e ? 0 : (uint8_t)par;
    code[i] = e;
}
__global__ __launch_bounds__(256) void k_probe_finish_sec(const uint8_t* d32, const uint8_t* t32, uint8_t* out32, uint8_t* code, size_t n) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    U256 out = u256_zero();
    const uint8_t e = taproot_finish_sec(schnorr_load_be(d32 + 32 * i), schnorr_load_be(t32 + 32 * i), out);
    schnorr_store_be(out32 + 32 * i, e ? u256_zero() : out);
    code[i] = e;
}

// `count` arrays of 32 n bytes each, then two arrays of n bytes, in one allocation
struct Block {
    uint8_t* d = nullptr;
    size_t n;
    hipError_t e;
    Block(size_t n_, int count) : n(n_) { e = hipMalloc(&d, (size_t)count * 32 * n + 2 * n); }
    ~Block() { (void)hipFree(d); }
    uint8_t* at(int k) const { return d + (size_t)k * 32 * n; }
    void up(int k, const uint8_t* src) {
        if (e == hipSuccess) e = hipMemcpy(at(k), src, 32 * n, hipMemcpyHostToDevice);
    }
    void down(const uint8_t* from, uint8_t* dst, size_t bytes) {
        if (e == hipSuccess) e = hipMemcpy(dst, from, bytes, hipMemcpyDeviceToHost);
    }
    void ran() {
        if (e == hipSuccess) e = hipGetLastError();
        if (e == hipSuccess) e = hipDeviceSynchronize();
    }
};
}  // namespace probe_taproot

extern "C" long probetr_finish_pub(const uint8_t* pk32, const uint8_t* t32, uint8_t* out32, uint8_t* parity, uint8_t* code, size_t n) {
    using namespace probe_taproot;
    if (!pk32 || !t32 || !out32 || !parity || !code) return -1;
    if (n == 0) return 0;
    const std::vector<Aff>& tab = host::consts().fbtab;   // the generator table the library uploads
    Aff* T = nullptr;
    hipError_t e = hipMalloc(&T, tab.size() * sizeof(Aff));
    if (e != hipSuccess) return -(long)e;
    e = hipMemcpy(T, tab.data(), tab.size() * sizeof(Aff), hipMemcpyHostToDevice);
    Block b(n, 3);   // pk | t | out | parity | code
    if (e != hipSuccess) b.e = e;
    b.up(0, pk32), b.up(1, t32);
    uint8_t *par = b.at(3), *cod = b.at(3) + n;
    if (b.e == hipSuccess) {
        hipLaunchKernelGGL(k_probe_finish_pub, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, T, b.at(0), b.at(1), b.at(2), par, cod, n);
        b.ran();
    }
    b.down(b.at(2), out32, 32 * n), b.down(par, parity, n), b.down(cod, code, n);
    (void)hipFree(T);
    return b.e == hipSuccess ? 0 : -(long)b.e;
}
extern "C" long probetr_finish_sec(const uint8_t* d32, const uint8_t* t32, uint8_t* out32, uint8_t* code, size_t n) {
    using namespace probe_taproot;
    if (!d32 || !t32 || !out32 || !code) return -1;
    if (n == 0) return 0;
    Block b(n, 3);   // d | t | out | code
    b.up(0, d32), b.up(1, t32);
    if (b.e == hipSuccess) {
        hipLaunchKernelGGL(k_probe_finish_sec, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, b.at(0), b.at(1), b.at(2), b.at(3), n);
        b.ran();
    }
    b.down(b.at(2), out32, 32 * n), b.down(b.at(3), code, n);
    return b.e == hipSuccess ? 0 : -(long)b.e;
}

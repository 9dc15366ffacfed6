// Test-only probe of the arithmetic behind BIP-32's hash (csrc/hd.hpp bip32_finish_priv, bip32_finish_pub).
//
// Through the product's entry points I_L is an HMAC-SHA512 output: no input reaches I_L >= n, I_L = 0, a child key of zero,
// a neutral child point or the doubling I_L G = K_par.  Here I_L is an ARGUMENT.  One kernel per body, one lane per element,
// the library's own flags (tests/probe_hd/Makefile); the CPU build of the same bodies is tests/emu_hd.
// Arguments are host pointers to 32-byte little-endian values; code: n bytes, the WIRE_* code; outputs are zeros where the
// code is not 0.  Returns 0, or the negated HIP error.  Nothing here is linked into the product library.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "../../plonky2-ecdsa_amd/csrc/consts.hpp"
#include "../../plonky2-ecdsa_amd/csrc/hd.hpp"

namespace probe_hd {
using namespace p2e;

__global__ __launch_bounds__(256) void k_probe_finish_priv(const uint8_t* il32, const uint8_t* k32, uint8_t* out32, uint8_t* code, size_t n) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    U256 kc = u256_zero();
    const uint8_t e = bip32_finish_priv(load_packed(il32, i), load_packed(k32, i), kc);
    hd_store_key(out32, i, kc, e != 0);
    code[i] = e;
}
__global__ __launch_bounds__(256) void k_probe_finish_pub(const Aff* T, const uint8_t* il32, const uint8_t* px32, const uint8_t* py32,
                                                          uint8_t* outx32, uint8_t* outy32, uint8_t* code, size_t n) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    Aff K, C;
    K.x = load_packed(px32, i), K.y = load_packed(py32, i);
    C.x = C.y = u256_zero();
    const uint8_t e = bip32_finish_pub(T, load_packed(il32, i), K, C);
    hd_store_key(outx32, i, C.x, e != 0);
    hd_store_key(outy32, i, C.y, e != 0);
    code[i] = e;
}

// `count` arrays of 32 n bytes each, then n code bytes, in one allocation
struct Block {
    uint8_t* d = nullptr;
    size_t n;
    hipError_t e;
    Block(size_t n_, int count) : n(n_) { e = hipMalloc(&d, (size_t)count * 32 * n + n); }
    ~Block() { (void)hipFree(d); }
    uint8_t* at(int k) const { return d + (size_t)k * 32 * n; }
    void up(int k, const uint8_t* src) {
        if (e == hipSuccess) e = hipMemcpy(at(k), src, 32 * n, hipMemcpyHostToDevice);
    }
    void down(int k, uint8_t* dst, size_t bytes) {
        if (e == hipSuccess) e = hipMemcpy(dst, at(k), bytes, hipMemcpyDeviceToHost);
    }
    void ran() {
        if (e == hipSuccess) e = hipGetLastError();
        if (e == hipSuccess) e = hipDeviceSynchronize();
    }
};
}  // namespace probe_hd

extern "C" long probehd_finish_priv(const uint8_t* il32, const uint8_t* k32, uint8_t* out32, uint8_t* code, size_t n) {
    using namespace probe_hd;
    if (!il32 || !k32 || !out32 || !code) return -1;
    if (n == 0) return 0;
    Block b(n, 3);   // il | k | out | code
    b.up(0, il32), b.up(1, k32);
    if (b.e == hipSuccess) {
        hipLaunchKernelGGL(k_probe_finish_priv, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, b.at(0), b.at(1), b.at(2), b.at(3), n);
        b.ran();
    }
    b.down(2, out32, 32 * n), b.down(3, code, n);
    return b.e == hipSuccess ? 0 : -(long)b.e;
}
extern "C" long probehd_finish_pub(const uint8_t* il32, const uint8_t* px32, const uint8_t* py32, uint8_t* outx32, uint8_t* outy32,
                                   uint8_t* code, size_t n) {
    using namespace probe_hd;
    if (!il32 || !px32 || !py32 || !outx32 || !outy32 || !code) return -1;
    if (n == 0) return 0;
    const std::vector<Aff>& tab = host::consts().fbtab;   // the generator table the library uploads
    Aff* T = nullptr;
    hipError_t e = hipMalloc(&T, tab.size() * sizeof(Aff));
    if (e != hipSuccess) return -(long)e;
    e = hipMemcpy(T, tab.data(), tab.size() * sizeof(Aff), hipMemcpyHostToDevice);
    Block b(n, 5);   // il | x | y | outx | outy | code
    if (e != hipSuccess) b.e = e;
    b.up(0, il32), b.up(1, px32), b.up(2, py32);
    if (b.e == hipSuccess) {
        hipLaunchKernelGGL(k_probe_finish_pub, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, T, b.at(0), b.at(1), b.at(2), b.at(3), b.at(4),
                           b.at(5), n);
        b.ran();
    }
    b.down(3, outx32, 32 * n), b.down(4, outy32, 32 * n), b.down(5, code, n);
    (void)hipFree(T);
    return b.e == hipSuccess ? 0 : -(long)b.e;
}

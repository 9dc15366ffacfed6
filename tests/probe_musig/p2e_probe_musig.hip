// Test-only probe of the arithmetic behind the MuSig2 hashes (csrc/musig.hpp musig_term / musig_key_agg_finish and
// musig_session_finish).
//
// Through the product's entry points a key's coefficient and the nonce coefficient b are SHA-256 outputs: no input reaches a
// key sum at infinity or R_1 = -b R_2.  Here both are ARGUMENTS.  Two kernels, one lane per element, the library's own flags
// (tests/probe_musig/Makefile); the CPU build of the same bodies is tests/emu_musig.  Arguments are host pointers, laid out as
// tests/emu_musig's emumusig_forced_key_agg and emumusig_forced_session take them.  Returns 0, or the negated HIP error.  Nothing
// here is linked into the product library.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../plonky2-ecdsa_amd/csrc/consts.hpp"
#include "../../plonky2-ecdsa_amd/csrc/musig.hpp"

namespace probe_musig {
using namespace p2e;

// session i sums coef32[j] P_j over its keys (at most 16: the caller checks), which must be valid
__global__ __launch_bounds__(256) void k_probe_key_agg(const uint8_t* pkx32, const uint8_t* pky32, const uint8_t* coef32, const uint64_t* key_offsets,
                                                       uint8_t* code, uint8_t* qx32, uint8_t* qy32, size_t n) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    SignSum<MusigCV> sum = msm_neutral<MusigCV>();
    for (uint64_t j = key_offsets[i]; j < key_offsets[i + 1]; j++)
        sum = msm_add<MusigCV, false>(sum, musig_term(musig_load_point(pkx32, pky32, (size_t)j), fe_canon<MusigCV::Fn>(schnorr_load_be(coef32 + 32 * j))));
    MusigKeyAgg r;
    r.Q.x = r.Q.y = u256_zero();
    const uint8_t e = musig_key_agg_finish(sum, r);
    code[i] = e;
    hd_store_key(qx32, i, r.Q.x, e != 0);
    hd_store_key(qy32, i, r.Q.y, e != 0);
}
__global__ __launch_bounds__(256) void k_probe_session(const Aff* T, const uint8_t* keyagg192, const uint8_t* aggnonce128, const uint8_t* msg32,
                                                       const uint8_t* b32, uint8_t* code, uint8_t* session128, size_t n) {
    __shared__ u32 lds[MUSIG_PARK_WORDS][256];
    MusigParkLds park{&lds[0][threadIdx.x]};
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const MusigKeyAgg ka = musig_load_keyagg(keyagg192, i);
    const Aff R1 = musig_load_nonce(aggnonce128, i, 0), R2 = musig_load_nonce(aggnonce128, i, 1);
    const bool n1 = u256_is_zero(R1.x) && u256_is_zero(R1.y), n2 = u256_is_zero(R2.x) && u256_is_zero(R2.y);
    MusigSession r;
    r.b = r.e = r.rx = u256_zero();
    r.flags = 0;
    const uint8_t e = musig_session_finish(park, T, ka.Q.x, R1, n1, R2, n2, fe_canon<MusigCV::Fn>(schnorr_load_be(b32 + 32 * i)),
                                           schnorr_load_be(msg32 + 32 * i), r);
    code[i] = e;
    musig_store_session(session128, i, r, e != 0);
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
        uint8_t* d = get(bytes);
        if (e == hipSuccess && bytes) e = hipMemcpy(d, src, bytes, hipMemcpyHostToDevice);
        return d;
    }
    void down(void* dst, const void* src, size_t bytes) {
        if (e == hipSuccess) e = hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost);
    }
    ~Arena() {
        for (void* d : held) (void)hipFree(d);
    }
};
}  // namespace probe_musig

extern "C" long probemusig_forced_key_agg(const uint8_t* pkx32, const uint8_t* pky32, const uint8_t* coef32, const uint64_t* key_offsets,
                                          uint8_t* code, uint8_t* qx32, uint8_t* qy32, size_t n) {
    using namespace probe_musig;
    if (!pkx32 || !pky32 || !coef32 || !key_offsets || !code || !qx32 || !qy32) return -1;
    if (n == 0) return 0;
    if (n > 4096 || key_offsets[0] != 0) return -1;
    for (size_t i = 0; i < n; i++)   // every offset inside the arrays that are copied, every session short
        if (key_offsets[i + 1] < key_offsets[i] || key_offsets[i + 1] - key_offsets[i] > 16) return -1;
    const size_t total = (size_t)key_offsets[n];
    Arena a;
    const uint8_t *x = a.up(pkx32, 32 * total), *y = a.up(pky32, 32 * total), *cf = a.up(coef32, 32 * total);
    const uint64_t* off = reinterpret_cast<const uint64_t*>(a.up(key_offsets, 8 * (n + 1)));
    uint8_t *d_code = a.get(n), *d_x = a.get(32 * n), *d_y = a.get(32 * n);
    if (a.e == hipSuccess) {
        hipLaunchKernelGGL(k_probe_key_agg, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, x, y, cf, off, d_code, d_x, d_y, n);
        a.e = hipGetLastError();
        if (a.e == hipSuccess) a.e = hipDeviceSynchronize();
    }
    a.down(code, d_code, n), a.down(qx32, d_x, 32 * n), a.down(qy32, d_y, 32 * n);
    return a.e == hipSuccess ? 0 : -(long)a.e;
}

extern "C" long probemusig_forced_session(const uint8_t* keyagg192, const uint8_t* aggnonce128, const uint8_t* msg32, const uint8_t* b32,
                                          uint8_t* code, uint8_t* session128, size_t n) {
    using namespace probe_musig;
    if (!keyagg192 || !aggnonce128 || !msg32 || !b32 || !code || !session128) return -1;
    if (n == 0) return 0;
    if (n > 4096) return -1;
    const std::vector<Aff>& tab = host::consts().fbtab;   // the generator table the library uploads
    Arena a;
    const Aff* T = reinterpret_cast<const Aff*>(a.up(tab.data(), tab.size() * sizeof(Aff)));
    const uint8_t *ka = a.up(keyagg192, 192 * n), *agg = a.up(aggnonce128, 128 * n), *msg = a.up(msg32, 32 * n), *b = a.up(b32, 32 * n);
    uint8_t *d_code = a.get(n), *d_ses = a.get(128 * n);
    if (a.e == hipSuccess) {
        hipLaunchKernelGGL(k_probe_session, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, T, ka, agg, msg, b, d_code, d_ses, n);
        a.e = hipGetLastError();
        if (a.e == hipSuccess) a.e = hipDeviceSynchronize();
    }
    a.down(code, d_code, n), a.down(session128, d_ses, 128 * n);
    return a.e == hipSuccess ? 0 : -(long)a.e;
}

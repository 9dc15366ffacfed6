// Test-only probe of the arithmetic behind the silent-payment tweak hash (csrc/sp.hpp sp_finish).
//
// Through the product's entry points t is a SHA-256 output: no input reaches t >= n, t = 0, t G = B_spend (the doubling),
// t G = -B_spend (the neutral element), a neutral P_k + L_j or L_j = P_k.  Here t is an ARGUMENT.  One kernel, one lane per
// element, the library's own flags (tests/probe_sp/Makefile); the CPU build of the same body is tests/emu_sp.
// Arguments are host pointers, laid out as tests/emu_sp's emusp_finish takes them: element i has its own B_spend (little-endian
// x, y), its own n_labels labels, its own t (32 big-endian bytes) and its own n_out outputs.  code: the WIRE_* code; found, and
// where it is 1 hit_output / hit_label; zeros otherwise.  Returns 0, or the negated HIP error.  Nothing here is linked into the
// product library.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../plonky2-ecdsa_amd/csrc/consts.hpp"
#include "../../plonky2-ecdsa_amd/csrc/sp.hpp"

namespace probe_sp {
using namespace p2e;

__global__ __launch_bounds__(256) void k_probe_finish(const Aff* T, const uint8_t* bx32, const uint8_t* by32, const uint8_t* label_x32,
                                                      const uint8_t* label_y32, u32 n_labels, const uint8_t* t32, const uint8_t* outputs32,
                                                      u32 n_out, uint8_t* code, uint8_t* found, uint32_t* hit_output, uint8_t* hit_label, size_t n) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    Aff B;
    B.x = load_packed(bx32, i), B.y = load_packed(by32, i);
    SpHits hits = sp_no_hits();
    bool f = false;
    code[i] = sp_finish(T, B, label_x32 + 32 * (size_t)n_labels * i, label_y32 + 32 * (size_t)n_labels * i, n_labels, schnorr_load_be(t32 + 32 * i),
                        outputs32 + 32 * (size_t)n_out * i, n_out, hits, f);
    found[i] = f ? 1 : 0;
    hit_output[i] = f ? hits.out[0] : 0u;
    hit_label[i] = f ? (uint8_t)hits.label[0] : (uint8_t)0;
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
}  // namespace probe_sp

extern "C" long probesp_finish(const uint8_t* bx32, const uint8_t* by32, const uint8_t* label_x32, const uint8_t* label_y32, size_t n_labels,
                               const uint8_t* t32, const uint8_t* outputs32, size_t n_out, uint8_t* code, uint8_t* found, uint32_t* hit_output,
                               uint8_t* hit_label, size_t n) {
    using namespace probe_sp;
    if (!bx32 || !by32 || !label_x32 || !label_y32 || !t32 || !outputs32 || !code || !found || !hit_output || !hit_label) return -1;
    if (n_labels > SP_MAX_LABELS || n_out > 64) return -1;
    if (n == 0) return 0;
    const std::vector<Aff>& tab = host::consts().fbtab;   // the generator table the library uploads
    Arena a;
    const Aff* T = reinterpret_cast<const Aff*>(a.up(tab.data(), tab.size() * sizeof(Aff)));
    const uint8_t *bx = a.up(bx32, 32 * n), *by = a.up(by32, 32 * n), *lx = a.up(label_x32, 32 * n_labels * n), *ly = a.up(label_y32, 32 * n_labels * n);
    const uint8_t *t = a.up(t32, 32 * n), *outs = a.up(outputs32, 32 * n_out * n);
    uint8_t *d_code = a.get(n), *d_found = a.get(n), *d_label = a.get(n);
    uint32_t* d_out = reinterpret_cast<uint32_t*>(a.get(4 * n));
    if (a.e == hipSuccess) {
        hipLaunchKernelGGL(k_probe_finish, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, T, bx, by, lx, ly, (u32)n_labels, t, outs, (u32)n_out,
                           d_code, d_found, d_out, d_label, n);
        a.e = hipGetLastError();
        if (a.e == hipSuccess) a.e = hipDeviceSynchronize();
    }
    a.down(code, d_code, n), a.down(found, d_found, n), a.down(hit_output, d_out, 4 * n), a.down(hit_label, d_label, n);
    return a.e == hipSuccess ? 0 : -(long)a.e;
}

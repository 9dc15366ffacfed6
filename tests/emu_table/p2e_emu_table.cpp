// CPU harness of the point tables (test infrastructure only): the bodies of csrc/point_table.hpp -- the two build steps and
// the three calls -- run per lane, compiled with g++ against the library's headers, on either curve.  The library's host
// side is mirrored as far as it decides bytes: create builds nothing when a point is rejected, and a zero Z in a row
// rejects its point.  A table is a plain array of m * 66 * 16 entries of 64 bytes, exactly the device layout, so a lane
// that read past it would read past the caller's allocation.
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../plonky2-ecdsa_amd/csrc/consts.hpp"
#include "../../plonky2-ecdsa_amd/csrc/curve_program.hpp"
#include "../../plonky2-ecdsa_amd/csrc/point_table.hpp"

using namespace p2e;

namespace {
template <class CV>
const Aff* generator_table();
template <>
const Aff* generator_table<Secp256k1>() {
    return host::consts().fbtab.data();
}
template <>
const Aff* generator_table<P256>() {
    static const std::vector<Aff> t = host::fixed_base_table_cv<P256>(host::generator_cv<P256>());
    return t.data();
}
template <class CV>
long run_build(const uint8_t* px, const uint8_t* py, size_t m, uint8_t* tab, uint8_t* perr) {
    typedef typename SignArith<CV>::Pt Pt;
    std::vector<Pt> pow(m * FB_WINDOWS);
    std::vector<uint8_t> code(m);
    long bad = 0;
#pragma omp parallel for schedule(dynamic, 1) reduction(+ : bad)
    for (long long j = 0; j < (long long)m; j++) {
        code[j] = body_table_powers<CV>(px, py, pow.data(), (size_t)j);
        bad += code[j] != 0;
    }
    if (bad == 0) {
        const long long rows = (long long)(m * FB_WINDOWS);
#pragma omp parallel for schedule(dynamic, 4)
        for (long long g = 0; g < rows; g++)
            if (!body_table_row<CV>(pow.data(), reinterpret_cast<Aff*>(tab), (size_t)g)) {
#pragma omp critical
                code[(size_t)g / FB_WINDOWS] = WIRE_NOT_ON_CURVE;
            }
        for (size_t j = 0; j < m; j++) bad += code[j] != 0;
    }
    if (perr) memcpy(perr, code.data(), m);
    return bad;
}
template <class CV>
long run_call(int what, const uint8_t* tab, const uint32_t* idx, uint32_t m, const uint8_t* a, const uint8_t* b, const uint8_t* s,
              uint8_t* out1, uint8_t* out2, size_t n, uint8_t* err) {
    const Aff* G = generator_table<CV>();
    const Aff* T = reinterpret_cast<const Aff*>(tab);
    long bad = 0;
#pragma omp parallel for schedule(dynamic, 16) reduction(+ : bad)
    for (long long i = 0; i < (long long)n; i++) {
        if (what == 0)
            err[i] = body_table_mul<CV>(T, idx, m, b, out1, out2, (size_t)i);
        else if (what == 1)
            err[i] = body_table_lincomb<CV>(G, T, idx, m, a, b, out1, out2, (size_t)i);
        else
            err[i] = body_table_verify<CV>(G, T, idx, m, a, b, s, out1, (size_t)i);
        bad += err[i] != 0;
    }
    return bad;
}
}  // namespace

extern "C" size_t emut_table_bytes(size_t m) { return m * TABLE_POINT_ENTRIES * sizeof(Aff); }
// p2e_point_table_create: returns the number of rejected points (then `tab` holds nothing meaningful), -1 on misuse
extern "C" long emut_build(int curve, const uint8_t* px, const uint8_t* py, size_t m, uint8_t* tab, uint8_t* perr) {
    if ((curve != 0 && curve != 1) || m < 1 || m > TABLE_MAX_POINTS) return -1;
    return curve == 0 ? run_build<Secp256k1>(px, py, m, tab, perr) : run_build<P256>(px, py, m, tab, perr);
}
// the generator's table as the library uploads it (fixed_base_table_cv), emut_table_bytes(1) bytes
extern "C" void emut_generator_table(int curve, uint8_t* out) {
    memcpy(out, curve == 0 ? generator_table<Secp256k1>() : generator_table<P256>(), emut_table_bytes(1));
}
// what: 0 = mul (b = k32), 1 = lincomb (a32, b32), 2 = verify (a = msg32, b = r32, s = s32; out1 = valid, out2 unused)
extern "C" long emut_call(int curve, int what, const uint8_t* tab, const uint32_t* idx, uint32_t m, const uint8_t* a, const uint8_t* b,
                          const uint8_t* s, uint8_t* out1, uint8_t* out2, size_t n, uint8_t* err) {
    if ((curve != 0 && curve != 1) || what < 0 || what > 2) return -1;
    return curve == 0 ? run_call<Secp256k1>(what, tab, idx, m, a, b, s, out1, out2, n, err)
                      : run_call<P256>(what, tab, idx, m, a, b, s, out1, out2, n, err);
}

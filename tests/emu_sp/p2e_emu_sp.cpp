// CPU harness of the silent-payment layer (test infrastructure only): the bodies of csrc/sp.hpp run per element, compiled with
// g++ against the library's headers and the generator table the library uploads.
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../plonky2-ecdsa_amd/csrc/consts.hpp"
#include "../../plonky2-ecdsa_amd/csrc/sp.hpp"

using namespace p2e;

namespace {
const Aff* gen_table() { return host::consts().fbtab.data(); }
}  // namespace

// the three constant chaining values, 8 words each
extern "C" void emusp_midstates(uint32_t* out24) {
    for (int t = 0; t < 3; t++) {
        const Sha256State s = sp_midstate(t);
        for (int j = 0; j < 8; j++) out24[8 * t + j] = s.h[j];
    }
}
// One step of the scan loop behind ANY t, per element, nothing recorded before it: element i has its own B_spend, its own
// n_labels labels, its own t (32 big-endian bytes) and its own n_out outputs.  code[i]: the WIRE_* code; found[i], and where it
// is 1 hit_output[i] / hit_label[i]; zeros otherwise.
extern "C" void emusp_finish(const uint8_t* bx32, const uint8_t* by32, const uint8_t* label_x32, const uint8_t* label_y32, size_t n_labels,
                             const uint8_t* t32, const uint8_t* outputs32, size_t n_out, uint8_t* code, uint8_t* found, uint32_t* hit_output,
                             uint8_t* hit_label, size_t count) {
    const Aff* T = gen_table();
    for (size_t i = 0; i < count; i++) {
        Aff B;
        B.x = load_packed(bx32, i), B.y = load_packed(by32, i);
        SpHits hits = sp_no_hits();
        bool f = false;
        code[i] = sp_finish(T, B, label_x32 + 32 * n_labels * i, label_y32 + 32 * n_labels * i, (u32)n_labels, schnorr_load_be(t32 + 32 * i),
                            outputs32 + 32 * n_out * i, (u32)n_out, hits, f);
        found[i] = f ? 1 : 0;
        hit_output[i] = f ? hits.out[0] : 0;
        hit_label[i] = f ? (uint8_t)hits.label[0] : 0;
    }
}

extern "C" long emusp_input_hash(const uint8_t* outpoint36, const uint8_t* ax32, const uint8_t* ay32, uint8_t* input_hash32, size_t count,
                                 uint8_t* err) {
    long bad = 0;
#pragma omp parallel for schedule(dynamic, 16) reduction(+ : bad)
    for (long long i = 0; i < (long long)count; i++) {
        err[i] = body_sp_input_hash(outpoint36, ax32, ay32, input_hash32, (size_t)i);
        bad += err[i] != 0;
    }
    return bad;
}
extern "C" long emusp_label(const uint8_t* scan_sk32, const uint32_t* label_index, uint8_t* label_tweak32, uint8_t* label_x32, uint8_t* label_y32,
                            size_t count, uint8_t* err) {
    const Aff* T = gen_table();
    long bad = 0;
#pragma omp parallel for schedule(dynamic, 16) reduction(+ : bad)
    for (long long i = 0; i < (long long)count; i++) {
        err[i] = body_sp_label(T, scan_sk32, label_index, label_tweak32, label_x32, label_y32, (size_t)i);
        bad += err[i] != 0;
    }
    return bad;
}
extern "C" long emusp_send(const uint8_t* a_sk32, const uint8_t* input_hash32, const uint8_t* scan_pkx32, const uint8_t* scan_pky32,
                           const uint8_t* spend_pkx32, const uint8_t* spend_pky32, const uint32_t* k, uint8_t* out_pk32, size_t count,
                           uint8_t* err) {
    const Aff* T = gen_table();
    long bad = 0;
#pragma omp parallel for schedule(dynamic, 4) reduction(+ : bad)
    for (long long i = 0; i < (long long)count; i++) {
        err[i] = body_sp_send(T, a_sk32, input_hash32, scan_pkx32, scan_pky32, spend_pkx32, spend_pky32, k, out_pk32, (size_t)i);
        bad += err[i] != 0;
    }
    return bad;
}
extern "C" long emusp_scan(const uint8_t* scan_sk32, const uint8_t* spend_pkx32, const uint8_t* spend_pky32, const uint8_t* label_x32,
                           const uint8_t* label_y32, size_t n_labels, const uint8_t* ax32, const uint8_t* ay32, const uint8_t* input_hash32,
                           const uint8_t* outputs32, const uint64_t* out_offsets, size_t max_hits, uint8_t* n_hits, uint32_t* hit_output,
                           uint8_t* hit_label, uint8_t* hit_tweak32, size_t count, uint8_t* err) {
    if (max_hits < 1 || max_hits > SP_MAX_HITS || n_labels > SP_MAX_LABELS) return -1;
    const Aff* T = gen_table();
    long bad = 0;
#pragma omp parallel for schedule(dynamic, 4) reduction(+ : bad)
    for (long long i = 0; i < (long long)count; i++) {
        err[i] = body_sp_scan(T, scan_sk32, spend_pkx32, spend_pky32, label_x32, label_y32, (u32)n_labels, ax32, ay32, input_hash32, outputs32,
                              out_offsets, (u32)max_hits, n_hits, hit_output, hit_label, hit_tweak32, (size_t)i);
        bad += err[i] != 0;
    }
    return bad;
}

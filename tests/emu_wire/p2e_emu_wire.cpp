// CPU harness of the key and signature codec bodies (test infrastructure only): body_point_decode, body_point_encode,
// body_sig_decode and body_sig_encode of csrc/wire.hpp run per element, compiled with g++ against the library's headers, on
// either curve.  Each call returns the number of flagged elements, or -1 for arguments the library refuses.
#include <cstdint>

#include "../../plonky2-ecdsa_amd/csrc/wire.hpp"

using namespace p2e;

namespace {
template <class CV>
long run_sig_decode(int form, unsigned flags, const uint8_t* data, const uint64_t* offsets, uint8_t* r, uint8_t* s, uint8_t* v, size_t n,
                    uint8_t* err) {
    long bad = 0;
#pragma omp parallel for schedule(dynamic, 64) reduction(+ : bad)
    for (long long i = 0; i < (long long)n; i++) {
        if (form == SIG_DER) err[i] = body_sig_decode<CV, SIG_DER>(flags, data, offsets, r, s, v, (size_t)i);
        if (form == SIG_COMPACT64) err[i] = body_sig_decode<CV, SIG_COMPACT64>(flags, data, offsets, r, s, v, (size_t)i);
        if (form == SIG_COMPACT65) err[i] = body_sig_decode<CV, SIG_COMPACT65>(flags, data, offsets, r, s, v, (size_t)i);
        bad += err[i] != 0;
    }
    return bad;
}
template <class CV>
long run_sig_encode(int form, unsigned flags, const uint8_t* r, const uint8_t* s, const uint8_t* v, uint8_t* out, uint8_t* out_len, size_t n,
                    uint8_t* err) {
    long bad = 0;
#pragma omp parallel for schedule(dynamic, 64) reduction(+ : bad)
    for (long long i = 0; i < (long long)n; i++) {
        if (form == SIG_DER) err[i] = body_sig_encode<CV, SIG_DER>(flags, r, s, v, out, out_len, (size_t)i);
        if (form == SIG_COMPACT64) err[i] = body_sig_encode<CV, SIG_COMPACT64>(flags, r, s, v, out, out_len, (size_t)i);
        if (form == SIG_COMPACT65) err[i] = body_sig_encode<CV, SIG_COMPACT65>(flags, r, s, v, out, out_len, (size_t)i);
        bad += err[i] != 0;
    }
    return bad;
}
bool bad_form(int form) { return form != SIG_DER && form != SIG_COMPACT64 && form != SIG_COMPACT65; }
}  // namespace

extern "C" long emuw_point_decode(int curve, const uint8_t* data, const uint64_t* offsets, uint8_t* px, uint8_t* py, size_t n, uint8_t* err) {
    if (curve != 0 && curve != 1) return -1;
    long bad = 0;
#pragma omp parallel for schedule(dynamic, 16) reduction(+ : bad)
    for (long long i = 0; i < (long long)n; i++) {
        err[i] = curve == 0 ? body_point_decode<Secp256k1>(data, offsets, px, py, (size_t)i) : body_point_decode<P256>(data, offsets, px, py, (size_t)i);
        bad += err[i] != 0;
    }
    return bad;
}
extern "C" long emuw_point_encode(int curve, int form, const uint8_t* px, const uint8_t* py, uint8_t* out, size_t n, uint8_t* err) {
    if ((curve != 0 && curve != 1) || (form != SEC1_COMPRESSED && form != SEC1_UNCOMPRESSED)) return -1;
    long bad = 0;
#pragma omp parallel for schedule(dynamic, 64) reduction(+ : bad)
    for (long long i = 0; i < (long long)n; i++) {
        if (curve == 0)
            err[i] = form == SEC1_COMPRESSED ? body_point_encode<Secp256k1, SEC1_COMPRESSED>(px, py, out, (size_t)i)
                                             : body_point_encode<Secp256k1, SEC1_UNCOMPRESSED>(px, py, out, (size_t)i);
        else
            err[i] = form == SEC1_COMPRESSED ? body_point_encode<P256, SEC1_COMPRESSED>(px, py, out, (size_t)i)
                                             : body_point_encode<P256, SEC1_UNCOMPRESSED>(px, py, out, (size_t)i);
        bad += err[i] != 0;
    }
    return bad;
}
extern "C" long emuw_sig_decode(int curve, int form, unsigned flags, const uint8_t* data, const uint64_t* offsets, uint8_t* r, uint8_t* s,
                                uint8_t* v, size_t n, uint8_t* err) {
    if ((curve != 0 && curve != 1) || bad_form(form) || flags > 2) return -1;
    return curve == 0 ? run_sig_decode<Secp256k1>(form, flags, data, offsets, r, s, v, n, err)
                      : run_sig_decode<P256>(form, flags, data, offsets, r, s, v, n, err);
}
extern "C" long emuw_sig_encode(int curve, int form, unsigned flags, const uint8_t* r, const uint8_t* s, const uint8_t* v, uint8_t* out,
                                uint8_t* out_len, size_t n, uint8_t* err) {
    if ((curve != 0 && curve != 1) || bad_form(form) || (flags != 0 && flags != SIG_NORMALIZE_S)) return -1;
    return curve == 0 ? run_sig_encode<Secp256k1>(form, flags, r, s, v, out, out_len, n, err)
                      : run_sig_encode<P256>(form, flags, r, s, v, out, out_len, n, err);
}

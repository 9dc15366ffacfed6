// Keys and signatures in the forms other programs read and write, one lane per element, on either curve:
//   SEC1 2.3.3 / 2.3.4 public keys (00 | 02 x | 03 x | 04 x y, big-endian)            body_point_decode / body_point_encode
//   ECDSA signatures as strict DER (BIP-66's rules), as r || s and as r || s || v      body_sig_decode / body_sig_encode
// The reference has no counterpart: its keys and signatures are field elements (curve/ecdsa.rs:7-23).  Everything on the
// library's side of these calls is the 32-byte little-endian form of every other entry point.
//
// Codes, not bits.  err[i] is the WIRE_* code of the FIRST failing check, in the order include/p2e.h lists them (the error
// byte's bits are all taken).  A flagged element writes zeros to every output.
//
// Reads.  An element of a variable-length batch is data[offsets[i], offsets[i + 1]) as in hash.hpp and is reached through
// the same MsgView: aligned 32-bit words, and only words that hold a byte of the lane's own element.  A wrong length is
// decided from the offsets alone and reads nothing.  Inside an element a field is fetched only once the checks before it
// have admitted the bytes it occupies (the prefix before the coordinates; b[0], b[1] before b[2], b[3]; the second tag
// and length only when lr keeps them inside the element; the integers last).  A DER field's position is a run-time value:
// it is fetched with loads at computed addresses (wire_byte, wire_be32), never by indexing a register array.
//
// Writes.  The wire outputs have strides 33, 65, 64, 65 and 72 and no alignment: they are written with byte stores, each
// from a register named at compile time (a DER integer's bytes go to a computed ADDRESS).  Nothing lives in the private
// segment, no LDS is used.
//
// The square root of a compressed key is recover.hpp's recover_decompress<CV>, unchanged; the curve test of the
// uncompressed forms is pmsm.hpp's msm_on_curve<CV>.
#pragma once
#include "hash.hpp"
#include "pmsm.hpp"
#include "recover.hpp"

namespace p2e {

// include/p2e.h P2E_WIRE_*
constexpr uint8_t WIRE_OK = 0, WIRE_BAD_LENGTH = 1, WIRE_BAD_PREFIX = 2, WIRE_COORD_RANGE = 3, WIRE_NOT_ON_CURVE = 4, WIRE_INFINITY = 5,
                  WIRE_DER_SYNTAX = 6, WIRE_DER_INTEGER = 7, WIRE_SCALAR_RANGE = 8, WIRE_HIGH_S = 9;
constexpr int SEC1_COMPRESSED = 0, SEC1_UNCOMPRESSED = 1;           // include/p2e.h P2E_SEC1_*
constexpr int SIG_DER = 0, SIG_COMPACT64 = 1, SIG_COMPACT65 = 2;    // include/p2e.h P2E_SIG_*
constexpr unsigned SIG_REQUIRE_LOW_S = 1, SIG_NORMALIZE_S = 2;      // include/p2e.h P2E_SIG_REQUIRE_LOW_S / _NORMALIZE_S
constexpr int SIG_DER_STRIDE = 72, SIG_DER_MIN = 8;

// ---------------------------------------------------------------------------------------------------------------------
// fetches from one element (all positions relative to its first byte; the caller keeps them inside the element)
// ---------------------------------------------------------------------------------------------------------------------
P2E_HD MsgView wire_view(const uint8_t* first, u64 len) {   // len > 0
    const uintptr_t a = (uintptr_t)first;
    MsgView m;
    m.len = len;
    m.p = reinterpret_cast<const u32*>(a & ~(uintptr_t)3);
    m.sh = 8u * (u32)(a & 3u);
    m.end = a + len;
    return m;
}
P2E_HD u32 wire_byte(const MsgView& m, u32 pos) {
    const u32 a = (m.sh >> 3) + pos;
    return (m.word(a >> 2) >> (8u * (a & 3u))) & 0xFFu;
}
// bytes pos .. pos + 3 as a big-endian number
P2E_HD u32 wire_be32(const MsgView& m, u32 pos) {
    const u32 a = (m.sh >> 3) + pos, k = a >> 2, sh = 8u * (a & 3u);
    const u32 lo = m.word(k);
    const u32 hi = sh ? m.word(k + 1) : 0u;   // (the next word holds byte pos + 3 or nothing that is wanted)
    return hash_bswap32(hash_join(lo, hi, sh));
}
// bytes pos .. pos + 31 as a big-endian number: nine aligned words, eight where the field is aligned
P2E_HD U256 wire_be256(const MsgView& m, u32 pos) {
    const u32 a = (m.sh >> 3) + pos, k = a >> 2, sh = 8u * (a & 3u);
    U256 r;
    u32 carry = m.word(k);
    P2E_UNROLL
    for (int j = 0; j < 8; j++) {
        const u32 next = (j < 7 || sh) ? m.word(k + j + 1) : 0u;
        r.w[7 - j] = hash_bswap32(hash_join(carry, next, sh));
        carry = next;
    }
    return r;
}
// the DER integer of `len` bytes (1 .. 33) at `pos`, its low 256 bits: word j holds the bytes len - 4 j - 4 .. len - 4 j - 1
// of the integer where it has them.  (pos >= 4, so pos + len - 4 j - 4 > 0 whenever len > 4 j: no fetch in front of the element.)
P2E_HD U256 wire_der_int(const MsgView& m, u32 pos, u32 len) {
    U256 r;
    P2E_UNROLL
    for (int j = 0; j < 8; j++) {
        u32 v = 0;
        if (len > 4u * j) {
            const u32 have = len - 4u * j;   // bytes of the integer at and above this word's lowest one
            v = wire_be32(m, pos + len - 4u * j - 4u);
            if (have < 4u) v &= (1u << (8u * have)) - 1u;
        }
        r.w[j] = v;
    }
    return r;
}
// 32 big-endian bytes of v at p (any alignment)
P2E_HD void wire_store_be256(uint8_t* p, const U256& v) {
    P2E_UNROLL
    for (int j = 0; j < 32; j++) p[j] = (uint8_t)(v.w[7 - j / 4] >> (8 * (3 - j % 4)));
}
P2E_HD void wire_store_zero(uint8_t* p, int count) {
    for (int j = 0; j < count; j++) p[j] = 0;
}

// s > (n - 1) / 2 for 0 < s < n, and the twin n - s
template <class CV>
P2E_HD bool wire_high_s(const U256& s, U256& twin) {
    twin = fe_neg<typename CV::Fn>(s);
    return !geq_n<8>(twin.w, s.w);   // n is odd: n - s != s
}
template <class CV>
P2E_HD bool wire_scalar_ok(const U256& a) {
    return !u256_is_zero(a) && !geq_mod<typename CV::Fn>(a.w);
}

// ---------------------------------------------------------------------------------------------------------------------
// bodies of the four kernels: element i; each returns the element's code
// ---------------------------------------------------------------------------------------------------------------------
template <class CV>
P2E_HD uint8_t body_point_decode(const uint8_t* data, const uint64_t* offsets, uint8_t* px32, uint8_t* py32, size_t i) {
    typedef typename CV::Fp F;
    const u64 lo = offsets[i], hi = offsets[i + 1];
    const u64 len = hi < lo ? 0 : hi - lo;
    uint8_t e = WIRE_OK;
    U256 x = u256_zero(), y = u256_zero();
    if (len != 1 && len != 33 && len != 65) {
        e = WIRE_BAD_LENGTH;
    } else {
        const MsgView m = wire_view(data + lo, len);
        const u32 prefix = wire_byte(m, 0);
        if (len == 1) {
            e = prefix == 0 ? WIRE_INFINITY : WIRE_BAD_PREFIX;
        } else if (len == 33 ? (prefix != 2 && prefix != 3) : prefix != 4) {
            e = WIRE_BAD_PREFIX;
        } else {
            x = wire_be256(m, 1);
            if (len == 65) y = wire_be256(m, 33);
            if (geq_mod<F>(x.w) || (len == 65 && geq_mod<F>(y.w))) {
                e = WIRE_COORD_RANGE;
            } else if (len == 33) {
                Aff R;
                if (!recover_decompress<CV>(x, (prefix & 1u) != 0, R)) e = WIRE_NOT_ON_CURVE;
                y = R.y;
            } else if (!msm_on_curve<CV>(x, y)) {
                e = WIRE_NOT_ON_CURVE;
            }
        }
    }
    if (e) x = y = u256_zero();
    store_packed(px32, i, x);
    store_packed(py32, i, y);
    return e;
}

template <class CV, int FORM>
P2E_HD uint8_t body_point_encode(const uint8_t* px32, const uint8_t* py32, uint8_t* out, size_t i) {
    constexpr int STRIDE = FORM == SEC1_COMPRESSED ? 33 : 65;
    const U256 x = load_packed(px32, i), y = load_packed(py32, i);
    uint8_t* p = out + (size_t)STRIDE * i;
    uint8_t e = WIRE_OK;
    if (u256_is_zero(x) && u256_is_zero(y))
        e = WIRE_INFINITY;
    else if (geq_mod<typename CV::Fp>(x.w) || geq_mod<typename CV::Fp>(y.w))
        e = WIRE_COORD_RANGE;
    else if (!msm_on_curve<CV>(x, y))
        e = WIRE_NOT_ON_CURVE;
    if (e) {
        wire_store_zero(p, STRIDE);
        return e;
    }
    p[0] = FORM == SEC1_COMPRESSED ? (uint8_t)(2u | (y.w[0] & 1u)) : (uint8_t)4;
    wire_store_be256(p + 1, x);
    if (FORM == SEC1_UNCOMPRESSED) wire_store_be256(p + 33, y);
    return e;
}

// v8 nullable (looked at in COMPACT65 only); offsets is DER's alone
template <class CV, int FORM>
P2E_HD uint8_t body_sig_decode(unsigned flags, const uint8_t* data, const uint64_t* offsets, uint8_t* r32, uint8_t* s32, uint8_t* v8,
                               size_t i) {
    uint8_t e = WIRE_OK;
    U256 r = u256_zero(), s = u256_zero();
    u32 v = 0;
    bool over = false;   // an integer of 33 bytes whose first byte is not 0: >= 2^256
    if (FORM == SIG_DER) {
        const u64 lo = offsets[i], hi = offsets[i + 1];
        const u64 len = hi < lo ? 0 : hi - lo;
        if (len < (u64)SIG_DER_MIN || len > (u64)SIG_DER_STRIDE) {
            e = WIRE_BAD_LENGTH;
        } else {
            const MsgView m = wire_view(data + lo, len);
            const u32 L = (u32)len;
            u32 lr = 0, ls = 0;
            if (wire_byte(m, 0) != 0x30u || wire_byte(m, 1) != L - 2u) {
                e = WIRE_DER_SYNTAX;
            } else {
                lr = wire_byte(m, 3);
                if (wire_byte(m, 2) != 0x02u || lr == 0 || lr > 33u || lr + 7u > L) e = WIRE_DER_SYNTAX;
            }
            if (!e) {
                ls = wire_byte(m, 5u + lr);
                if (wire_byte(m, 4u + lr) != 0x02u || ls == 0 || ls > 33u || lr + ls + 6u != L) e = WIRE_DER_SYNTAX;
            }
            if (!e) {
                const u32 r0 = wire_byte(m, 4), s0 = wire_byte(m, 6u + lr);
                const bool r_padded = lr > 1u && r0 == 0 && wire_byte(m, 5) < 0x80u;
                const bool s_padded = ls > 1u && s0 == 0 && wire_byte(m, 7u + lr) < 0x80u;
                if (r0 >= 0x80u || r_padded || s0 >= 0x80u || s_padded) {
                    e = WIRE_DER_INTEGER;
                } else {
                    r = wire_der_int(m, 4, lr);
                    s = wire_der_int(m, 6u + lr, ls);
                    over = (lr == 33u && r0 != 0) || (ls == 33u && s0 != 0);
                }
            }
        }
    } else {
        constexpr u32 STRIDE = FORM == SIG_COMPACT64 ? 64 : 65;
        const MsgView m = wire_view(data + (size_t)STRIDE * i, STRIDE);
        r = wire_be256(m, 0);
        s = wire_be256(m, 32);
        if (FORM == SIG_COMPACT65) v = wire_byte(m, 64);
    }
    if (!e) {
        if (over || !wire_scalar_ok<CV>(r) || !wire_scalar_ok<CV>(s)) {
            e = WIRE_SCALAR_RANGE;
        } else if (flags) {
            U256 twin;
            if (wire_high_s<CV>(s, twin)) {
                if (flags & SIG_REQUIRE_LOW_S) {
                    e = WIRE_HIGH_S;
                } else {
                    s = twin;
                    v ^= 1u;
                }
            }
        }
    }
    if (e) {
        r = s = u256_zero();
        v = 0;
    }
    store_packed(r32, i, r);
    store_packed(s32, i, s);
    if (FORM == SIG_COMPACT65 && v8) v8[i] = (uint8_t)v;
    return e;
}

// minimal length in bytes of the DER integer of a (non-zero): its bytes plus a 00 in front where the top bit is set
P2E_HD u32 wire_der_len(const U256& a) {
    u32 bits = 0;
    P2E_UNROLL
    for (int k = 0; k < 8; k++)
        if (a.w[k]) bits = 32u * k + 32u - (u32)__builtin_clz(a.w[k]);
    return bits / 8u + 1u;
}
// tag, length and the `len` bytes of the integer at p; returns len + 2
P2E_HD u32 wire_store_der_int(uint8_t* p, const U256& a) {
    const u32 len = wire_der_len(a);
    p[0] = 0x02;
    p[1] = (uint8_t)len;
    if (len == 33u) p[2] = 0;
    P2E_UNROLL
    for (int j = 0; j < 33; j++) {                        // byte j of the 33-byte big-endian form 00 || a
        if (j == 0) continue;                             // (written above where it is wanted)
        const uint8_t b = (uint8_t)(a.w[7 - (j - 1) / 4] >> (8 * (3 - (j - 1) % 4)));
        if ((u32)j + len >= 33u) p[2u + (u32)j + len - 33u] = b;
    }
    return len + 2u;
}

// v8: COMPACT65's input; out_len: DER's output
template <class CV, int FORM>
P2E_HD uint8_t body_sig_encode(unsigned flags, const uint8_t* r32, const uint8_t* s32, const uint8_t* v8, uint8_t* out, uint8_t* out_len,
                               size_t i) {
    constexpr int STRIDE = FORM == SIG_DER ? SIG_DER_STRIDE : FORM == SIG_COMPACT64 ? 64 : 65;
    const U256 r = load_packed(r32, i);
    U256 s = load_packed(s32, i);
    u32 v = FORM == SIG_COMPACT65 ? v8[i] : 0u;
    uint8_t* p = out + (size_t)STRIDE * i;
    if (!wire_scalar_ok<CV>(r) || !wire_scalar_ok<CV>(s)) {
        wire_store_zero(p, STRIDE);
        if (FORM == SIG_DER) out_len[i] = 0;
        return WIRE_SCALAR_RANGE;
    }
    if (flags & SIG_NORMALIZE_S) {
        U256 twin;
        if (wire_high_s<CV>(s, twin)) {
            s = twin;
            v ^= 1u;
        }
    }
    if (FORM == SIG_DER) {
        const u32 nr = wire_store_der_int(p + 2, r);
        const u32 ns = wire_store_der_int(p + 2 + nr, s);
        const u32 total = 2u + nr + ns;
        p[0] = 0x30;
        p[1] = (uint8_t)(total - 2u);
        for (u32 k = total; k < (u32)SIG_DER_STRIDE; k++) p[k] = 0;
        out_len[i] = (uint8_t)total;
    } else {
        wire_store_be256(p, r);
        wire_store_be256(p + 32, s);
        if (FORM == SIG_COMPACT65) p[64] = (uint8_t)v;
    }
    return WIRE_OK;
}

#if defined(__HIPCC__)
// thread g owns element g
template <class CV>
__global__ __launch_bounds__(256) void k_point_decode(const uint8_t* data, const uint64_t* offsets, uint8_t* px32, uint8_t* py32, size_t n,
                                                      uint8_t* err, unsigned long long* counter) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    uint8_t e = 0;
    if (i < n) {
        e = body_point_decode<CV>(data, offsets, px32, py32, i);
        err[i] = e;
    }
    sign_count_err(e, counter);
}
template <class CV, int FORM>
__global__ __launch_bounds__(256) void k_point_encode(const uint8_t* px32, const uint8_t* py32, uint8_t* out, size_t n, uint8_t* err,
                                                      unsigned long long* counter) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    uint8_t e = 0;
    if (i < n) {
        e = body_point_encode<CV, FORM>(px32, py32, out, i);
        err[i] = e;
    }
    sign_count_err(e, counter);
}
template <class CV, int FORM>
__global__ __launch_bounds__(256) void k_sig_decode(unsigned flags, const uint8_t* data, const uint64_t* offsets, uint8_t* r32, uint8_t* s32,
                                                    uint8_t* v8, size_t n, uint8_t* err, unsigned long long* counter) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    uint8_t e = 0;
    if (i < n) {
        e = body_sig_decode<CV, FORM>(flags, data, offsets, r32, s32, v8, i);
        err[i] = e;
    }
    sign_count_err(e, counter);
}
template <class CV, int FORM>
__global__ __launch_bounds__(256) void k_sig_encode(unsigned flags, const uint8_t* r32, const uint8_t* s32, const uint8_t* v8, uint8_t* out,
                                                    uint8_t* out_len, size_t n, uint8_t* err, unsigned long long* counter) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    uint8_t e = 0;
    if (i < n) {
        e = body_sig_encode<CV, FORM>(flags, r32, s32, v8, out, out_len, i);
        err[i] = e;
    }
    sign_count_err(e, counter);
}
#endif

}  // namespace p2e
